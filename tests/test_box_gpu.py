"""captra_part_box_hist (csrc/pose_box.hip) through the C ABI on sentinel-filled outputs against the integer / float32 judge of
tests/box_judge.py: every output -- the histograms, the held and the frame's extents, the member and the held counts -- with
torch.equal.  Both LDS forms of the kernel (one histogram per workgroup, one per wave) run every shape."""
import numpy as np
import pytest

from tests import box_judge as J

B = 3
SIZES = (1, 63, 64, 65, 130, 1000)
SENT_F, SENT_I = float("nan"), -7
OUT_KEYS = ("hist", "extent", "frame", "added", "total")
_FIX = {}


def make_case(P, N, bins, seed):
    """labels (B,N) with labels outside [0, P), src (B,P,3,N) with the edge values planted at random places, a state with negative
    cells, the four verdict codes.  Built once per key and never modified."""
    key = (P, N, bins, seed)
    if key in _FIX:
        return _FIX[key]
    rng = np.random.default_rng(seed)
    labels = rng.integers(-1, P + 1, size=(B, N)).astype(np.int32)
    src = rng.uniform(-0.6, 0.6, size=(B, P, 3, N)).astype(np.float32)
    edges = np.arange(bins + 1, dtype=np.float32) / np.float32(bins)           # exact bin edges, 1.0 included
    rare = np.float32([0.0, -0.0, 1.0, -1.0, 1.5, -3.0, 3e19, -3e19, 1e-40, np.nextafter(np.float32(1), np.float32(0)), np.nan, np.inf, -np.inf])
    flat = src.reshape(-1)
    where = rng.random(flat.shape) < 0.3                               # three coordinates of ten: half of them bin edges, half the rare values
    picks = np.where(rng.random(int(where.sum())) < 0.5, rng.choice(np.concatenate([edges, -edges]), size=int(where.sum())),
                     rng.choice(rare, size=int(where.sum())))
    flat[where] = picks
    hist_in = rng.integers(-5, 40, size=(B, P, 3, bins)).astype(np.int32)
    verdict = rng.integers(0, 4, size=(B, P)).astype(np.int32)
    _FIX[key] = dict(labels=labels, src=src, hist_in=hist_in, verdict=verdict, bins=bins)
    return _FIX[key]


def _dev(a, device):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _abi(device, labels, src, hist_in, verdict, bins, radial, permille, min_points, alias=False, null=(), shape=None):
    """The C ABI on sentinel-filled outputs -> (err, dict of CPU tensors).  alias: hist_out IS hist_in's buffer."""
    import torch
    from captra_amd import _lib as L
    Bn, P, _, N = src.shape
    d = dict(labels=_dev(labels, device), src=_dev(src, device), verdict=_dev(verdict, device), hist_in=_dev(hist_in, device))
    out = {"hist": d["hist_in"] if alias else torch.full((Bn, P, 3, bins if bins in J.BINS else 64), SENT_I, dtype=torch.int32, device=device),
           "extent": torch.full((Bn, P, 3), SENT_F, device=device), "frame": torch.full((Bn, P, 3), SENT_F, device=device),
           "added": torch.full((Bn, P), SENT_I, dtype=torch.int32, device=device), "total": torch.full((Bn, P), SENT_I, dtype=torch.int32, device=device)}
    ptr = lambda name, t: None if name in null else L.ptr(t)          # noqa: E731
    b_, p_, n_ = shape if shape is not None else (Bn, P, N)
    with torch.cuda.device(device):
        err = L.lib().captra_part_box_hist(b_, p_, n_, bins, radial, permille, min_points, ptr("labels", d["labels"]), ptr("src", d["src"]),
                                           L.ptr(d["verdict"]), L.ptr(d["hist_in"]), *(ptr(k, out[k]) for k in OUT_KEYS), L.stream_ptr())
    torch.cuda.synchronize(device)
    return err, {k: v.cpu() for k, v in out.items()}


def _untouched(got):
    return all(bool(torch_isnan(got[k]).all()) if k in ("extent", "frame") else bool((got[k] == SENT_I).all()) for k in OUT_KEYS)


def torch_isnan(t):
    import torch
    return torch.isnan(t)


def _equal(got, want, what):
    import torch
    for k in OUT_KEYS:
        w = torch.from_numpy(want[k])
        assert got[k].dtype == w.dtype and torch.equal(got[k], w), (what, k, got[k].flatten()[:12], w.flatten()[:12])


class _Subhists:
    """The calling thread's choice of the kernel's LDS form for the block (0 = the default again on exit)."""

    def __init__(self, sub):
        self.sub = sub

    def __enter__(self):
        from captra_amd import _lib as L
        L.lib().captra_part_box_set_subhists(self.sub)

    def __exit__(self, *a):
        from captra_amd import _lib as L
        L.lib().captra_part_box_set_subhists(0)


# ================================================================================================================== 1. the shapes
@pytest.mark.gpu
@pytest.mark.parametrize("sub", [1, 4])
@pytest.mark.parametrize("radial", [0, 1])
@pytest.mark.parametrize("bins", [64, 512])
@pytest.mark.parametrize("P", [1, 2, 4])
def test_box_hist_shapes(device, P, bins, radial, sub):
    with _Subhists(sub):
        for N in SIZES:
            c = make_case(P, N, bins, 100 * P + N + bins)
            for permille, min_points in ((950, 16), (500, 1), (1000, 1)):
                err, got = _abi(device, c["labels"], c["src"], c["hist_in"], c["verdict"], bins, radial, permille, min_points)
                assert err == 0
                want = J.judge_batch(c["labels"], c["src"], c["hist_in"], c["verdict"], bins, bool(radial), permille, min_points)
                _equal(got, want, (P, N, bins, radial, sub, permille))
    # the planted values took part: non-finite coordinates kept points out, values >= 1 filled the last bin
    c = make_case(P, 1000, bins, 100 * P + 1000 + bins)
    members = sum(int(((c["labels"][b] == q) & np.isfinite(c["src"][b, q]).all(0)).sum()) for b in range(B) for q in range(P))
    labelled = int(((c["labels"] >= 0) & (c["labels"] < P)).sum())
    assert 0 < members < labelled < B * 1000
    assert J.frame_hist(c["labels"][0], c["src"][0, 0], 0, bins, False)[0][:, bins - 1].min() > 0


# ================================================================================================================ 2. edge inputs
@pytest.mark.gpu
@pytest.mark.parametrize("radial", [0, 1])
def test_box_hist_edge_inputs(device, radial):
    bins, N, P = 128, 200, 2
    labels = np.zeros((B, N), np.int32)
    labels[1] = np.arange(N) % 2
    labels[2] = np.where(np.arange(N) % 3 == 0, 7, np.where(np.arange(N) % 3 == 1, -1, 1))      # labels outside [0, P); part 0 of b = 2 is empty
    src = np.full((B, P, 3, N), 0.3, np.float32)                       # b = 0: every member in one bin; its part 1 is empty
    edges = (np.arange(N) % (bins + 1)).astype(np.float32) / np.float32(bins)
    src[1, 0] = np.stack([edges, -edges, edges])                       # coordinates exactly on bin edges, 0 and 1 included
    # part 1 of b = 1 is the odd points, in four kinds
    src[1, 1, :, 1::8] = np.float32([[1.0], [-1.5], [2.0]])            # coordinates >= 1
    src[1, 1, 0, 3::8], src[1, 1, 1, 3::8], src[1, 1, 2, 3::8] = 0.0, -0.0, 0.0
    src[1, 1, 0, 5::8], src[1, 1, 2, 5::8] = -edges[5::8], -0.0        # r = |x| exactly: on a bin edge only if the root is rounded correctly
    m = (np.arange(len(edges[7::8])) % 25 + 1).astype(np.float32)
    src[1, 1, 0, 7::8], src[1, 1, 2, 7::8] = 3 * m / np.float32(bins), -4 * m / np.float32(bins)     # r = 5 m / bins exactly
    # part 1 of b = 2 is the points 2, 5, 8, ... (mod 3)
    src[2, 1, 0, 2::18], src[2, 1, 1, 5::18], src[2, 1, 2, 8::18] = np.nan, np.inf, -np.inf      # not members
    src[2, 1, 0, 11::18] = 3e19                                        # x x overflows: r = Inf, the last bin
    src[2, 1, 2, 14::18] = 1e-30                                       # z z underflows to 0
    err, got = _abi(device, labels, src, None, None, bins, radial, 900, 1)
    assert err == 0
    want = J.judge_batch(labels, src, None, None, bins, bool(radial), 900, 1)
    _equal(got, want, ("edges", radial))
    # what the fixture was built for, in the judge's numbers
    assert want["added"][0].tolist() == [N, 0] and want["added"][2, 0] == 0 and 0 < want["added"][2, 1] < (labels[2] == 1).sum()
    assert (want["extent"][0, 1] == 0).all() and (want["extent"][2, 0] == 0).all() and not want["hist"][0, 1].any()
    one_bin = int(np.float32(0.3) * bins) if not radial else int(J.bin_of(J.axis_values([[0.3, 0.3, 0.3]], True)[0, 0], bins))
    assert want["hist"][0, 0, 0, one_bin] == N and (want["extent"][0, 0, 0] == np.float32(one_bin + 1) / np.float32(bins))
    assert want["extent"][1, 1].max() == 1.0 and want["hist"][1, 1, :, bins - 1].min() > 0
    assert want["hist"][2, 1, 0, bins - 1] > 0


# ========================================================================================================== 3. read-out and state
@pytest.mark.gpu
def test_box_hist_read_out_and_state(device):
    import torch
    bins, N, P = 64, 130, 2
    c = make_case(P, N, bins, 77)
    labels, src = c["labels"], c["src"]
    zeros = np.zeros((B, P, 3, bins), np.int32)
    ref = J.judge_batch(labels, src, None, None, bins, False, 950, 1)
    # hist_in NULL is an empty state
    for hist_in in (None, zeros):
        err, got = _abi(device, labels, src, hist_in, None, bins, 0, 950, 1)
        assert err == 0
        _equal(got, ref, "empty state")
    # min_points just at T and just above it, per (b, q): established exactly where T >= min_points
    T = ref["total"]
    for b in range(B):
        for q in range(P):
            t = int(T[b, q])
            assert t >= 2
            for mp in (t, t + 1):
                err, got = _abi(device, labels, src, None, None, bins, 0, 950, mp)
                assert err == 0
                _equal(got, J.judge_batch(labels, src, None, None, bins, False, 950, mp), ("min_points", mp))
                assert bool((got["extent"][b, q] > 0).all()) == (mp == t) and bool((got["frame"][b, q] > 0).all()) == (mp == t)
    # hist_out aliasing hist_in
    err, got = _abi(device, labels, src, c["hist_in"].copy(), c["verdict"], bins, 0, 950, 16, alias=True)
    assert err == 0
    _equal(got, J.judge_batch(labels, src, c["hist_in"], c["verdict"], bins, False, 950, 16), "aliased")
    # a state whose T * permille does not fit 32 bits, and a cell at 2^31 - 10 that saturates
    big = np.zeros((B, P, 3, bins), np.int32)
    big[:, :, :, 10] = 3_000_000
    big[0, 0, :, 40] = 2 ** 31 - 10
    big[1, 1, 1, :] = 2 ** 31 - 1                    # T of an axis beyond 2^31: total is axis 0's, clamped; the read-out is exact in 64 bits
    big[2, 0, 0, :] = 2 ** 31 - 1
    crowd_labels = np.zeros((B, N), np.int32)
    crowd = np.full((B, P, 3, N), np.float32(40.5 / 64), np.float32)          # 130 members of part 0 into bin 40
    for permille in (950, 1000, 500):
        err, got = _abi(device, crowd_labels, crowd, big, None, bins, 0, permille, 16)
        assert err == 0
        want = J.judge_batch(crowd_labels, crowd, big, None, bins, False, permille, 16)
        _equal(got, want, ("wide", permille))
    assert want["hist"][0, 0, 0, 40] == 2 ** 31 - 1 and want["total"][2, 0] == 2 ** 31 - 1 and want["total"][1, 0] == 3_000_000 + N
    assert (J.judge_batch(crowd_labels, crowd, big, None, bins, False, 950, 16, mutate="product_32bit")["extent"] != want["extent"]).any()
    assert torch.equal(got["hist"][1, 1], torch.from_numpy(big[1, 1]))        # (no member of part 1: the state passes through)


# ================================================================================================================= 4. the verdicts
@pytest.mark.gpu
def test_box_hist_verdicts(device):
    import torch
    bins, N, P = 64, 65, 4
    c = make_case(P, N, bins, 9)
    labels = (np.arange(N) % P).astype(np.int32)[None].repeat(B, 0)
    state = np.abs(c["hist_in"])
    verdict = np.array([[0, 1, 2, 3], [3, 2, 1, 0], [2, 2, 0, 0]], np.int32)
    err, got = _abi(device, labels, c["src"], state, verdict, bins, 0, 950, 16)
    assert err == 0
    want = J.judge_batch(labels, c["src"], state, verdict, bins, False, 950, 16)
    _equal(got, want, "verdicts")
    counts = np.isin(verdict, (0, 3))
    assert torch.equal(got["hist"][torch.from_numpy(~counts)], torch.from_numpy(state[~counts]))      # lost / too_few: the state as it is
    assert (want["hist"][counts].astype(np.int64).sum((1, 2)) > state[counts].astype(np.int64).sum((1, 2))).all()
    assert (want["added"] > 0).all()                                   # ... while the frame's own record is written all the same
    # no verdict: every frame counts
    err, got = _abi(device, labels, c["src"], state, None, bins, 0, 950, 16)
    assert err == 0
    _equal(got, J.judge_batch(labels, c["src"], state, None, bins, False, 950, 16), "no verdict")
    assert (J.judge_batch(labels, c["src"], state, verdict, bins, False, 950, 16, mutate="accumulate_lost")["hist"] != want["hist"]).any()


# ============================================================================================================ 5. refused arguments
@pytest.mark.gpu
def test_box_hist_refused_arguments(device):
    c = make_case(2, 65, 64, 5)
    args = (c["labels"], c["src"], c["hist_in"], c["verdict"])
    good = dict(bins=64, radial=0, permille=950, min_points=16)
    refused = [dict(bins=b) for b in (0, 32, 63, 100, 1024, -64)]
    refused += [dict(permille=q) for q in (499, 1001, 0, -1)] + [dict(min_points=0), dict(min_points=-3)]
    refused += [dict(shape=s) for s in ((0, 2, 65), (-1, 2, 65), (3, 0, 65), (3, 9, 65), (3, 2, 0), (3, 2, -5))]
    refused += [dict(null=(k,)) for k in ("labels", "src") + OUT_KEYS]
    for kw in refused:
        err, got = _abi(device, *args, **{**good, **kw})
        assert err == -1 and _untouched(got), kw
    err, got = _abi(device, *args, **good)
    assert err == 0 and not _untouched(got)


# ======================================================================================================================= 6. wrapper
@pytest.mark.gpu
def test_box_hist_wrapper(device):
    """part_box_hist returns the ABI's bits, leaves the state it was given alone and takes None for a track's start."""
    import torch
    from captra_amd.pose_utils.pose_fit import part_box_hist
    c = make_case(4, 1000, 128, 11)
    state = _dev(c["hist_in"], device)
    new, info = part_box_hist(_dev(c["labels"], device), _dev(c["src"], device), state, bins=128, radial=True, quantile_permille=900, min_points=16,
                              verdict=_dev(c["verdict"], device))
    err, got = _abi(device, c["labels"], c["src"], c["hist_in"], c["verdict"], 128, 1, 900, 16)
    assert err == 0 and set(info) == {"extent", "frame", "added", "total"} and new.data_ptr() != state.data_ptr()
    assert torch.equal(state.cpu(), torch.from_numpy(c["hist_in"]))
    for k, t in (("hist", new), ("extent", info["extent"]), ("frame", info["frame"]), ("added", info["added"]), ("total", info["total"])):
        assert torch.equal(t.cpu(), got[k]), k
    new0, info0 = part_box_hist(_dev(c["labels"], device), _dev(c["src"], device), None, bins=128, radial=False, quantile_permille=900, min_points=16)
    want = J.judge_batch(c["labels"], c["src"], None, None, 128, False, 900, 16)
    assert torch.equal(new0.cpu(), torch.from_numpy(want["hist"])) and torch.equal(info0["extent"].cpu(), torch.from_numpy(want["extent"]))
