"""captra_part_fit_st_size (csrc/pose_size.hip) through the C ABI on sentinel-filled outputs against the float64 judge of
tests/size_judge.py: the nine (b, p) cells of st_ransac_judge.batch_case carry nine rows of the transition table, in plain mode (the
free fit is an input: exact comparisons at the ratio) and in robust mode (the kernel computes the free fit: captra_part_fit_st_ransac's
bits).  State and record are exact; a held translation follows the rule of tests/test_st_ransac_gpu.py::_check -- at most twice as far
from float64 as the fp32 mirror, with a floor of 4 fp32 ulps.  The fixtures and their preconditions are built on the CPU
(tests/test_size_judge_cpu.py)."""
import numpy as np
import pytest

from tests import size_judge as ZJ
from tests import st_ransac_judge as SJ

F32_EPS = float(np.finfo(np.float32).eps)
SIZES = (257, 4096, 4100)                   # 4100: the first size whose coordinates are not staged in LDS
EXTRA_SHAPES = ({"num_hyps": 1, "B": 1}, {"num_hyps": 17, "B": 1}, {"num_hyps": 256, "B": 1}, {"P": 8})
# case seeds: 3000 + N + 10 sym + num_hyps + 100 P unless the CPU found that seed's fixture broken (the free or the held fit's
# preconditions): the replacement is listed here
SEEDS = {(257, False, 1, 1, 3): 7174}       # (one hypothesis: most seeds draw an outlier into it)
OPTS = ZJ.TABLE_OPTS
_FIX = {}


def fixture(N, sym, num_hyps=64, B=3, P=3):
    """(case, robust-mode state (mean, n, miss, names)), built once and never modified; every precondition asserted."""
    k = (N, bool(sym), num_hyps, B, P)
    if k not in _FIX:
        seed = SEEDS.get(k, 3000 + N + 10 * bool(sym) + num_hyps + 100 * P)
        case = SJ.batch_case(N, seed, False, True, bool(sym), num_hyps=num_hyps, B=B, P=P)
        base = np.float32(float(case["th"]) / 0.02)
        state = ZJ.table_state(base, B, P, robust=True)
        ref = SJ.judge_batch(case)
        free = (ref["scale"].astype(np.float32), ref["trans"].astype(np.float32), ref["valid"])
        ZJ.check_batch(case, free, state, OPTS)
        _FIX[k] = (case, state)
    return _FIX[k]


def drawn_fixture(sym, seed=5):
    """The member ranks the kernel draws for fixture(257, sym) from `seed` with b0 = 0, the preconditions of both fits asserted."""
    case, state = fixture(257, sym)
    B, P, H = case["ranks"].shape[:3]
    ranks = np.zeros_like(case["ranks"])
    for b in range(B):
        for p in range(P):
            c = int((case["labels"][b] == p).sum())
            if c >= 3:
                ranks[b, p] = SJ.draw_ranks(seed, b, p, H, c)
    SJ.check_batch(case, ranks)
    ref = SJ.judge_batch(case, ranks)
    ZJ.check_batch(case, (ref["scale"].astype(np.float32), ref["trans"].astype(np.float32), ref["valid"]), state, OPTS, ranks)
    return ranks


def _dev(a, device):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)


SENT_F, SENT_I = float("nan"), -7
OUT_F = {"scale": (), "trans": (3,), "scale_free": (), "trans_free": (3,), "mean_out": ()}
OUT_I = ("valid", "valid_free", "best", "num_inliers", "n_out", "miss_out", "held", "accepted", "held_best", "held_inliers")
ORDER = ("scale", "trans", "valid", "scale_free", "trans_free", "valid_free", "best", "num_inliers", "mean_out", "n_out", "miss_out", "held",
         "accepted", "held_best", "held_inliers")


def _abi(case, device, state, free=None, ranks="given", seed=0, b0=0, opts=OPTS, shape=None, sym=None, null=(), num_hyps=None):
    """The C ABI on sentinel-filled outputs -> (err, dict of numpy outputs).  free = None: robust mode (ranks 'given' = the case's,
    None = drawn in the kernel); free = (scale, trans, valid): plain mode.  null: names of pointers passed as NULL."""
    import torch
    from captra_amd import _lib as L
    B, P, _, N = case["src"].shape
    H = case["ranks"].shape[2] if free is None else 0
    H = H if num_hyps is None else num_hyps
    r = case["ranks"] if isinstance(ranks, str) else ranks
    d = {k: _dev(case[k], device) for k in ("labels", "src", "tgt", "tgt_mean", "rot", "prev_scale", "prev_trans")}
    d["sample_rank"] = None if (r is None or free is not None) else _dev(np.asarray(r, np.int32), device)
    fin = (None, None, None) if free is None else (_dev(np.asarray(free[0], np.float32), device), _dev(np.asarray(free[1], np.float32), device),
                                                  _dev(np.asarray(free[2], np.int32), device))
    d.update(scale_free_in=fin[0], trans_free_in=fin[1], valid_free_in=fin[2], size_mean=_dev(np.asarray(state[0], np.float32), device),
             size_n=_dev(np.asarray(state[1], np.int32), device), size_miss=_dev(np.asarray(state[2], np.int32), device))
    out = {k: torch.full((B, P) + s, SENT_F, device=device) for k, s in OUT_F.items()}
    out.update({k: torch.full((B, P), SENT_I, dtype=torch.int32, device=device) for k in OUT_I})
    ptr = lambda name, t: None if name in null else L.ptr(t)
    outs = [None if (free is not None and k in ("scale_free", "trans_free", "valid_free", "best", "num_inliers")) else ptr(k, out[k]) for k in ORDER]
    b_, p_, n_ = shape if shape is not None else (B, P, N)
    o = {"max_frames": None, "reset_after": None, **opts}
    with torch.cuda.device(device):
        err = L.lib().captra_part_fit_st_size(b_, p_, n_, int(case["sym"]) if sym is None else sym, b0, H, float(case["th"]),
                                              ptr("labels", d["labels"]), ptr("src", d["src"]), ptr("tgt", d["tgt"]), 0, L.ptr(d["tgt_mean"]),
                                              ptr("rot", d["rot"]), L.ptr(d["prev_scale"]), L.ptr(d["prev_trans"]), L.ptr(d["sample_rank"]), seed,
                                              *(ptr(k, d[k]) for k in ("scale_free_in", "trans_free_in", "valid_free_in", "size_mean", "size_n", "size_miss")),
                                              int(o["min_frames"]), float(o["max_ratio"]), int(o["max_frames"] or 0), int(o["reset_after"] or 0),
                                              *outs, L.stream_ptr())
    torch.cuda.synchronize(device)
    return err, {k: v.cpu().numpy() for k, v in out.items()}


def _untouched(got, keys=ORDER):
    return all((np.isnan(got[k]).all() if k in OUT_F else (got[k] == SENT_I).all()) for k in keys)


def _bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.dtype.itemsize == 4, what
    np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32), err_msg=str(what))


def _check(got, case, state, free, robust, name, ranks=None, opts=OPTS):
    """Everything the issue asserts for one launch; free = the free fit as the kernel read (plain) or wrote (robust) it."""
    ranks = case["ranks"] if ranks is None else ranks
    B, P = got["held"].shape
    ref = ZJ.judge_batch(case, free, state, opts, robust, ranks, given=got["mean_out"])
    mir = ZJ.judge_batch(case, free, state, opts, robust, ranks, dt=np.float32, given=got["mean_out"])
    fs, ft, fv = free
    for b in range(B):
        for p in range(P):
            d = ref["decision"][b, p]
            pts, S, T = SJ.members_of(case, b, p)
            tag = (name, b, p, len(pts), state[3].get((b, p)))
            # ---- state and record: integers and pass-through bits exactly, an averaged mean within 1 fp32 ulp of float64
            assert (got["n_out"][b, p], got["miss_out"][b, p], got["accepted"][b, p], got["held"][b, p]) == (d["n"], d["miss"], d["accepted"], d["held"]), (tag, d)
            if d["exact"]:
                _bits(got["mean_out"][b, p], d["mean32"], tag)
            else:
                assert abs(float(got["mean_out"][b, p]) - d["mean"]) <= float(np.spacing(np.float32(abs(d["mean"])))), (tag, got["mean_out"][b, p], d["mean"])
            assert np.isfinite(got["mean_out"][b, p]), tag
            if not d["held"]:
                # ---- not held: the free fit, bit for bit
                _bits(got["scale"][b, p], np.float32(fs[b, p]), tag)
                _bits(got["trans"][b, p], np.asarray(ft[b, p], np.float32), tag)
                assert got["valid"][b, p] == int(fv[b, p]) and got["held_inliers"][b, p] == 0 and got["held_best"][b, p] == 0, tag
                continue
            # ---- held: the scale is mean_out's bits; the judge's inlier set and count; the translation by the mirror rule
            _bits(got["scale"][b, p], got["mean_out"][b, p], tag)
            assert got["held_inliers"][b, p] == ref["held_inliers"][b, p], (tag, got["held_inliers"][b, p], ref["held_inliers"][b, p])
            if robust and len(pts) >= 3:
                h = int(got["held_best"][b, p])
                assert 0 <= h < ranks.shape[2], tag
                tri = (np.asarray(ranks[b, p, h]) % len(pts))[None]
                Rp, t = ZJ.estimator_given(S[tri], T[tri], case["rot"][b, p], got["mean_out"][b, p], case["sym"])
                sv = np.full(1, np.float64(got["mean_out"][b, p]))
                mask = np.zeros(case["labels"].shape[1], bool)
                mask[pts[SJ.errors(S, T, case["rot"][b, p], Rp, sv, t, case["sym"])[0] < float(case["th"])]] = True
                np.testing.assert_array_equal(mask, ref["inliers"][b, p], err_msg=str(tag))
            assert bool(got["valid"][b, p]) == bool(ref["valid"][b, p]), tag
            if not ref["valid"][b, p]:
                _bits(got["trans"][b, p], np.asarray(ft[b, p], np.float32), tag)      # an invalid held fit: trans_free's bits
                continue
            assert mir["valid"][b, p], tag
            et, mt = np.abs(got["trans"][b, p] - ref["trans"][b, p]).max(), np.abs(mir["trans"][b, p] - ref["trans"][b, p]).max()
            print(f"{tag}: held trans err kernel {et:.2e} mirror {mt:.2e}")
            assert et <= max(2 * mt, 4 * F32_EPS * np.abs(ref["trans"][b, p]).max()), (tag, et, mt)
    for k in ("scale", "trans", "mean_out"):
        assert np.isfinite(got[k]).all(), (name, k)
    return ref


def _plain_free(case, rng_seed=1):
    """Plain mode's free fit is an INPUT: scale = base in every cell (so the rows' comparisons are exact), a random finite translation,
    valid everywhere but in cell (2, 2)."""
    B, P = case["rot"].shape[:2]
    base = np.float32(float(case["th"]) / 0.02)
    rng = np.random.default_rng(rng_seed)
    valid = np.ones((B, P), np.int32)
    if B > 2:
        valid[2, 2] = 0
    return np.full((B, P), base, np.float32), rng.uniform(-1, 1, (B, P, 3)).astype(np.float32), valid


def _st_ransac(case, device, **kw):
    from tests.test_st_ransac_gpu import _abi as st_abi
    return st_abi(case, device, **kw)


# ============================================================================================================ 1. kernel vs judge
@pytest.mark.gpu
@pytest.mark.parametrize("sym", [False, True])
@pytest.mark.parametrize("N", SIZES)
def test_size_plain_vs_judge(device, N, sym):
    case, rstate = fixture(N, sym)
    base = np.float32(float(case["th"]) / 0.02)
    state = ZJ.table_state(base)
    free = _plain_free(case)
    err, got = _abi(case, device, state, free=free)
    assert err == 0
    assert _untouched(got, ("scale_free", "trans_free", "valid_free", "best", "num_inliers"))
    ref = _check(got, case, state, free, False, f"plain N={N} sym={sym}")
    dec = ref["decision"]
    # the nine rows did what their names say
    assert [dec[c]["accepted"] for c in sorted(dec)] == [1, 1, 1, 0, 1, 1, 1, 1, 0]
    assert [dec[c]["held"] for c in sorted(dec)] == [0, 1, 1, 1, 1, 0, 1, 0, 1]
    assert [dec[c]["n"] for c in sorted(dec)] == [1, 2, 3, 2, 3, 1, 4, 1, 2]
    assert dec[1, 0]["miss"] == 1 and dec[2, 2]["miss"] == 1 and dec[1, 2]["miss"] == 0
    # held and valid: the recipe part, the outlier part and the whole-cloud part; held and invalid: 2, 3 and 0 members
    assert got["valid"].tolist() == [[1, 1, 1], [0, 0, 1], [1, 1, 0]]
    assert got["held_inliers"][2, 0] == N and got["held_inliers"][1].tolist() == [2, 3, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("sym", [False, True])
@pytest.mark.parametrize("N", SIZES)
def test_size_robust_vs_judge(device, N, sym):
    case, state = fixture(N, sym)
    err, got = _abi(case, device, state)
    assert err == 0
    # the free outputs are captra_part_fit_st_ransac's on the same inputs, bit for bit
    err, st = _st_ransac(case, device)
    assert err == 0
    for mine, theirs in (("scale_free", "scale"), ("trans_free", "trans"), ("valid_free", "valid"), ("best", "best"), ("num_inliers", "num_inliers")):
        _bits(got[mine], st[theirs], mine)
    free = (got["scale_free"], got["trans_free"], got["valid_free"])
    ref = _check(got, case, state, free, True, f"robust N={N} sym={sym}")
    dec = ref["decision"]
    assert got["valid_free"].tolist() == [[1, 1, 0], [0, 0, 1], [1, 0, 0]]
    assert [dec[c]["held"] for c in sorted(dec)] == [0, 1, 1, 1, 1, 0, 1, 0, 1]
    assert [dec[c]["accepted"] for c in sorted(dec)] == [1, 1, 0, 0, 0, 1, 1, 0, 0]
    assert [dec[c]["n"] for c in sorted(dec)] == [1, 2, 2, 2, 2, 1, 4, 0, 2]
    _bits(got["mean_out"][2, 1], np.float32(0.0), "an empty state leaves as +0")
    # held and valid: the recipe part and the whole-cloud part; the outlier part, 2, 3 and 0 members: held, invalid, trans_free's bits
    assert got["valid"].tolist() == [[1, 1, 0], [0, 0, 1], [1, 0, 0]]
    assert got["held_inliers"][1].tolist() == [0, 3, 0] and got["held_inliers"][0, 2] < 3
    assert got["held_inliers"][0, 1] == int(case["true_in"][0, 1].sum()) and got["held_inliers"][2, 0] == int(case["true_in"][2, 0].sum())


# ============================================================================================================== 2. kernel draws
def _slice(case, state, sl):
    out = dict(case)
    for k in ("labels", "src", "tgt", "tgt_mean", "rot", "prev_scale", "prev_trans", "ranks"):
        out[k] = None if case[k] is None else np.ascontiguousarray(case[k][sl])
    return out, tuple(np.ascontiguousarray(s[sl]) for s in state[:3])


@pytest.mark.gpu
@pytest.mark.parametrize("sym", [False, True])
def test_size_kernel_draws(device, sym):
    """sample_rank = NULL: the slice b in [1, 3) launched with b0 = 1 equals the whole batch's rows, bit for bit; the free outputs are
    captra_part_fit_st_ransac's with the same seed and b0."""
    case, state = fixture(257, sym)
    err, got = _abi(case, device, state, ranks=None, seed=5)
    assert err == 0
    err, st = _st_ransac(case, device, ranks=None, seed=5)
    assert err == 0
    _bits(got["scale_free"], st["scale"], "scale_free")
    _bits(got["best"], st["best"], "best")
    sub, sstate = _slice(case, state, slice(1, 3))
    err, part = _abi(sub, device, sstate, ranks=None, seed=5, b0=1)
    assert err == 0
    for k in ORDER:
        _bits(part[k], got[k][1:3], k)
    _, other = _abi(sub, device, sstate, ranks=None, seed=5, b0=0)
    assert (other["best"] != part["best"]).any() or (other["held_best"] != part["held_best"]).any()      # (b0 reaches the draws)
    # and the drawn ranks give the judge's results (seed 5 meets the preconditions: drawn_fixture, checked on the CPU)
    _check(got, case, state, (got["scale_free"], got["trans_free"], got["valid_free"]), True, f"drawn sym={sym}", ranks=drawn_fixture(sym))


# ===================================================================================================== 3. non-members, refusals
@pytest.mark.gpu
@pytest.mark.parametrize("robust", [False, True])
def test_size_non_members_reach_no_output(device, robust):
    """batch_case fills half of the non-members with NaN / Inf; filling ALL of them changes no output bit."""
    case, rstate = fixture(257, False)
    state = rstate if robust else ZJ.table_state(np.float32(float(case["th"]) / 0.02))
    free = None if robust else _plain_free(case)
    err, got = _abi(case, device, state, free=free)
    assert err == 0
    member = case["labels"][:, None, :] == np.arange(3)[None, :, None]
    bad = dict(case)
    bad["src"] = np.where(member[:, :, None, :], case["src"], np.float32(np.nan))
    bad["tgt"] = np.where(member.any(1)[:, None, :], case["tgt"], np.float32(np.inf))
    err, got2 = _abi(bad, device, state, free=free)
    assert err == 0
    for k in ORDER:
        if robust or k not in ("scale_free", "trans_free", "valid_free", "best", "num_inliers"):
            _bits(got2[k], got[k], k)
            assert np.isfinite(got2[k]).all(), k


@pytest.mark.gpu
def test_size_refused_arguments(device):
    case, state = fixture(257, False)
    free = _plain_free(case)
    refused = [dict(shape=(3, 9, 257)), dict(shape=(3, 0, 257)), dict(shape=(3, 3, 16385)), dict(shape=(3, 3, 0)), dict(shape=(-1, 3, 257)),
               dict(num_hyps=257), dict(num_hyps=-1), dict(sym=2), dict(sym=-1), dict(b0=-1), dict(b0=2 ** 31 - 3),
               dict(opts={**OPTS, "min_frames": 0}), dict(opts={**OPTS, "max_ratio": 1.0}), dict(opts={**OPTS, "max_ratio": 0.5}),
               dict(opts={**OPTS, "max_ratio": float("nan")}), dict(opts={**OPTS, "max_ratio": float("inf")}),
               dict(opts={**OPTS, "max_frames": -1}), dict(opts={**OPTS, "reset_after": -1})]
    refused += [dict(null=(k,)) for k in ("labels", "src", "tgt", "rot", "size_mean", "size_n", "size_miss", "scale", "trans", "valid", "mean_out",
                                          "n_out", "miss_out", "held", "accepted", "scale_free", "trans_free", "valid_free")]
    for kw in refused:
        err, got = _abi(case, device, state, **kw)
        assert err == -1 and _untouched(got), kw
    # plain mode: all three free inputs or none; robust mode: none of them
    for k in ("scale_free_in", "trans_free_in", "valid_free_in"):
        err, got = _abi(case, device, state, free=free, null=(k,))
        assert err == -1 and _untouched(got), k
    err, got = _abi(case, device, state, free=free, num_hyps=64)
    assert err == -1 and _untouched(got)
    err, got = _abi(case, device, state, shape=(0, 3, 257))
    assert err == 0 and _untouched(got)
    err, _ = _abi(case, device, state, b0=2 ** 31 - 4)                      # b0 = INT_MAX - b: the largest allowed
    assert err == 0
    err, got = _abi(case, device, state, null=("best", "num_inliers", "held_best", "held_inliers"))       # the optional outputs
    assert err == 0 and _untouched(got, ("best", "num_inliers", "held_best", "held_inliers")) and not np.isnan(got["scale"]).any()
    # options absent: no cap, never a restart
    err, got = _abi(case, device, state, free=free, opts={"min_frames": 1, "max_ratio": 2.0})
    assert err == 0 and got["n_out"][2, 0] == 5 and got["n_out"][1, 2] == 3 and got["miss_out"][1, 2] == 3 and got["held"].all()


# ================================================================================================================ 4. extra shapes
@pytest.mark.gpu
@pytest.mark.parametrize("kw", EXTRA_SHAPES, ids=["H1", "H17", "H256", "P8"])
def test_size_extra_shapes(device, kw):
    case, state = fixture(257, False, **kw)
    err, got = _abi(case, device, state)
    assert err == 0
    err, st = _st_ransac(case, device)
    assert err == 0
    _bits(got["scale_free"], st["scale"], "scale_free")
    _bits(got["num_inliers"], st["num_inliers"], "num_inliers")
    _check(got, case, state, (got["scale_free"], got["trans_free"], got["valid_free"]), True, f"robust {kw}")
    pstate = ZJ.table_state(np.float32(float(case["th"]) / 0.02), *case["rot"].shape[:2])
    free = _plain_free(case)
    err, got = _abi(case, device, pstate, free=free)
    assert err == 0
    _check(got, case, pstate, free, False, f"plain {kw}")


# ===================================================================================================================== 5. wrapper
@pytest.mark.gpu
@pytest.mark.parametrize("robust", [False, True])
def test_size_wrapper(device, robust):
    """part_fit_st_size_track returns the ABI's bits; in plain mode behind part_fit_st_track, as the loop calls it."""
    from captra_amd.pose_utils.pose_fit import part_fit_st_size_track, part_fit_st_track
    case, state = fixture(257, True)
    dv = {k: _dev(case[k], device) for k in ("labels", "src", "tgt", "tgt_mean", "rot", "prev_scale", "prev_trans")}
    st = {"size_mean": _dev(state[0], device), "size_n": _dev(state[1], device), "size_miss": _dev(state[2], device)}
    args = (dv["labels"], dv["src"], dv["tgt"], dv["tgt_mean"], dv["rot"], dv["prev_scale"], dv["prev_trans"].unsqueeze(-1), True, st)
    if robust:
        pose, new, info = part_fit_st_size_track(*args, **OPTS, inlier_th=float(case["th"]), sample_rank=_dev(case["ranks"], device))
        err, got = _abi(case, device, state)
        assert set(info) >= {"inliers", "best"}
        np.testing.assert_array_equal(info["inliers"].cpu().numpy(), got["num_inliers"])
    else:
        fs, ft, fv = part_fit_st_track(*args[:8])
        pose, new, info = part_fit_st_size_track(*args, **OPTS, free=(fs, ft, fv))
        err, got = _abi(case, device, state, free=(fs.cpu().numpy(), ft[..., 0].cpu().numpy(), fv.int().cpu().numpy()))
        assert info["free"] is not None and info["free"].data_ptr() == fs.data_ptr()
    assert err == 0 and pose["translation"].shape == (3, 3, 3, 1) and set(new) == {"size_mean", "size_n", "size_miss"}
    _bits(pose["scale"].cpu().numpy(), got["scale"], "scale")
    _bits(pose["translation"][..., 0].cpu().numpy(), got["trans"], "trans")
    np.testing.assert_array_equal(pose["valid"].cpu().numpy(), got["valid"].astype(bool))
    _bits(new["size_mean"].cpu().numpy(), got["mean_out"], "mean")
    for mine, theirs in (("size_n", "n_out"), ("size_miss", "miss_out")):
        np.testing.assert_array_equal(new[mine].cpu().numpy(), got[theirs])
    for k in ("held", "accepted", "held_inliers", "held_best"):
        np.testing.assert_array_equal(info[k].cpu().numpy(), got[k])
    assert info["n"] is new["size_n"] and got["held"].any() and not got["held"].all()
