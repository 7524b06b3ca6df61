"""The geometry kernels on knife-edge, tie, scaled, non-finite and thin clouds, every route against the judge (tests/geom_judge.py),
which tests/test_geom_judge_cpu.py ties to the C oracle row by row and proves to bite: a distance that is fused, re-associated,
expanded or taken in double, a '<=' for a '<', an r^2 rounded from double, a tie resolved towards the later index -- each changes
an index of these clouds.  Indices, squared distances, running minima and gathered coordinates are compared element by element,
with no tolerance; only the 3-NN WEIGHTS have a bound (gamma_8 against float64) beside the bit comparison with the fp32 mirror.

Why every route may run the non-finite clouds (no data-dependent loop or data-derived index is left open):
* register-resident samplers (csrc/fps.hip, fps_round.h): the round loop runs m - 1 times whatever the data; the only data-derived
  index is the pick, which is always the index of a lane's own slot.  Slots beyond the cloud hold minimum 0 and the highest indices, a
  NaN distance has the largest bit pattern and so never lowers a minimum (the oracle's `d < temp` is false too): an all-NaN cloud or a
  NaN start point leaves every minimum at 1e10 and the pick at index 0.
* pruned sampler (csrc/fps_pruned.hip): the Morton cell (line 141) is min(15, max(0, (int)...)): in 0..15 whatever the conversion makes
  of a NaN or Inf; a zero, infinite or NaN extent gives a scale of 16 / max(extent, 1e-30) or 0, nothing else.  The round loop advances
  by np >= 1 picks: the order on the wave tops is a strict total order of (bits, index, wave) triples of unsigned integers, so exactly
  one top has no predecessor, and that one is always accepted.  Boxes come from fminf / fmaxf (NaNs dropped): a NaN point is outside
  its bucket's box, and its distance is NaN, which lowers nothing, so skipping the bucket is right; a NaN sample gives lb = 0
  (fmaxf(NaN, 0)) and visits every bucket.
* ball query scan (csrc/bq_scan.h), captra_query_and_group: loops over the cloud's 256-point groups; a list slot is cnt + rank < nsample
  and holds k0 + lane < n (padding slots hold +inf and never hit), so the grouping reads inside the cloud.
* ball query grid (csrc/ball_query.hip, PRUNE): built only if every axis has hi >= lo and the extent is finite and positive (this
  pull request: an all-NaN axis used to reach (int)(-inf) cells), so every f in the sizing loop is finite and >= 0; the loop ends
  because the edge grows by 1.26 per turn (an infinite edge gives one cell); point keys are clamped to the grid after the conversion,
  centre cells are clamped in float (fminf / fmaxf drop a NaN) before it.
* three_nn / knn / 3-NN weights / interp_concat: loops over the known cloud; indices are loop counters (0 for an unused slot).
The level-1 stream kernel gets finite clouds only: its consumers spin on the sampler's progress.

The sampler's NaN-temp row is held to the reference CUDA kernel's `min(d, temp[k])` (sampling_gpu.cu:134: a NaN temp is replaced), which
is what every sampler here computes; the oracle restates the torch path's ternary (a NaN temp stays).  The judge has both and the
CPU test shows they differ on exactly that row.

Measured on an MI355X: see DESIGN.md §4 ("geometry judge").

The file's name sorts it LAST in the suite on purpose.  Collected in front of the hipGraph tests (as tests/test_geom_edges_gpu.py) the
suite's process ended twice in a segmentation fault inside the HIP runtime's graph replay, in two different tests that were there before
(test_l1_stream_gpu.py::test_track_step_with_level1_stream_equals_plain_step, test_stream_gpu.py::
test_track_step_with_streamed_sampler_equals_plain_step; neither launches a kernel these tests or their kernel fixes touch) -- what
DESIGN.md §7 records for a gather-gradient device test.  Cause not found; behind the last graph replay nothing of this file can
precede one.
"""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

from oracle import ops as O
from tests import f32_judge as FJ
from tests import geom_judge as J

pytestmark = pytest.mark.gpu


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    """Equal as values, NaN == NaN."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


@contextlib.contextmanager
def _knobs(waves=0, variant=0, pruned_min=8192, prune=0, split=1):
    from captra_amd import _lib
    lib = _lib.lib()
    lib.captra_fps_set_waves(ctypes.c_int(waves)); lib.captra_fps_set_variant(ctypes.c_int(variant))
    lib.captra_fps_set_pruned_min(ctypes.c_int(pruned_min)); lib.captra_ball_query_set_prune(ctypes.c_int(prune))
    lib.captra_three_nn_set_split(ctypes.c_int(split))
    try:
        yield
    finally:
        lib.captra_fps_set_waves(ctypes.c_int(0)); lib.captra_fps_set_variant(ctypes.c_int(0))
        lib.captra_fps_set_pruned_min(ctypes.c_int(8192)); lib.captra_ball_query_set_prune(ctypes.c_int(0))
        lib.captra_three_nn_set_split(ctypes.c_int(1))


def _rows(op, pred=lambda r: True):
    return [r for r in J.RUNS if r["op"] == op and pred(r)]


# ==== furthest point sampling =============================================================================================================
def _fps_expected(e):
    """(idx, temp) the kernels are held to: the judge's, with the CUDA kernel's min on the NaN-temp rows (module docstring)."""
    return (e["idx_fminf"], e["temp_fminf"]) if e["temp_in"] is not None else (e["idx"], e["temp"])


def _check_fps(device, row, gather=True, drop_in=True, what=""):
    from captra_amd import _lib, fused
    e = J.expected(row)
    want_idx, want_temp = _fps_expected(e)
    xyz, m = e["xyz"], row["m"]
    B, n, _ = xyz.shape
    x = _dev(xyz, device)
    tag = f"{J.row_id(row)} {what}"
    if drop_in:
        temp = torch.full((B, n), 1e10, device=device) if e["temp_in"] is None else _dev(e["temp_in"], device)
        idx = torch.full((B, m), -1, dtype=torch.int32, device=device)
        _lib.call("captra_furthest_point_sampling", B, n, m, x.data_ptr(), temp.data_ptr(), idx.data_ptr())
        np.testing.assert_array_equal(idx.cpu().numpy(), want_idx, err_msg=f"{tag}: picks")
        assert _same(temp.cpu().numpy(), want_temp), f"{tag}: running minima handed back"
    if gather and e["temp_in"] is None:
        idx, n3, cn = fused.fps_gather(x, m)
        np.testing.assert_array_equal(idx.cpu().numpy(), want_idx, err_msg=f"{tag}: fps_gather picks")
        picked = np.take_along_axis(xyz, want_idx[..., None].astype(np.int64).repeat(3, -1), axis=1)
        assert (_bits(n3.cpu().numpy()) == _bits(picked)).all() and (_bits(cn.cpu().numpy()) == _bits(picked.transpose(0, 2, 1))).all(), \
            f"{tag}: gathered coordinates"


@pytest.mark.parametrize("row", _rows("fps"), ids=J.row_id)
def test_fps_default_dispatch(device, row):
    """captra_furthest_point_sampling and captra_fps_gather as dispatched: <1,8> at 512 points, <4,16> at 4096, the pruned kernel from
    8192 on (32 register slots up to 16384, LDS-resident slots and up to four certified picks per round at 20480)."""
    _check_fps(device, row)


@pytest.mark.parametrize("row", _rows("fps", lambda r: r["cloud"][1] == 16384), ids=J.row_id)
def test_fps_16384_without_the_pruned_kernel(device, row):
    """captra_fps_set_pruned_min(0): sixteen waves x 16 points, the cloud beyond the LDS mirror -- the winner's coordinates travel
    through the wave slots."""
    with _knobs(pruned_min=0):
        _check_fps(device, row, what="pruned kernel off")


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("waves", [1, 2, 4, 8, 16])
def test_fps_every_wave_configuration_at_4096(device, waves, variant):
    for row in _rows("fps", lambda r: r["cloud"][1] == 4096 and r["cloud"][0] in ("knife", "ties", "nonfinite", "nan_temp")):
        with _knobs(waves=waves, variant=variant):
            # captra_fps_gather is instantiated for two waves and more of the blocked kernel only
            _check_fps(device, row, gather=variant == 0 and waves > 1, what=f"waves={waves} variant={variant}")


@pytest.mark.parametrize("stride,counts", [(4096, (4096, 3000, 64, 2999, 1, 513, 4095, 100, 2048, 65)),
                                           (20480, (20480, 8300, 4096, 13001, 9000, 20479, 8192, 16384, 12000, 1000))])
def test_fps_gather_ragged(device, stride, counts):
    """captra_fps_gather_ragged on the non-finite clouds cut to unequal lengths: every cloud as if sampled alone."""
    from captra_amd import fused
    xyz = J.nonfinite_clouds(stride)[0]
    m = 12
    idx, n3, _ = fused.fps_gather(_dev(xyz, device), m, n_per_cloud=torch.tensor(counts, dtype=torch.int32, device=device))
    idx, n3 = idx.cpu().numpy(), n3.cpu().numpy()
    for b, c in enumerate(counts):
        want, _ = J.fps(xyz[b, :c], m)
        np.testing.assert_array_equal(idx[b], want, err_msg=f"cloud {b} of {c} points")
        assert (_bits(n3[b]) == _bits(xyz[b, want])).all()
        np.testing.assert_array_equal(want, O.furthest_point_sample(xyz[b:b + 1, :c], m)[0])


@pytest.mark.parametrize("n", [512, 4096])
def test_fps_gather_part_cut_at_the_knife_picks(device, n):
    """captra_fps_gather_part cut before and after every knife-edge pick (picks 1 and 2), resuming from the state it handed back;
    then with a NaN written into that state between two parts (held to the CUDA kernel's min: the entry is replaced)."""
    from captra_amd import fused
    row = dict(op="fps", cloud=("knife", n), m=8)
    e = J.expected(row)
    x = _dev(e["xyz"], device)
    bufs = fused.fps_gather_parts(x, 8)
    for j0, j1 in ((0, 1), (1, 2), (2, 3), (3, 8)):
        fused.fps_gather_part(x, 8, j0, j1, bufs)
    np.testing.assert_array_equal(bufs[0].cpu().numpy(), e["idx"])
    assert _same(bufs[3].cpu().numpy(), e["temp"])
    assert (_bits(bufs[1].cpu().numpy()) == _bits(np.take_along_axis(e["xyz"], e["idx"][..., None].astype(np.int64).repeat(3, -1), 1))).all()
    # NaN in the state of two finite clouds: picks 0..3, poison, picks 4..11
    xyz = J.fps_inputs(("scaled", n, 0))[0]
    x = _dev(xyz, device)
    bufs = fused.fps_gather_parts(x, 12)
    fused.fps_gather_part(x, 12, 0, 4, bufs)
    head, state = bufs[0].cpu().numpy().copy(), bufs[3].cpu().numpy().copy()
    for b in range(2):
        i4, t4 = J.fps(xyz[b], 4)
        np.testing.assert_array_equal(head[b, :4], i4)
        assert _same(state[b], t4)
    state[0, 5] = J.NAN_POS; state[1, n // 2] = J.NAN_NEG; state[1, n - 1] = J.NAN_POS
    bufs[3].copy_(_dev(state, device))
    fused.fps_gather_part(x, 12, 4, 12, bufs)
    for b in range(2):
        want, temp = J.fps(xyz[b], 12, temp=state[b], tmin="fminf", j0=4, idx=np.concatenate([head[b, :4], np.zeros(8, np.int32)]))
        np.testing.assert_array_equal(bufs[0][b].cpu().numpy(), want)
        assert _same(bufs[3][b].cpu().numpy(), temp)


# ==== ball query ==========================================================================================================================
def _ball_multi(device, x, c, queries):
    from captra_amd import fused
    outs = [torch.full((x.shape[0], c.shape[1], k), -1, dtype=torch.int32, device=device) for _, k in queries]
    fused.ball_query_multi([r for r, _ in queries], [k for _, k in queries], x, c, outs=outs)
    return [o.cpu().numpy() for o in outs]


@pytest.mark.parametrize("prune", [0, 1])
@pytest.mark.parametrize("row", _rows("ball"), ids=J.row_id)
def test_ball_query_routes(device, row, prune):
    """captra_ball_query per radius and captra_ball_query_multi with 3 and 4 radii per scan (on the knife clouds two of them straddle
    every knife), the grid path switched off and on (it answers clouds of 1024..4096 points and up to three radii; n = 9000 is the
    scan's second LDS tile), 64 centres and more."""
    from captra_amd import _lib
    e = J.expected(row)
    B, n, _ = e["xyz"].shape
    m = e["centres"].shape[1]
    x, c = _dev(e["xyz"], device), _dev(e["centres"], device)
    with _knobs(prune=prune):
        for (r, k), want in zip(e["queries"], e["lists"]):
            idx = torch.full((B, m, k), -1, dtype=torch.int32, device=device)
            _lib.call("captra_ball_query", B, n, m, float(r), k, c.data_ptr(), x.data_ptr(), idx.data_ptr())
            np.testing.assert_array_equal(idx.cpu().numpy(), want, err_msg=f"{J.row_id(row)} prune={prune} r={r} k={k}")
        for nr in (3, 4):
            q = e["queries"][:nr]
            if len(q) < 2:
                continue
            for (r, k), got, want in zip(q, _ball_multi(device, x, c, q), e["lists"]):
                np.testing.assert_array_equal(got, want, err_msg=f"{J.row_id(row)} prune={prune} {len(q)} radii, r={r} k={k}")


def test_ball_query_centre_window(device):
    """centre_m0 / centre_mc: a launch fills its window of the lists and nothing else, on a knife cloud (the knife centre inside the
    first window, outside the second)."""
    from captra_amd import fused
    e = J.expected(dict(op="ball", cloud=("knife", "fused_a", 4096)))
    x, c = _dev(e["xyz"], device), _dev(e["centres"], device)
    q = e["queries"][:3]
    for m0, mc in ((0, 5), (37, 20), (63, 1)):
        outs = [torch.full((1, 64, k), -1, dtype=torch.int32, device=device) for _, k in q]
        with fused.centre_window(m0, mc):
            fused.ball_query_multi([r for r, _ in q], [k for _, k in q], x, c, outs=outs)
        for o, want in zip(outs, e["lists"]):
            o = o.cpu().numpy()
            np.testing.assert_array_equal(o[:, m0:m0 + mc], want[:, m0:m0 + mc])
            assert (o[:, :m0] == -1).all() and (o[:, m0 + mc:] == -1).all()


@pytest.mark.parametrize("row", _rows("ball", lambda r: r["cloud"][-1] == 4096 or r["cloud"][1] == 4096), ids=J.row_id)
def test_query_and_group_lists_and_coordinates(device, row):
    """captra_query_and_group with want_idx: the lists are the judge's and every grouped coordinate is xyz[idx] - centre, bit for bit."""
    from captra_amd import fused
    e = J.expected(row)
    x, c = _dev(e["xyz"], device), _dev(e["centres"], device)
    done = 0
    for (r, k), want in zip(e["queries"], e["lists"]):
        if k % 4:
            continue
        out, idx = fused.query_and_group(float(r), k, x, c, None, True, want_idx=True)
        np.testing.assert_array_equal(idx.cpu().numpy(), want, err_msg=f"{J.row_id(row)} r={r} k={k}")
        with np.errstate(invalid="ignore"):
            grouped = np.stack([e["xyz"][b][want[b]] - e["centres"][b][:, None] for b in range(x.shape[0])]).transpose(0, 3, 1, 2)
        assert _same(out.cpu().numpy(), grouped), f"{J.row_id(row)} r={r} k={k}: grouped coordinates"
        done += 1
    assert done


# ==== three_nn, knn =======================================================================================================================
@pytest.mark.parametrize("row", _rows("nn3") + _rows("knn"), ids=J.row_id)
def test_three_nn_and_knn(device, row):
    from captra_amd import pointnet2_cuda as pc
    e = J.expected(row)
    B, n, _ = e["unknown"].shape
    s = e["known"].shape[1]
    k = row.get("k", 3)
    u, kn = _dev(e["unknown"], device), _dev(e["known"], device)
    d2 = torch.empty(B, n, k, device=device)
    idx = torch.full((B, n, k), -1, dtype=torch.int32, device=device)
    pc.knn_wrapper(B, n, s, k, u, kn, d2, idx)
    np.testing.assert_array_equal(idx.cpu().numpy(), e["idx"], err_msg=f"{J.row_id(row)}: knn")
    assert _same(d2.cpu().numpy(), e["d2"]), f"{J.row_id(row)}: knn squared distances"
    if row["op"] == "nn3":
        d2.fill_(-1.0); idx.fill_(-1)
        pc.three_nn_wrapper(B, n, s, u, kn, d2, idx)
        np.testing.assert_array_equal(idx.cpu().numpy(), e["idx"], err_msg=f"{J.row_id(row)}: three_nn")
        assert _same(d2.cpu().numpy(), e["d2"]), f"{J.row_id(row)}: three_nn squared distances"


# ==== the product path's 3-NN weights and interpolation ===================================================================================
@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("row", _rows("weights"), ids=J.row_id)
def test_three_nn_weights_and_interp_concat(device, row, split):
    """captra_three_nn_weights, one lane and four lanes per point, s up to 5000 (4097 and 5000 run the second 4096-point tile, with a
    knife pair across its edge): indices exact, weights within gamma_8 of the float64 evaluation of the fp32 squared distances and
    bit-equal to the fp32 mirror (numpy's float32 sqrt and divide are correctly rounded, and so are the kernel's); then
    captra_interp_concat on that (idx, weight), the NaN-weight triples (fewer than three finite neighbours) included."""
    from captra_amd import fused
    e = J.expected(row)
    u, kn = _dev(e["unknown"], device), _dev(e["known"], device)
    with _knobs(split=split):
        idx, w = fused.three_nn_weights(u, kn)
    idx, w = idx.cpu().numpy(), w.cpu().numpy()
    np.testing.assert_array_equal(idx, e["idx"], err_msg=f"{J.row_id(row)} split={split}")
    fin = np.isfinite(e["w64"]).all(-1)
    assert (np.isfinite(w).all(-1) == fin).all() and (np.isnan(w) == np.isnan(e["w32"])).all()
    pos = e["w64"][fin] > 0
    err = np.abs(w[fin].astype(np.float64) - e["w64"][fin])[pos] / e["w64"][fin][pos]
    off = int((w[fin] != e["w32"][fin]).sum())
    print(f"geom edges {J.row_id(row)} split={split}: finite triples {int(fin.sum())} of {fin.size}, worst error {float(err.max()) / J.U if err.size else 0:.2f} u "
          f"(bound 8 u), weights off the fp32 mirror's bits {off} of {int(fin.sum()) * 3}")
    assert (err <= J.GAMMA8).all()
    assert (w[fin][~pos] == 0).all()
    assert off == 0
    # interpolation of known features through these triples
    B, n, _ = idx.shape
    s = e["known"].shape[1]
    rng = np.random.default_rng(s + n)
    skip, fk = rng.standard_normal((B, 5, n)).astype(np.float32), rng.standard_normal((B, 7, s)).astype(np.float32)
    got = fused.interp_concat(_dev(skip, device), _dev(fk, device), _dev(idx, device), _dev(w, device)).cpu().numpy()
    cls, val, _ = FJ.verdict(FJ.interp_concat(FJ.T(skip), FJ.T(fk), idx, w))
    assert (FJ.classify(got) == cls).all(), f"{J.row_id(row)}: classes of the interpolated features"
    ok = cls == FJ.FIN
    ref = np.concatenate([skip, O.three_interpolate(fk, idx, w)], 1)
    assert (_bits(got)[ok] == _bits(ref)[ok]).all()
    assert float(np.abs(got[ok] - val[ok]).max()) <= 1e-5 * max(1.0, float(np.abs(val[ok]).max()))


# ==== the level-1 stream kernel ===========================================================================================================
def _stream_clouds():
    parts = [J.fps_knife_batch(4096)["xyz"], J.tie_clouds(4096)] + [J.ball_knife_cloud(d, 4096)["xyz"][None] for d in J.DEVIATIONS]
    return np.concatenate(parts).astype(np.float32)


def test_level1_stream_kernel_on_finite_knife_and_tie_clouds(device):
    """captra_sa1_stream_bf16 at N = 4096, M = 512: the sampler's knife pairs and tie clouds, and the ball knife clouds (their knife
    centre is point 0, the first pick; KNIFE_R = 0.1 is the middle SA1 radius and its ball holds fewer than 64 points).  Picks and
    neighbour lists are the judge's; the pooled features are the three-launch composition's."""
    from captra_amd import fused
    from tests.test_l1_stream_gpu import _check, _module, _reference
    xyz = _stream_clouds()
    picks, _ = J.fps_batch(xyz, 512)
    centres = np.take_along_axis(xyz, picks[..., None].astype(np.int64).repeat(3, -1), 1)
    fused.set_mlp_dtype("bf16")
    try:
        x_n3 = _dev(xyz, device)
        x_cn = x_n3.transpose(1, 2).contiguous()
        mods = [_module(0, 11, device), _module(3, 12, device)]
        feats = [None, x_cn.clone() * 0.5]
        assert fused.sa1_stream_supported(4096, mods, (0, 3))
        got = fused.sa1_stream_bf16(x_n3, x_cn, mods, feats)
        torch.cuda.synchronize()
        assert not fused.sa1_stream_gave_up(got[5])
        np.testing.assert_array_equal(got[0].cpu().numpy(), picks, err_msg="stream kernel: picks")
        assert (_bits(got[1].cpu().numpy()) == _bits(centres)).all()
        for r, k, lst in zip(J.SA_RADII, J.SA_KS, got[3]):
            np.testing.assert_array_equal(lst.cpu().numpy(), J.ball_query_batch(J.r2_float(r), k, xyz, centres), err_msg=f"stream kernel: lists of r={r}")
        _check(got[:6], _reference(x_n3, x_cn, mods, feats), "knife and tie clouds")
    finally:
        fused.set_mlp_dtype("fp32")
