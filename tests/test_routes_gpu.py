"""Every selectable launch route of an operation gives the default route's bits.

The rest of the suite pins a kernel on the route its launcher picks by default, on the whole chip, at the test's shape.  Here the
same operation runs every OTHER way the launchers can be made to run it -- a per-call option (captra_launch_opts::reserved_cus: the
persistent kernels sized for a smaller grid), a knob that tools/ and bench.py set, a shape condition (the furthest-point sampler
whose picks no longer fit LDS beside the cloud) -- and every such route is held, bit for bit, to

  * the default route's output on the same inputs, and
  * the reference the default is held to: oracle.ops for the exact-fp32 and the geometry kernels, for the bf16 kernels the route
    that tests/test_bf16_edges_gpu.py / tests/test_tile_bf16_gpu.py / tests/test_neck_gpu.py hold to the bf16 judge.

Output buffers are filled with a sentinel and everything outside the written window must keep it.  Which kernel a launch took cannot
be seen from outside (the profiler's names are shared between variants), so where a route is chosen by a condition the test
restates the condition next to the source line it mirrors and asserts that its shape satisfies it.

A  grid-size independence: sa_wave_lds_kernel, sa_wave_pipe_kernel, captra_sa_scales_multi, tb_head12p_kernel under reserved_cus
B  routes only a knob reaches (plus the sampler's automatic non-deferred form)
C  the f32x6 persistent kernels, whose grid is the CU count: job counts cus - 1, cus, cus + 1, 2 cus + 1
"""
import contextlib
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import ops as O
from tests import clouds
from tests.test_sa_pipe_rows_gpu import CF, NARROW, WIDE
from tests.test_sa_pipe_rows_gpu import _inputs as sp_inputs
from tests.test_sa_pipe_rows_gpu import _reference as sp_reference

pytestmark = pytest.mark.gpu

# every knob this file touches and its default (include/captra_hip.h section 4)
KNOB_DEFAULTS = {
    "captra_ball_query_set_cpw": (0,), "captra_fps_set_defer": (1,), "captra_dense_bf16_set_shared_affine": (1,),
    "captra_neck_chain_set_split": (4,), "captra_pw_set_occupancy": (0,), "captra_pw_set_pair": (1,), "captra_sa_fused_set_wn": (0,),
    "captra_sa_fused_set_mode": (0,), "captra_group_set_shape": (64, 32, 0), "captra_query_and_group_set_shape": (0, 0),
    "captra_sa_fused_set_split": (1,), "captra_fps_set_pruned_min": (8192,), "captra_tile_bf16_set_persistent": (1,),
}
PAD = 4          # channel offset of a scale's block inside the (wider) output tensor
FILL = 12345     # what an untouched slot of the dynamic hand-out's counter pool holds


def _set(name, values):
    from captra_amd import _lib
    getattr(_lib.lib(), name)(*[ctypes.c_int(int(v)) for v in values])


@contextlib.contextmanager
def knob(name, *values):
    """A thread-local knob of the library for the block, back at its default afterwards."""
    _set(name, values)
    try:
        yield
    finally:
        _set(name, KNOB_DEFAULTS[name])


@pytest.fixture(autouse=True)
def _knobs_back_at_their_defaults(device):
    yield
    from captra_amd import fused
    for name, values in KNOB_DEFAULTS.items():
        _set(name, values)
    fused.USE_NECK_CHAIN = True
    fused.set_mlp_dtype("fp32")


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _cus(device):
    return torch.cuda.get_device_properties(device).multi_processor_count


FREE = [1, 2, 3, 5, 32, "cus-1"]          # free CUs f: reserved_cus = cus - f


def _reserved(device, f):
    cus = _cus(device)
    return cus - (cus - 1 if f == "cus-1" else int(f))


_DEVICE_CACHE = {}


def _cached(key, make):
    """Device-side inputs and default-route outputs of a case: made once, shared by the tests of the case, never written to."""
    if key not in _DEVICE_CACHE:
        _DEVICE_CACHE[key] = make()
    return _DEVICE_CACHE[key]


@pytest.fixture(scope="module", autouse=True)
def _drop_the_cache_after_the_module():
    yield
    _DEVICE_CACHE.clear()


# ================================================================================================ A. grid-size independence
WALKS = {"static": 0, "heuristic": 1, "split": 2, "dynamic": 0}       # captra_sa_fused_set_split of the walk


def _walk(device, launch, walk, reserved, centres, k, wave_per_wg):
    """launch() (-> the output tensor) as one of the four walks of the persistent SA kernels with `reserved` CUs left free.  The
    dynamic hand-out: the launchers give a launch its counter when the walk is not the slice-per-wave one, k > 32 and the static
    grid has more than one workgroup (sa_fused.hip:920, sa_pipe.hip:501); it is zeroed, counts at least the centres, and the pool's
    other slot keeps its fill.  At k == 32 (one slice per centre) no launch takes a counter: the slot keeps its fill too."""
    from captra_amd import _lib
    pool = None
    opts = {"reserved_cus": reserved}
    if walk == "dynamic":
        pool = torch.full((2,), FILL, dtype=torch.int32, device=device)
        opts["dyn_pool"] = (pool.data_ptr(), 2)
    with knob("captra_sa_fused_set_split", WALKS[walk]), _lib.launch_options(**opts):
        out = launch()
    if pool is not None:
        counts = pool.cpu().tolist()
        wgs = (centres + wave_per_wg - 1) // wave_per_wg
        print(f"dynamic hand-out, reserved {reserved}: counter slots {counts} for {centres} centres")
        assert counts[1] == FILL, counts
        if k > 32 and wgs > 1:
            assert centres <= counts[0] < FILL, counts
        else:
            assert counts[0] == FILL, counts
    return out


# ---- A.1 sa_wave_lds_kernel through fused.sa_scale_fused: 111, 111 and 82 centres = 14, 14 and 11 workgroups of 8 waves
SL_CASES = [(0, (32, 32, 64), 200, 37, 32, 3), (3, (64, 64, 128), 200, 37, 64, 3), (0, (64, 96, 128), 300, 41, 128, 2)]


@functools.lru_cache(maxsize=None)
def _sl_inputs(cfeat, chans, n, m, k, B):
    rng = np.random.default_rng(1000 * cfeat + sum(chans) + 7 * n + 3 * m + k + B)
    xyz_cn = rng.random((B, 3, n), dtype=np.float32) - 0.5
    feat = rng.standard_normal((B, cfeat, n)).astype(np.float32) if cfeat else None
    new_xyz = rng.random((B, m, 3), dtype=np.float32) - 0.5
    idx = rng.integers(0, n, (B, m, k)).astype(np.int32)
    dims = (cfeat + 3,) + chans
    layers = tuple(((rng.standard_normal((dims[i], dims[i + 1])) / np.sqrt(dims[i])).astype(np.float32),
                    rng.standard_normal(dims[i + 1]).astype(np.float32)) for i in range(3))
    return xyz_cn, feat, new_xyz, idx, layers


@functools.lru_cache(maxsize=None)
def _sl_reference(*case):
    xyz_cn, feat, new_xyz, idx, layers = _sl_inputs(*case)
    x = O.sa_group(feat, xyz_cn, new_xyz, idx)
    for w, b in layers:
        x = O.pointwise_mlp(x, w, b, 1)
    ref = O.max_over_k(x)
    ref.setflags(write=False)
    return ref


def _sl_device(device, case):
    def make():
        from captra_amd import fused
        xyz_cn, feat, new_xyz, idx, layers = _sl_inputs(*case)
        return dict(xyz=_dev(xyz_cn, device), feat=None if feat is None else _dev(feat, device), new=_dev(new_xyz, device), idx=_dev(idx, device),
                    packed=[fused.pack(_dev(w, device), _dev(b, device)) for w, b in layers])
    return _cached(("sl", case), make)


def _sl_launch(device, case, jobs=None, out=None):
    from captra_amd import fused
    d = _sl_device(device, case)
    B, m, c3 = case[5], case[3], case[1][2]
    out = torch.full((B, c3 + 9, m), -1.0, device=device) if out is None else out
    return fused.sa_scale_fused(d["feat"], d["xyz"], d["new"], d["idx"], d["packed"], out, PAD, jobs=jobs)


def _block_is_ref(out, ref, what):
    """The scale's channel block holds the oracle's bits and the rows around it the sentinel."""
    got = out.cpu().numpy()
    c3 = ref.shape[1]
    assert (got[:, :PAD] == -1).all() and (got[:, PAD + c3:] == -1).all(), what
    np.testing.assert_array_equal(got[:, PAD:PAD + c3], ref, err_msg=str(what))


def _sl_default(device, case):
    def make():
        out = _sl_launch(device, case)
        _block_is_ref(out, _sl_reference(*case), ("default", case))
        return out
    return _cached(("sl_default", case), make)


@pytest.mark.parametrize("f", FREE)
@pytest.mark.parametrize("case", SL_CASES)
def test_sa_lds_kernel_on_a_smaller_grid(device, case, f):
    """sa_wave_lds_kernel with f free CUs: the grid is min(workgroups, resident) (sa_fused.hip:909-921), so at f = 1 a workgroup walks
    five or more rounds and the last one is partial; the heuristic's split decision (l.916) reads `resident` and flips as f shrinks."""
    cfeat, chans, n, m, k, B = case
    want, ref = _sl_default(device, case), _sl_reference(*case)
    for walk in WALKS:
        out = _walk(device, lambda: _sl_launch(device, case), walk, _reserved(device, f), B * m, k, 8)
        assert torch.equal(out, want), (case, f, walk)
        _block_is_ref(out, ref, (case, f, walk))


def _clamp_check(device, launch, want, what):
    """reserved_cus at and beyond the chip clamps to one free CU (common.h:98-101), below zero to none reserved (common.h:43)."""
    from captra_amd import _lib
    cus = _cus(device)
    with _lib.launch_options(reserved_cus=cus - 1):
        one = launch()
    assert torch.equal(one, want), what
    for reserved in (cus, cus + 7, 2 ** 31 - 1):
        for split in (0, 1):
            with knob("captra_sa_fused_set_split", split), _lib.launch_options(reserved_cus=reserved):
                assert torch.equal(launch(), one), (what, reserved, split)
    with _lib.launch_options(reserved_cus=-3):
        assert torch.equal(launch(), want), (what, -3)


@pytest.mark.parametrize("case", SL_CASES)
def test_sa_lds_kernel_reserved_cus_clamps(device, case):
    _clamp_check(device, lambda: _sl_launch(device, case), _sl_default(device, case), case)


# ---- A.2 sa_wave_pipe_kernel through fused.sa_first_layer_pre_pm + fused.sa_scale_pre_pm (M * K a multiple of 128)
SP_CASES = [(chans, n, m, k, B) for chans in (WIDE, NARROW) for n, m, k, B in ((200, 6, 64, 3), (96, 5, 128, 2))]


def _sp_device(device, case):
    def make():
        from captra_amd import fused
        xyz_cn, feat, new_xyz, idx, layers = sp_inputs(*case)
        packed = [fused.pack(_dev(w, device), _dev(b, device)) for w, b in layers]
        chans, n, m, k, B = case
        assert fused.sa_scale_pipe_supported(CF, packed, m, k, b=B, n=n)
        return dict(xyz=_dev(xyz_cn, device), new=_dev(new_xyz, device), idx=_dev(idx, device), packed=packed,
                    v1pm=fused.sa_first_layer_pre_pm(_dev(feat, device), packed[0]))
    return _cached(("sp", case), make)


def _sp_launch(device, case, jobs=None, out=None):
    from captra_amd import fused
    d = _sp_device(device, case)
    chans, n, m, k, B = case
    out = torch.full((B, chans[2] + 9, m), -1.0, device=device) if out is None else out
    return fused.sa_scale_pre_pm(d["v1pm"], d["xyz"], d["new"], d["idx"], d["packed"], out, PAD, CF, jobs=jobs)


def _sp_default(device, case):
    def make():
        out = _sp_launch(device, case)
        _block_is_ref(out, sp_reference(*case), ("default", case))
        return out
    return _cached(("sp_default", case), make)


@pytest.mark.parametrize("f", FREE)
@pytest.mark.parametrize("case", SP_CASES)
def test_sa_pipe_kernel_on_a_smaller_grid(device, case, f):
    """sa_wave_pipe_kernel (one workgroup of four waves per free CU, sa_pipe.hip:493-501): 18 and 10 centres are 5 and 3 workgroups,
    so one or two free CUs make every wave walk several centres and the split decision (l.498) flips."""
    chans, n, m, k, B = case
    want, ref = _sp_default(device, case), sp_reference(*case)
    for walk in WALKS:
        out = _walk(device, lambda: _sp_launch(device, case), walk, _reserved(device, f), B * m, k, 4)
        assert torch.equal(out, want), (case, f, walk)
        _block_is_ref(out, ref, (case, f, walk))


@pytest.mark.parametrize("case", SP_CASES)
def test_sa_pipe_kernel_reserved_cus_clamps(device, case):
    _clamp_check(device, lambda: _sp_launch(device, case), _sp_default(device, case), case)


# ---- A.3 a level's scales in one launch (captra_sa_scales_multi): sa_wave_lds3_kernel's g0 / g1 and sa_wave_pipe2_kernel's g0 are
# the per-scale grids, which shrink with the free CUs
def _level1_cases(cfeat):
    """The three SA1 widths in the level's order with one input width (sl_collect_flush launches them together only then,
    sa_fused.hip:840-844): A.1's shapes with cfeat set."""
    return [(cfeat,) + c[1:] for c in SL_CASES]


@pytest.mark.parametrize("f", [1, 3, "cus-1"])
@pytest.mark.parametrize("level", ["sa1_cfeat0", "sa1_cfeat3", "sa2"])
def test_sa_scales_multi_on_a_smaller_grid(device, level, f):
    from captra_amd import _lib, fused
    if level == "sa2":
        cases = [(NARROW, 200, 6, 64, 3), (WIDE, 96, 5, 128, 2)]          # (128, 128, 256) first: sa_pipe.hip:463 wants code 0 then 1
        launch, default, refs = _sp_launch, _sp_default, [sp_reference(*c) for c in cases]
    else:
        cases = _level1_cases(0 if level == "sa1_cfeat0" else 3)
        launch, default, refs = _sl_launch, _sl_default, [_sl_reference(*c) for c in cases]
    alone = [default(device, c) for c in cases]                             # every scale launched on its own, whole chip
    outs = [torch.full_like(a, -1.0) for a in alone]
    jobs = []
    with _lib.launch_options(reserved_cus=_reserved(device, f)):
        for c, o in zip(cases, outs):
            launch(device, c, jobs=jobs, out=o)
        assert len(jobs) == len(cases)
        fused.sa_scales_multi(jobs, device)
    for c, o, a, r in zip(cases, outs, alone, refs):
        assert torch.equal(o, a), (level, f, c)
        _block_is_ref(o, r, (level, f, c))


# ---- A.4 tb_head12p_kernel: short and uneven tile runs
@pytest.mark.parametrize("f", [8, 4, 2, 1, 9])
def test_head12_persistent_tile_runs(device, f):
    """x (3, 300, 128): three 128-position tiles per cloud, the last one ragged, nine in all.  tile_bf16.hip:826-836: persistent when
    tiles > free CUs, tpw = ceil(tiles / free) tiles per workgroup.  f = 8: runs of 2, the fifth workgroup holds one tile; f = 4: runs of
    3 = one cloud each; f = 2: runs of 5 and 4, both crossing a cloud boundary mid-run (the cloud's GroupNorm coefficients reload);
    f = 1: one workgroup walks everything; f = 9: not persistent.  y2 and its statistics against the one-tile-per-workgroup launch
    (captra_tile_bf16_set_persistent(0): the form tests/test_bf16_edges_gpu.py holds to the bf16 judge), bit for bit."""
    from captra_amd import _lib, fused
    B, l = 3, 300
    tiles = B * ((l + 127) // 128)
    tpw = (tiles + f - 1) // f
    nwg = (tiles + tpw - 1) // tpw
    assert tiles == 9 and (tiles > f) == (f != 9)
    assert (tpw, nwg) == {8: (2, 5), 4: (3, 3), 2: (5, 2), 1: (9, 1), 9: (1, 9)}[f]

    def make():
        rng = np.random.default_rng(300)
        lin1 = fused.pack(_dev((rng.standard_normal((128, 512)) / 11.3).astype(np.float32), device), _dev(rng.standard_normal(512).astype(np.float32), device))
        lin2 = fused.pack(_dev((rng.standard_normal((512, 512)) / 22.6).astype(np.float32), device), _dev(rng.standard_normal(512).astype(np.float32), device))
        x = _dev(rng.standard_normal((B, l, 128)).astype(np.float32), device).to(torch.bfloat16)
        ab1 = _dev(rng.standard_normal((B, 512, 2)).astype(np.float32), device)          # a different affine per cloud
        assert fused.head12_bf16_supported(x, lin1, lin2)
        with knob("captra_tile_bf16_set_persistent", 0):
            want = fused.head12_bf16(x, lin1, ab1, lin2)
        return x, lin1, ab1, lin2, want
    x, lin1, ab1, lin2, want = _cached("head12", make)
    with _lib.launch_options(reserved_cus=_cus(device) - f):
        y2, st = fused.head12_bf16(x, lin1, ab1, lin2)
    assert torch.equal(y2.view(torch.int16), want[0].view(torch.int16)), f
    assert torch.equal(st, want[1]), f


# ================================================================================================ B. routes only a knob reaches
# ---- B.1 ball query, two centres per wave on the index-order scan (ball_query_kernel<NR, false, 2>, ball_query.hip:386-406)
def _bq_run(device, xyz, new_xyz, radii, ks, single=False, window=None):
    """captra_ball_query (single) / captra_ball_query_multi into sentinel-filled lists -> [numpy (B, M, K)]."""
    from captra_amd import _lib, fused
    B, n, _ = xyz.shape
    m = new_xyz.shape[1]
    xd, nd = _dev(xyz, device), _dev(new_xyz, device)
    outs = [torch.full((B, m, k), -1, dtype=torch.int32, device=device) for k in ks]
    with fused.centre_window(*window) if window else contextlib.nullcontext():
        if single:
            _lib.call("captra_ball_query", B, n, m, float(radii[0]), int(ks[0]), nd.data_ptr(), xd.data_ptr(), outs[0].data_ptr())
        else:
            fused.ball_query_multi(radii, ks, xd, nd, outs=outs)
    return [o.cpu().numpy() for o in outs]


def _bq_check(device, xyz, new_xyz, radii, ks, what, window=None):
    for single in ((True, False) if len(radii) == 1 else (False,)):
        with knob("captra_ball_query_set_cpw", 2):
            two = _bq_run(device, xyz, new_xyz, radii, ks, single, window)
        one = _bq_run(device, xyz, new_xyz, radii, ks, single, window)
        for r, k, a, b in zip(radii, ks, two, one):
            np.testing.assert_array_equal(a, b, err_msg=f"{what}: two centres per wave vs one, r={r} k={k} single={single}")
            ref = O.ball_query(r, k, xyz, new_xyz)
            if window:
                m0, mc = window
                assert (a[:, :m0] == -1).all() and (a[:, m0 + mc:] == -1).all(), what
                a, ref = a[:, m0:m0 + mc], ref[:, m0:m0 + mc]
            assert (a >= 0).all(), what                    # the whole written window: no sentinel left
            np.testing.assert_array_equal(a, ref, err_msg=f"{what}: vs the oracle, r={r} k={k} single={single}")


def _radii(r, k, nr):
    return [r, 0.5 * r, 1.5 * r, 0.25 * r][:nr], [k, max(1, k // 2), k + 1, 2][:nr]


@pytest.mark.parametrize("nr", [1, 2, 3, 4])
@pytest.mark.parametrize("n,m,k,r", [(1, 1, 4, 0.5), (63, 5, 7, 0.3), (65, 33, 1, 0.2), (1000, 37, 200, 0.6)])
def test_ball_query_two_centres_per_wave(device, n, m, k, r, nr):
    """Odd m: the last wave holds one centre; n no multiple of 64: a ragged last chunk."""
    rng = np.random.default_rng(n + m)
    xyz = (rng.random((2, n, 3), dtype=np.float32) - 0.5).astype(np.float32)
    new_xyz = (rng.random((2, m, 3), dtype=np.float32) - 0.5).astype(np.float32)
    _bq_check(device, xyz, new_xyz, *_radii(r, k, nr), what=(n, m, k, r, nr))


@pytest.mark.parametrize("nr", [1, 3])
@pytest.mark.parametrize("kind", ["far_and_nan", "duplicates", "window", "window_far_and_nan"])
def test_ball_query_two_centres_per_wave_edges(device, kind, nr):
    """A centre at 50.0 and a NaN centre (empty balls are zeros) sharing their waves with ordinary centres; a duplicate-padded cloud;
    a centre window with odd start and odd length (a wave's pair straddles both ends), rows outside it untouched."""
    n, m, k, r = 1000, 37, 20, 0.3
    rng = np.random.default_rng(len(kind))
    xyz = (rng.random((2, n, 3), dtype=np.float32) - 0.5).astype(np.float32)
    new_xyz = xyz[:, rng.integers(0, n, m)].copy()
    if kind == "duplicates":
        xyz[:, n // 3:] = xyz[:, :1]
    if kind.endswith("far_and_nan"):
        new_xyz[:, 4] = 50.0
        new_xyz[:, 7] = np.nan
        new_xyz[1, 36] = np.nan                                    # the lone centre of the last wave
    radii, ks = _radii(r, k, nr)
    _bq_check(device, xyz, new_xyz, radii, ks, what=(kind, nr), window=(3, 7) if kind.startswith("window") else None)
    if kind.endswith("far_and_nan") and not kind.startswith("window"):
        got = _bq_run(device, xyz, new_xyz, radii, ks)[0]
        assert (got[:, 4] == 0).all() and (got[:, 7] == 0).all() and (got[1, 36] == 0).all()


# ---- B.2 furthest-point sampling, outputs written inside the rounds (defer = 0): by knob, and automatically
def _fps_clouds(n):
    a = np.stack([clouds.s_nocs(i)[0][:n] for i in range(2)])
    dup = np.stack([clouds.s_nocs_dup(i, n_unique=max(1, (2 * n) // 3), n=n)[0] for i in range(2)])
    same = np.full((2, n, 3), 0.25, np.float32)
    return {"nocs": a.astype(np.float32), "nocs_dup": dup.astype(np.float32), "identical": same}


def _fps_all_entries(device, xyz, m):
    """Every entry point of the blocked kernel on one batch -> dict of numpy results."""
    from captra_amd import _lib, fused
    B, n, _ = xyz.shape
    x = _dev(xyz, device)
    res = {}
    temp = torch.full((B, n), 1e10, device=device)
    idx = torch.full((B, m), -1, dtype=torch.int32, device=device)
    _lib.call("captra_furthest_point_sampling", B, n, m, x.data_ptr(), temp.data_ptr(), idx.data_ptr())
    res["fps.idx"], res["fps.temp"] = idx.cpu().numpy(), temp.cpu().numpy()
    i, n3, cn = fused.fps_gather(x, m)
    res["gather.idx"], res["gather.n3"], res["gather.cn"] = i.cpu().numpy(), n3.cpu().numpy(), cn.cpu().numpy()
    counts = [n, n - n // 3]
    i, n3, cn = fused.fps_gather(x, m, n_per_cloud=torch.tensor(counts, dtype=torch.int32, device=device))
    res["ragged.idx"], res["ragged.n3"], res["ragged.cn"] = i.cpu().numpy(), n3.cpu().numpy(), cn.cpu().numpy()
    bufs = fused.fps_gather_parts(x, m)
    assert bufs is not None
    bufs[0].fill_(-1)
    cuts = [0, m // 3, (2 * m) // 3, m]
    for j0, j1 in zip(cuts[:-1], cuts[1:]):
        fused.fps_gather_part(x, m, j0, j1, bufs)
    for name, t in zip(("idx", "n3", "cn", "state"), bufs):
        res["part." + name] = t.cpu().numpy()
    return res, counts


@pytest.mark.parametrize("n,m", [(100, 37), (512, 128), (1000, 300)])
def test_fps_outputs_written_inside_the_rounds(device, n, m):
    """captra_fps_set_defer(0) (fps.hip:316-332: the blocked kernel stores every pick and its coordinates in its round instead of
    after the last one) on captra_furthest_point_sampling, captra_fps_gather, captra_fps_gather_ragged and captra_fps_gather_part in
    three parts: indices, both coordinate layouts and the running minima against the default and against the oracle."""
    for kind, xyz in _fps_clouds(n).items():
        with knob("captra_fps_set_defer", 0):
            got, counts = _fps_all_entries(device, xyz, m)
        want, _ = _fps_all_entries(device, xyz, m)
        for key in want:
            np.testing.assert_array_equal(got[key], want[key], err_msg=f"{kind} {key}: defer 0 vs 1")
        t_ref = np.full(xyz.shape[:2], 1e10, np.float32)
        ref = O.furthest_point_sample(xyz, m, temp=t_ref)
        picked = np.take_along_axis(xyz, ref[..., None].astype(np.int64).repeat(3, -1), axis=1)
        for entry in ("fps", "gather", "part"):
            np.testing.assert_array_equal(got[entry + ".idx"], ref, err_msg=f"{kind} {entry}")
        for entry in ("gather", "part"):
            np.testing.assert_array_equal(got[entry + ".n3"], picked, err_msg=f"{kind} {entry}")
            np.testing.assert_array_equal(got[entry + ".cn"], picked.transpose(0, 2, 1), err_msg=f"{kind} {entry}")
        np.testing.assert_array_equal(got["fps.temp"], t_ref, err_msg=kind)
        np.testing.assert_array_equal(got["part.state"], t_ref, err_msg=kind)
        if kind == "identical":
            assert (ref == 0).all()
        for i, c in enumerate(counts):
            r = O.furthest_point_sample(xyz[i:i + 1, :c], m)[0]
            np.testing.assert_array_equal(got["ragged.idx"][i], r, err_msg=f"{kind} ragged cloud {i}")
            np.testing.assert_array_equal(got["ragged.n3"][i], xyz[i, r], err_msg=f"{kind} ragged cloud {i}")
            np.testing.assert_array_equal(got["ragged.cn"][i], xyz[i, r].T, err_msg=f"{kind} ragged cloud {i}")


def test_fps_cloud_fits_lds_but_cloud_and_picks_do_not(device):
    """The non-deferred form WITHOUT a knob: fps.hip:323-330 defers the outputs only while slots + cloud + picks fit 150 KiB of LDS.
    12000 points and 4096 picks: the cloud's mirror fits, mirror + picks do not.  (The pruned sampler that clouds of this size take
    by default is switched off: captra_fps_set_pruned_min(0).)  Picks, coordinates and running minima against the pruned kernel's
    and the oracle's."""
    from captra_amd import _lib, fused
    n, m, B = 12000, 4096, 1
    slots = 2 * 16 * 8
    assert n * 12 + slots <= 150 * 1024 < n * 12 + slots + 4 * m            # fps.hip:326 holds, fps.hip:330 does not
    xyz = clouds.s_uni(1, n)[None]
    x = _dev(xyz, device)

    def run():
        temp = torch.full((B, n), 1e10, device=device)
        idx = torch.full((B, m), -1, dtype=torch.int32, device=device)
        _lib.call("captra_furthest_point_sampling", B, n, m, x.data_ptr(), temp.data_ptr(), idx.data_ptr())
        return (idx, temp) + tuple(fused.fps_gather(x, m))
    pruned = run()
    with knob("captra_fps_set_pruned_min", 0):
        plain = run()
    for a, b, name in zip(plain, pruned, ("idx", "temp", "gather idx", "gather n3", "gather cn")):
        assert torch.equal(a, b), name
    t_ref = np.full((B, n), 1e10, np.float32)
    ref = O.furthest_point_sample(xyz, m, temp=t_ref)
    np.testing.assert_array_equal(plain[0].cpu().numpy(), ref)
    np.testing.assert_array_equal(plain[1].cpu().numpy(), t_ref)
    np.testing.assert_array_equal(plain[2].cpu().numpy(), ref)
    np.testing.assert_array_equal(plain[3].cpu().numpy()[0], xyz[0, ref[0]])
    np.testing.assert_array_equal(plain[4].cpu().numpy()[0], xyz[0, ref[0]].T)


# ---- B.3 bf16 dense layer, GroupNorm on load: every wave transforms its own operand (dense_bf16.hip:421,458)
@pytest.mark.parametrize("L", [100, 257])
@pytest.mark.parametrize("cin,cout", [(128, 256), (512, 256), (128, 512), (512, 512)])
def test_dense_bf16_per_wave_affine(device, cin, cout, L):
    """captra_dense_bf16_set_shared_affine(0) at nt = cout / 32 >= 8, where the default transforms the operand once per workgroup and
    shares it through LDS.  Both compute bf16(relu(fma(a, x, b))) in front of the same k-ascending MFMA sequence, so the bits are
    the default's -- point-major bf16 and channel-major fp32 output, and the statistics epilogue -- and the LDS-tiled kernel's
    (captra_dense_bf16_tile, bit-equal to this layer in tests/test_tile_bf16_gpu.py)."""
    from captra_amd import fused
    B = 2
    assert cout // 32 >= 8                                          # dense_bf16.hip:458
    rng = np.random.default_rng(cin + cout + L)
    lin = fused.pack(_dev((rng.standard_normal((cin, cout)) / np.sqrt(cin)).astype(np.float32), device), _dev(rng.standard_normal(cout).astype(np.float32), device))
    x = _dev(rng.standard_normal((B, L, cin)).astype(np.float32), device).to(torch.bfloat16)
    ab = _dev(rng.standard_normal((B, cin, 2)).astype(np.float32), device)

    def run():
        pm = fused.pointwise_mlp_bf16pm(x, lin, L, in_pm=True, out_pm=True, ab=ab, act=fused.ACT_RELU)
        cm = fused.pointwise_mlp_bf16pm(x, lin, L, in_pm=True, out_pm=False, ab=ab, act=fused.ACT_RELU)
        raw, st = fused.pointwise_mlp_bf16pm(x, lin, L, in_pm=True, out_pm=True, ab=ab, with_stats=True)
        plain = fused.pointwise_mlp_bf16pm(x, lin, L, in_pm=True, out_pm=True, ab=ab)
        return pm.view(torch.int16), cm.view(torch.int32), raw.view(torch.int16), st, plain.view(torch.int16)
    want = run()
    with knob("captra_dense_bf16_set_shared_affine", 0):
        got = run()
    for g, w, name in zip(got, want, ("point-major", "channel-major", "raw with statistics", "statistics", "raw")):
        assert torch.equal(g, w), (name, int((g != w).sum()))
    assert fused.dense_bf16_tile_supported(x, lin)
    tile = fused.dense_bf16_tile(x, lin, ab=ab)
    assert torch.equal(got[4], tile.view(torch.int16))


# ---- B.4 the neck's SA3 module, last layer shared by one or two workgroups (neck_bf16.hip:429-431)
@pytest.mark.parametrize("L", [128, 68])
def test_neck_sa3_last_layer_split(device, L):
    """captra_neck_chain_set_split(1 | 2) on the only shape that reads it (c0 -> 256 -> 512 -> 1024: row tiles per wave 1, 2, 4)
    through fused.neck_chain(0, ...), against the default (4) and against the layer-by-layer route (the LDS-tiled chain with the
    pooled epilogue: what PointNetSetAbstraction runs with the one-launch module off, and what tests/test_neck_gpu.py holds the
    default to).  L = 68: a ragged position tile (the module itself never asks for it: it pools whole 32s)."""
    from captra_amd import _lib, fused
    from tests.test_neck_gpu import _layers
    B = 3
    rng = np.random.default_rng(L)
    layers = _layers((515, 256, 512, 1024), rng, device)
    assert [(c // 32 + 7) // 8 for c in (256, 512, 1024)] == [1, 2, 4]      # neck_bf16.hip:425-428
    xyz = _dev(rng.random((B, 3, L), dtype=np.float32) - 0.5, device)
    feat = _dev(np.abs(rng.standard_normal((B, 512, L))).astype(np.float32), device)
    fused.set_mlp_dtype("bf16")
    try:
        assert fused.neck_chain_supported(515, L, layers, 3, 0) and fused.chain_tile_bf16_supported(515, L, layers, pool=True)
        res = {}
        for split in (4, 1, 2):
            _lib.prof_reset(); _lib.prof_enable(True)
            with knob("captra_neck_chain_set_split", split):
                res[split] = fused.neck_chain(0, xyz, layers, x2=feat)
            _lib.prof_enable(False)
            assert _lib.prof_read("neck_chain")[1] == 1, "the one-launch kernel did not run"
        layerwise = fused.mlp_chain_bf16_tile(xyz, layers, [fused.ACT_RELU] * 3, x2=feat, pool=True)
    finally:
        fused.set_mlp_dtype("fp32")
        _lib.prof_enable(False)
    assert res[4].shape == (B, 1024, 1) and layerwise.shape == (B, 1024, 1)
    for split in (1, 2, 4):
        assert torch.equal(res[split], res[4]), split
        assert torch.equal(res[split], layerwise), (split, float((res[split] - layerwise).abs().max()))


# ---- B.5 64x64-tile dense launches padded to three or two workgroups per CU (pointwise_mlp.hip:830-832)
def test_dense_launches_with_padded_occupancy(device):
    """captra_pw_set_occupancy(2 | 3) (bench.py --pw-occ) asks every 64x64 wave-tile launch for unused dynamic LDS.  The padded form
    needs ceil(L / 64) ceil(cout / 64) B >= 2048 (pointwise_mlp.hip:862-868); the smallest such shape is 128 -> 512 at 4 x 4096
    positions.  Every launcher that adds the pad -- captra_pointwise_mlp (paired and unpaired columns), _mlp2, _pm, _cb, _gn with and
    without coefficients and statistics -- against occupancy 0, and the plain forms against the oracle on cloud 0."""
    from captra_amd import _lib, fused
    cin, cout, L, B, csplit = 128, 512, 4096, 4, 3
    assert ((L + 63) // 64) * ((cout + 63) // 64) * B >= 2048 > ((L + 63) // 64) * ((cout + 63) // 64) * (B - 1)
    rng = np.random.default_rng(5)
    xs = rng.standard_normal((B, cin, L)).astype(np.float32)
    w = (rng.standard_normal((cin, cout)) / np.sqrt(cin)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    lin = fused.pack(_dev(w, device), _dev(b, device))
    x = _dev(xs, device)
    flat = torch.empty(xs.size, dtype=torch.float32, device=device)       # the two-source form: both tensors in one allocation
    xa, xb = flat[:B * csplit * L].view(B, csplit, L), flat[B * csplit * L:].view(B, cin - csplit, L)
    xa.copy_(x[:, :csplit]); xb.copy_(x[:, csplit:])
    ab = _dev(rng.standard_normal((B, cin, 2)).astype(np.float32), device)
    ldw = (cout + 127) // 128 * 128
    bias_bc = torch.zeros(B, ldw, device=device)
    bias_bc[:, :cout] = _dev(b, device)

    def run():
        res = {"mlp": fused.pointwise_mlp(x, lin, fused.ACT_RELU, out=torch.full((B, cout, L), -1.0, device=device))}
        with knob("captra_pw_set_pair", 0):
            res["mlp unpaired"] = fused.pointwise_mlp(x, lin, fused.ACT_RELU, out=torch.full((B, cout, L), -1.0, device=device))
        res["mlp2"] = fused.pointwise_mlp2(xa, xb, lin, fused.ACT_RELU)
        assert res["mlp2"] is not None
        pm = torch.full((B, L, cout), -1.0, device=device)
        _lib.call("captra_pointwise_mlp_pm", B, cin, cout, L, x.data_ptr(), lin.wt.data_ptr(), lin.bias.data_ptr(), fused.ACT_RELU, pm.data_ptr())
        res["pm"] = pm
        cb = torch.full((B, cout, L), -1.0, device=device)
        _lib.call("captra_pointwise_mlp_cb", B, cin, cout, L, x.data_ptr(), lin.wt.data_ptr(), bias_bc.data_ptr(), fused.ACT_RELU, cb.data_ptr())
        res["cb"] = cb
        res["gn"] = fused.pointwise_mlp_gn(x, lin, act=fused.ACT_RELU)
        res["gn ab"] = fused.pointwise_mlp_gn(x, lin, ab_in=ab, act=fused.ACT_RELU)
        res["gn stats"], res["gn stats.s"] = fused.pointwise_mlp_gn(x, lin, want_stats=True)
        res["gn ab stats"], res["gn ab stats.s"] = fused.pointwise_mlp_gn(x, lin, ab_in=ab, want_stats=True)
        return res
    want = run()
    ref = O.pointwise_mlp(xs[:1], w, b, 1)[0]
    for occ in (2, 3):
        with knob("captra_pw_set_occupancy", occ):
            got = run()                                                # (a launch refused for its LDS raises: a finding, not a skip)
        for key in want:
            assert torch.equal(got[key], want[key]), (occ, key)
        for key in ("mlp", "mlp unpaired", "mlp2", "cb", "gn"):
            np.testing.assert_array_equal(got[key][0].cpu().numpy(), ref, err_msg=f"occupancy {occ}, {key}")
        np.testing.assert_array_equal(got["pm"][0].cpu().numpy().T, ref, err_msg=f"occupancy {occ}, pm")


# ---- B.6 the generic SA kernel with its sub-tile width forced (sa_fused.hip:964-971)
@pytest.mark.parametrize("k", [32, 64])
def test_sa_generic_kernel_forced_sub_tile_width(device, k):
    """captra_sa_fused_set_wn(1 | 2) under captra_sa_fused_set_mode(1), odd widths (5 + 3 -> 40 -> 37 -> 70), 7 centres: the last
    workgroup's 128 positions are ragged.  Both widths give the oracle's bits; a width whose LDS exceeds 160 KiB must raise and write
    nothing (none does at this shape: the condition is restated)."""
    from captra_amd import _lib, fused
    case = (5, (40, 37, 70), 100, 7, k, 2)
    cfeat, chans, n, m, _, B = case
    ref = _sl_reference(*case)
    pad32 = lambda c: (c + 31) & ~31                                  # noqa: E731
    rows = max(pad32(cfeat + 3), pad32(chans[1])) + pad32(chans[0])
    lds = {wn: (256 * 4 + 3 * 256 + rows * 32 * wn) * 4 for wn in (1, 2)}       # sa_fused.hip:962-963 (SF_MAXC 256, SF_POS 128)
    outs = {}
    for wn in (0, 1, 2):
        with knob("captra_sa_fused_set_mode", 1), knob("captra_sa_fused_set_wn", wn):
            out = torch.full((B, chans[2] + 9, m), -1.0, device=device)
            if wn and lds[wn] > 160 * 1024:
                with pytest.raises(_lib.CaptraHipError):
                    _sl_launch(device, case, out=out)
                assert bool((out == -1).all()), wn
                continue
            outs[wn] = _sl_launch(device, case, out=out)
        _block_is_ref(outs[wn], ref, (case, wn))
    assert set(outs) == {0, 1, 2}                                       # 40 and 72 KiB: neither width is refused here
    assert torch.equal(outs[1], outs[0]) and torch.equal(outs[2], outs[0])
    assert torch.equal(_sl_launch(device, case), outs[0])               # back on the heuristic (no instantiated shape: the same kernel)


# ---- B.7 staging shapes of group_points and query_and_group: exactly the values tools/bench_group.py and tools/bench_qg.py sweep
GROUP_SHAPES = [(64, 32, 0), (64, 32, 8192), (64, 16, 0), (32, 16, 0), (32, 16, 8192), (48, 24, 0), (16, 8, 0), (16, 8, 8192), (32, 8, 0), (64, 32, 16384)]


@pytest.mark.parametrize("c,n,m,k,B", [(3, 300, 37, 32, 2), (6, 4096, 20, 64, 2), (323, 512, 16, 64, 3), (5, 100, 7, 3, 2)])
def test_group_points_staging_shapes(device, c, n, m, k, B):
    """captra_group_set_shape (staging budget KiB, channels per workgroup, positions per workgroup) over the tool's tuples; the last
    shape has npos % 4 != 0: the scalar kernel.  Against a numpy gather; the floats behind the output keep the sentinel."""
    from captra_amd import _lib
    rng = np.random.default_rng(c + n)
    feat = rng.standard_normal((B, c, n)).astype(np.float32)
    idx = rng.integers(0, n, (B, m, k)).astype(np.int32)
    ref = np.stack([feat[i][:, idx[i].reshape(-1)] for i in range(B)]).reshape(B, c, m, k)
    assert ((m * k) % 4 != 0) == ((c, n, m, k, B) == (5, 100, 7, 3, 2))
    fd, idd = _dev(feat, device), _dev(idx, device)
    size, tail = B * c * m * k, 64
    for shape in GROUP_SHAPES:
        buf = torch.full((size + tail,), -1.0, device=device)
        with knob("captra_group_set_shape", *shape):
            _lib.call("captra_group_points", B, c, n, m, k, fd.data_ptr(), idd.data_ptr(), buf.data_ptr())
        got = buf.cpu().numpy()
        assert (got[size:] == -1).all(), shape
        np.testing.assert_array_equal(got[:size].reshape(B, c, m, k), ref, err_msg=str(shape))


@pytest.mark.parametrize("c,use_xyz", [(0, True), (3, True), (3, False), (320, True), (320, False)])
@pytest.mark.parametrize("k", [32, 64])
def test_query_and_group_staging_shapes(device, k, c, use_xyz):
    """captra_query_and_group_set_shape over the tool's combinations (centres per workgroup | threads << 8, staged channels |
    channels per workgroup << 8): the grouped tensor and the lists against the default shape, against ball_query +
    grouping_operation and against the oracle's lists."""
    from captra_amd import fused
    from captra_amd.pointnet_lib import pointnet2_utils as pn
    n, m, B, r = 700, 41, 2, 0.2
    rng = np.random.default_rng(k + c)
    xyz = (rng.random((B, n, 3), dtype=np.float32) - 0.5).astype(np.float32)
    new_xyz = xyz[:, :m].copy()
    feat = rng.standard_normal((B, c, n)).astype(np.float32) if c else None
    xd, nd, fd = _dev(xyz, device), _dev(new_xyz, device), (_dev(feat, device) if c else None)
    if c < 8:
        combos = [(mcb, nt, 0, 0) for mcb in (16, 32) for nt in (256, 512)]
    else:
        combos = [(mcb, 256, cc, cs) for mcb in (16, 32) for cc in (8, 16) for cs in (cc, 48, 96, 192, 323)]
    combos = [q for q in combos if q[0] * k <= 8192]
    idx_ref = O.ball_query(r, k, xyz, new_xyz)
    idx2 = pn.ball_query(r, k, xd, nd)
    np.testing.assert_array_equal(idx2.cpu().numpy(), idx_ref)
    gx = pn.grouping_operation(xd.transpose(1, 2).contiguous(), idx2) - nd.transpose(1, 2).unsqueeze(-1)
    two_ops = gx if c == 0 else (torch.cat([pn.grouping_operation(fd, idx2), gx], dim=1) if use_xyz else pn.grouping_operation(fd, idx2))
    want, want_idx = fused.query_and_group(r, k, xd, nd, fd, use_xyz, want_idx=True)
    assert torch.equal(want, two_ops) and torch.equal(want_idx, idx2)
    for mcb, nt, cc, cs in combos:
        with knob("captra_query_and_group_set_shape", mcb | (nt << 8), cc | (cs << 8)):
            got, got_idx = fused.query_and_group(r, k, xd, nd, fd, use_xyz, want_idx=True)
        assert torch.equal(got, want), (mcb, nt, cc, cs)
        assert torch.equal(got_idx, want_idx), (mcb, nt, cc, cs)


# ================================================================================================ C. grids that are the CU count
JOBS = ["cus-1", "cus", "cus+1", "2cus+1"]


def _jobs(device, j):
    cus = _cus(device)
    return {"cus-1": cus - 1, "cus": cus, "cus+1": cus + 1, "2cus+1": 2 * cus + 1}[j]


@pytest.mark.parametrize("j", JOBS)
def test_chain_x6_job_count_around_the_cu_count(device, j):
    """chain_x6.hip:256-258: a job is four waves x 32 positions, the grid min(jobs, CUs).  One cloud of 128 j positions; positions are
    independent, so the call equals the same positions run as two calls on the two halves, bit for bit (equality with the f32x6
    judge is held in tests/test_x6_gpu.py)."""
    from captra_amd import fused
    nj = _jobs(device, j)
    L, c0 = 128 * nj, 131
    assert (1 * ((L + 31) // 32) + 3) // 4 == nj
    rng = np.random.default_rng(7)
    dims = (c0, 128, 128, 128)
    layers = [fused.pack(_dev((rng.standard_normal((dims[i], dims[i + 1])) / np.sqrt(dims[i])).astype(np.float32), device),
                         _dev(rng.standard_normal(dims[i + 1]).astype(np.float32), device)) for i in range(3)]
    x = _dev(rng.standard_normal((1, c0, L)).astype(np.float32), device)
    whole = fused.mlp_chain3_x6(x, layers)
    h = 128 * (nj // 2)
    halves = torch.cat([fused.mlp_chain3_x6(x[:, :, :h].contiguous(), layers), fused.mlp_chain3_x6(x[:, :, h:].contiguous(), layers)], dim=2)
    assert whole.shape == (1, 128, L) and torch.equal(whole, halves)


@pytest.mark.parametrize("j", JOBS)
@pytest.mark.parametrize("cfeat,chans,waves", [(3, (32, 32, 64), 8), (320, (128, 128, 256), 4)])
def test_sa_x6_job_count_around_the_cu_count(device, cfeat, chans, waves, j):
    """sa_x6.hip:441-444: a job is `waves` centres (8 for the small-input shapes, 4 for the SA2 ones: the SX_CASE table), the grid
    min(jobs, CUs).  One cloud of waves x j centres against the two halves of the centres as two calls."""
    from captra_amd import fused
    nj = _jobs(device, j)
    n, k, m = 64, 32, waves * nj
    assert (1 * m + waves - 1) // waves == nj
    rng = np.random.default_rng(cfeat + nj)
    xyz_cn = _dev(rng.random((1, 3, n), dtype=np.float32) - 0.5, device)
    feat = _dev(rng.standard_normal((1, cfeat, n)).astype(np.float32), device)
    new_xyz = _dev(rng.random((1, m, 3), dtype=np.float32) - 0.5, device)
    idx = _dev(rng.integers(0, n, (1, m, k)).astype(np.int32), device)
    dims = (cfeat + 3,) + chans
    layers = [fused.pack(_dev((rng.standard_normal((dims[i], dims[i + 1])) / np.sqrt(dims[i])).astype(np.float32), device),
                         _dev(rng.standard_normal(dims[i + 1]).astype(np.float32), device)) for i in range(3)]

    def run(m0, m1):
        out = torch.full((1, chans[2] + 9, m1 - m0), -1.0, device=device)
        fused.sa_scale_x6(feat, xyz_cn, new_xyz[:, m0:m1].contiguous(), idx[:, m0:m1].contiguous(), layers, out, PAD)
        assert bool((out[:, :PAD] == -1).all()) and bool((out[:, PAD + chans[2]:] == -1).all())
        assert bool((out[:, PAD:PAD + chans[2]] >= 0).all())             # behind the ReLU: the whole block was written
        return out
    h = waves * (nj // 2)
    assert torch.equal(run(0, m), torch.cat([run(0, h), run(h, m)], dim=2))
