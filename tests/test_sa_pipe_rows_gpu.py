"""The pipelined SA2 kernel's (128, 196, 256) shape (csrc/sa_pipe.hip): layer 2's rows 192..195 run on the vector pipe as two
v_fma_f32 chains per lane beside the six whole MFMA tiles.  The arithmetic is the same k-ascending fmaf chain from the bias, so
every output keeps its bits:

  * shapes: one slice per centre and one centre per wave (M = 4, K = 32: the launcher takes M * K in multiples of 128, so M = 1
    exists at K = 128 only), two and four slices, a static walk with more centres than resident waves, and the (128, 128, 256) shape;
  * row isolation: W3 zero except its input rows 192..195 (W2's rows 192..195 at distinct magnitudes), and the complement;
  * special values reaching rows 192..195: pre-activations of exactly +0 and -0, negative ones, subnormal ones (W2's rows and b2
    scaled by 2^-130: v_fma_f32 must not flush where the MFMA does not), +-Inf and NaNs in v1 and in W2;
  * the slice-per-wave split, the dynamic centre hand-out and the level's two scales in one launch (sa_wave_pipe2_kernel).

Finite cases are held to the CPU oracle (gather -> 3 x pointwise_mlp -> max over K) with assert_array_equal and to the
previous-generation kernel (fused.sa_scale_pre) with torch.equal; non-finite ones to fused.sa_scale_pre: NaN at the same positions,
every other element bit-equal.  Every case prints what it measured before it asserts.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import ops as O

pytestmark = pytest.mark.gpu
CF = 320
WIDE, NARROW = (128, 196, 256), (128, 128, 256)
PAD = 4          # channel offset of the scale's block in the output tensor


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _f32(pattern):
    return np.array([pattern], np.uint32).view(np.float32)[0]


@functools.lru_cache(maxsize=None)
def _inputs(chans, n, m, k, B):
    rng = np.random.default_rng(sum(chans) + 7 * n + 3 * m + k + B)
    xyz_cn = rng.random((B, 3, n), dtype=np.float32) - 0.5
    feat = rng.standard_normal((B, CF, n)).astype(np.float32)
    new_xyz = rng.random((B, m, 3), dtype=np.float32) - 0.5
    idx = rng.integers(0, n, (B, m, k)).astype(np.int32)
    dims = (CF + 3,) + chans
    layers = tuple(((rng.standard_normal((dims[i], dims[i + 1])) / np.sqrt(dims[i])).astype(np.float32),
                    rng.standard_normal(dims[i + 1]).astype(np.float32)) for i in range(3))
    return xyz_cn, feat, new_xyz, idx, layers


def _oracle(xyz_cn, feat, new_xyz, idx, layers):
    x = O.sa_group(feat, xyz_cn, new_xyz, idx)
    for w, b in layers:
        x = O.pointwise_mlp(x, w, b, 1)
    return O.max_over_k(x)


@functools.lru_cache(maxsize=None)
def _reference(chans, n, m, k, B):
    """The oracle's output on the unmodified inputs of a shape: computed once, shared, never written to."""
    ref = _oracle(*_inputs(chans, n, m, k, B))
    ref.setflags(write=False)
    return ref


def _run(device, xyz_cn, feat, new_xyz, idx, layers, route="pipe", poison_v1=None):
    """One SA scale through `route`: "pipe" = the pipelined kernel, "pre" = the previous-generation kernel, "multi" = the scale
    twice in one call of captra_sa_scales_multi (with the (128, 128, 256) scale first where the scale is the wide one: the level's
    two scales in one launch).  `poison_v1` = [(cloud, point, channel, value)] written into the pre-transformed first layer."""
    from captra_amd import fused
    packed = [fused.pack(_dev(w, device), _dev(b, device)) for w, b in layers]
    B, m, k = idx.shape
    c3 = layers[2][0].shape[1]
    fd, xd, nd, idd = _dev(feat, device), _dev(xyz_cn, device), _dev(new_xyz, device), _dev(idx, device)
    out = torch.full((B, c3 + 9, m), -1.0, device=device)
    if route == "pre":
        assert fused.sa_scale_pre_supported(CF, packed, k)
        v1 = fused.sa_first_layer_pre(fd, packed[0])
        for cloud, point, ch, val in poison_v1 or ():
            v1[cloud, ch, point] = float(val)
        fused.sa_scale_pre(v1, xd, nd, idd, packed, out, PAD, CF)
    else:
        assert fused.sa_scale_pipe_supported(CF, packed, m, k, b=B, n=xyz_cn.shape[2])
        v1pm = fused.sa_first_layer_pre_pm(fd, packed[0])
        for cloud, point, ch, val in poison_v1 or ():
            v1pm[cloud, point, ch] = float(val)
        if route == "pipe":
            fused.sa_scale_pre_pm(v1pm, xd, nd, idd, packed, out, PAD, CF)
        else:
            assert route == "multi"
            return _run_multi(device, fd, xd, nd, packed, v1pm, idd, c3)
    got = out.cpu().numpy()
    assert (got[:, :PAD] == -1).all() and (got[:, PAD + c3:] == -1).all(), route
    return got[:, PAD:PAD + c3]


def _run_multi(device, fd, xd, nd, packed_wide, v1pm_wide, idd_wide, c3):
    """The level's two scales recorded as jobs and launched by captra_sa_scales_multi: the narrow scale (its own weights, K = 64)
    into the first channel block, the wide one into the second.  Returns the wide block."""
    from captra_amd import fused
    B, m, _ = idd_wide.shape
    rng = np.random.default_rng(5)
    dims = (CF + 3,) + NARROW
    packed_n = [fused.pack(_dev((rng.standard_normal((dims[i], dims[i + 1])) / np.sqrt(dims[i])).astype(np.float32), device),
                           _dev(rng.standard_normal(dims[i + 1]).astype(np.float32), device)) for i in range(3)]
    idd_n = _dev(rng.integers(0, xd.shape[2], (B, m, 64)).astype(np.int32), device)
    v1pm_n = fused.sa_first_layer_pre_pm(fd, packed_n[0])
    out = torch.zeros((B, NARROW[2] + c3, m), device=device)
    alone = torch.full_like(out, -1.0)
    fused.sa_scale_pre_pm(v1pm_n, xd, nd, idd_n, packed_n, alone, 0, CF)
    jobs = []
    with fused.L.launch_options(sa_prezeroed=1):
        fused.sa_scale_pre_pm(v1pm_n, xd, nd, idd_n, packed_n, out, 0, CF, jobs=jobs)
        fused.sa_scale_pre_pm(v1pm_wide, xd, nd, idd_wide, packed_wide, out, NARROW[2], CF, jobs=jobs)
        assert len(jobs) == 2
        fused.sa_scales_multi(jobs, device)
    assert torch.equal(out[:, :NARROW[2]], alone[:, :NARROW[2]])          # the narrow scale next to it: what its own launch gives
    return out.cpu().numpy()[:, NARROW[2]:]


def _same_as_pre(what, got, pre):
    """The way the NaN / Inf tests compare two kernels: NaN at the same positions, every other element bit-equal."""
    nan_g, nan_p = np.isnan(got), np.isnan(pre)
    diff = (_bits(got) != _bits(pre)) & ~nan_g & ~nan_p
    print(f"sa_pipe rows {what}: NaN outputs {int(nan_g.sum())} (previous-generation kernel {int(nan_p.sum())}), NaN positions that differ "
          f"{int((nan_g != nan_p).sum())}, Inf outputs {int(np.isinf(got).sum())}, other elements with different bits {int(diff.sum())} of {got.size}")
    assert not (nan_g != nan_p).any(), what
    assert not diff.any(), what


# the smallest shapes that take every walk: M = 4, K = 32 is one slice per centre and one centre per wave; (200, 6, 64, 3) two
# slices; (96, 5, 128, 2) four; (64, 128, 32, 9) is 1152 centres on at most 1024 resident waves (K = 32 never splits): a static walk
# in which waves take a second centre; the last case is the other SA2 shape, whose layer 2 has no remainder rows
SHAPES = [(WIDE, 64, 4, 32, 1), (WIDE, 200, 6, 64, 3), (WIDE, 96, 5, 128, 2), (WIDE, 64, 128, 32, 9), (NARROW, 200, 6, 64, 3)]


@pytest.mark.parametrize("chans,n,m,k,B", SHAPES)
def test_sa_pipe_rows_shapes_bit_exact(device, chans, n, m, k, B):
    """The pipelined kernel == the oracle's gather -> 3 layers -> max, bit for bit, and == the previous-generation kernel."""
    inp = _inputs(chans, n, m, k, B)
    got = _run(device, *inp)
    ref = _reference(chans, n, m, k, B)
    print(f"sa_pipe rows shape {(chans, n, m, k, B)}: outputs off the oracle's bits {int((_bits(got) != _bits(ref)).sum())} of {got.size}")
    np.testing.assert_array_equal(got, ref)
    assert torch.equal(torch.from_numpy(got), torch.from_numpy(_run(device, *inp, route="pre")))


@pytest.mark.parametrize("only_rows", [True, False])
def test_sa_pipe_rows_isolated(device, only_rows):
    """W3 zero except its input rows 192..195, W2's rows 192..195 at distinct magnitudes: the output depends on the vector-pipe rows
    only.  And the complement (W3's rows 192..195 zero): on the matrix-pipe rows only."""
    xyz_cn, feat, new_xyz, idx, layers = _inputs(WIDE, 200, 6, 64, 3)
    (w1, b1), (w2, b2), (w3, b3) = [(w.copy(), b.copy()) for w, b in layers]
    w2[:, 192:196] *= np.array([1.0, 3.0, 1.0 / 7.0, 11.0], np.float32)
    if only_rows:
        w3[:192] = 0.0
    else:
        w3[192:196] = 0.0
    mod = ((w1, b1), (w2, b2), (w3, b3))
    got = _run(device, xyz_cn, feat, new_xyz, idx, mod)
    ref = _oracle(xyz_cn, feat, new_xyz, idx, mod)
    print(f"sa_pipe rows isolated (only rows 192..195 = {only_rows}): outputs off the oracle's bits {int((_bits(got) != _bits(ref)).sum())} of "
          f"{got.size}; outputs that differ from the bias alone {int((got != np.maximum(b3, 0)[None, :, None]).sum())}")
    assert (got != np.maximum(b3, 0)[None, :, None]).any()          # the rows reach the output
    np.testing.assert_array_equal(got, ref)
    assert torch.equal(torch.from_numpy(got), torch.from_numpy(_run(device, xyz_cn, feat, new_xyz, idx, mod, route="pre")))


def test_sa_pipe_rows_zero_and_negative_preactivations(device):
    """Row 192: every weight and the bias +0, the pre-activation is +0.  Row 193: every weight and the bias -0, it is -0 (the
    activations are >= 0).  Row 194: weights -|w| and a negative bias, it is negative everywhere.  Row 195 stays as it is."""
    xyz_cn, feat, new_xyz, idx, layers = _inputs(WIDE, 200, 6, 64, 3)
    (w1, b1), (w2, b2), (w3, b3) = [(w.copy(), b.copy()) for w, b in layers]
    w2[:, 192], b2[192] = 0.0, 0.0
    w2[:, 193], b2[193] = -0.0, -0.0
    w2[:, 194], b2[194] = -np.abs(w2[:, 194]), -abs(b2[194])
    w3[192:196] *= 8.0
    mod = ((w1, b1), (w2, b2), (w3, b3))
    got = _run(device, xyz_cn, feat, new_xyz, idx, mod)
    ref = _oracle(xyz_cn, feat, new_xyz, idx, mod)
    print(f"sa_pipe rows +0 / -0 / negative pre-activations: outputs off the oracle's bits {int((_bits(got) != _bits(ref)).sum())} of {got.size}")
    np.testing.assert_array_equal(_bits(got), _bits(ref))
    assert torch.equal(torch.from_numpy(got), torch.from_numpy(_run(device, xyz_cn, feat, new_xyz, idx, mod, route="pre")))


def test_sa_pipe_rows_subnormal_preactivations(device):
    """W2's rows 192..195 and their biases scaled by 2^-130: their pre-activations are subnormal.  With W3 zero elsewhere and b3 = 0
    the outputs are subnormal products of them: a flush on the vector pipe would show as zeros."""
    xyz_cn, feat, new_xyz, idx, layers = _inputs(WIDE, 200, 6, 64, 3)
    (w1, b1), (w2, b2), (w3, b3) = [(w.copy(), b.copy()) for w, b in layers]
    tiny = np.float32(2.0 ** -130)
    w2[:, 192:196] *= tiny
    b2[192:196] *= tiny
    w3[:192] = 0.0
    b3[:] = 0.0
    mod = ((w1, b1), (w2, b2), (w3, b3))
    got = _run(device, xyz_cn, feat, new_xyz, idx, mod)
    ref = _oracle(xyz_cn, feat, new_xyz, idx, mod)
    sub = (got != 0) & (np.abs(got) < np.finfo(np.float32).tiny)
    print(f"sa_pipe rows subnormal pre-activations: {int(sub.sum())} of {got.size} outputs subnormal and non-zero (oracle "
          f"{int(((ref != 0) & (np.abs(ref) < np.finfo(np.float32).tiny)).sum())}), off the oracle's bits {int((_bits(got) != _bits(ref)).sum())}")
    assert sub.any()
    np.testing.assert_array_equal(_bits(got), _bits(ref))
    assert torch.equal(torch.from_numpy(got), torch.from_numpy(_run(device, xyz_cn, feat, new_xyz, idx, mod, route="pre")))


POISONS = {"inf_pos": 0x7F800000, "inf_neg": 0xFF800000, "nan": 0x7FC00000}


@pytest.mark.parametrize("name", list(POISONS))
def test_sa_pipe_rows_non_finite_in_v1(device, name):
    """A poisoned source point in the pre-transformed first layer (four of its channels, so that +Inf under weights of both signs
    meets in rows 192..195), gathered by the first and the last neighbour slot of a centre in the middle cloud."""
    xyz_cn, feat, new_xyz, idx, layers = _inputs(WIDE, 200, 6, 64, 3)
    idx = idx.copy()
    point = 17
    idx[1, 2, 0] = idx[1, 2, 63] = idx[1, 5, 31] = point
    val = _f32(POISONS[name])
    poison = [(1, point, ch, val) for ch in (0, 37, 64, 127)]
    clean = _run(device, xyz_cn, feat, new_xyz, idx, layers)
    got = _run(device, xyz_cn, feat, new_xyz, idx, layers, poison_v1=poison)
    pre = _run(device, xyz_cn, feat, new_xyz, idx, layers, route="pre", poison_v1=poison)
    print(f"sa_pipe rows {name} in v1: outputs changed by the poison {int((_bits(got) != _bits(clean)).sum())}; other clouds changed "
          f"{int((_bits(got[[0, 2]]) != _bits(clean[[0, 2]])).sum())}")
    _same_as_pre(f"{name} in v1", got, pre)
    np.testing.assert_array_equal(_bits(got[[0, 2]]), _bits(clean[[0, 2]]))        # the other clouds keep their bits


@pytest.mark.parametrize("name", list(POISONS) + ["nan_neg"])
def test_sa_pipe_rows_non_finite_in_w2(device, name):
    """One weight of each of W2's rows 192..195 (a different input row each) is +Inf / -Inf / a NaN of either sign: 0 x Inf where the
    activation is 0, Inf elsewhere, Inf - Inf across positions of layer 3."""
    xyz_cn, feat, new_xyz, idx, layers = _inputs(WIDE, 200, 6, 64, 3)
    (w1, b1), (w2, b2), (w3, b3) = [(w.copy(), b.copy()) for w, b in layers]
    val = _f32(0xFFC00000 if name == "nan_neg" else POISONS[name])
    for r, krow in enumerate((0, 63, 64, 127)):
        w2[krow, 192 + r] = val
    mod = ((w1, b1), (w2, b2), (w3, b3))
    clean = _run(device, xyz_cn, feat, new_xyz, idx, layers)
    got = _run(device, xyz_cn, feat, new_xyz, idx, mod)
    pre = _run(device, xyz_cn, feat, new_xyz, idx, mod, route="pre")
    changed = int((_bits(got) != _bits(clean)).sum())
    print(f"sa_pipe rows {name} in W2 rows 192..195: outputs changed by the poison {changed}")
    _same_as_pre(f"{name} in W2", got, pre)
    if name != "nan_neg":             # (a sign-set NaN is 0 behind the integer ReLU: the documented exception; it may change nothing)
        assert changed > 0


@pytest.mark.parametrize("route", ["split", "static", "dynamic", "multi"])
def test_sa_pipe_rows_other_walks(device, route):
    """The slice-per-wave split (forced), the static walk over four slices per centre (split off), the dynamic centre hand-out and
    the level's two scales in one launch: the oracle's bits."""
    from captra_amd import _lib
    shape = (WIDE, 96, 5, 128, 2) if route in ("split", "static") else (WIDE, 200, 6, 64, 3)
    inp = _inputs(*shape)
    ref = _reference(*shape)
    if route in ("split", "static"):
        _lib.lib().captra_sa_fused_set_split(ctypes.c_int(2 if route == "split" else 0))
        try:
            got = _run(device, *inp)
        finally:
            _lib.lib().captra_sa_fused_set_split(ctypes.c_int(1))
    elif route == "dynamic":
        pool = torch.full((2,), 12345, dtype=torch.int32, device=device)
        _lib.lib().captra_sa_fused_set_split(ctypes.c_int(0))
        try:
            with _lib.launch_options(dyn_pool=(pool.data_ptr(), 2)):
                got = _run(device, *inp)
        finally:
            _lib.lib().captra_sa_fused_set_split(ctypes.c_int(1))
        counts = pool.cpu().tolist()
        print(f"sa_pipe rows dynamic hand-out: counter slots {counts}")
        assert counts[0] >= shape[4] * shape[2] and counts[1] == 12345, counts      # the launch took its centres from the counter
    else:
        got = _run(device, *inp, route="multi")
    print(f"sa_pipe rows {route}: outputs off the oracle's bits {int((_bits(got) != _bits(ref)).sum())} of {got.size}")
    np.testing.assert_array_equal(got, ref)
