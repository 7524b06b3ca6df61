"""The bf16 kernels (csrc/bf16_mlp.hip, dense_bf16.hip, tile_bf16.hip, sa_bf16.hip, neck_bf16.hip; `fused.use_mlp_dtype("bf16")`) held to
bit-exact checks on integer lattices.  The loose tests (tests/test_model_gpu.py, test_tile_bf16_gpu.py, test_neck_gpu.py) pin these
kernels to each other bit for bit and to the float64 contract within statistical bounds on N(0,1) data, which cannot see a wrong
rounding rule, a rounding in the wrong place, or an error confined to a ragged tail, one slot of the channel permutation or one
neighbour of a max-pool.  The judge is tests/bf16_judge.py (proven by tests/test_bf16_judge_cpu.py, which also runs every case
builder of this file on the CPU: the share conditions and the 2^24 bound are asserted where a case is built).

Families (the judge's header): S nothing rounds (data movement; its outputs are small, so it is also the statistics' family),
T the hand-over or the bf16 store rounds with ties of both parities, W weights and fp32 inputs round, G the on-load GroupNorm
operand bf16(relu(fma(a, x, b))) rounds, with negative a.  Every lattice comparison is an equality.  The one tolerance is the
sigmoid head's 1e-6 (tests/test_x6_edges_gpu.py::test_coord_tail_lattice_bits): its raw input is an exact multiple of 2^-6.

Notes on scope:
  * captra_pointwise_mlp_bf16_pm is reached through sa_scale_bf16's 320-channel shapes (the first layer's feature part).
  * neck_chain kind 2 takes the interpolation weights as given (`nn=`): dyadic weights on features that are multiples of 4 make the
    interpolation exact, so FP2's interpolation IS part of the exact claim.
  * sa1_stream_bf16 has no lattices of its own: tests/test_l1_stream_gpu.py pins it bit for bit to the three launches covered here,
    and its scan and ticket logic are not arithmetic.
  * head12: `ab1` is given by the test (family G), so gn_finalize is not part of the exact claim.
  * The wrappers allocate their outputs themselves; `_poison` leaves a block of the same size filled with a sentinel in the
    allocator's cache just before, so that an element the kernel does not write shows (best effort).  Where the entry point takes
    the output tensor it is filled with the sentinel directly, with guard channels around the written range.
(e) containment: one NaN / one +Inf at a single input element changes no bit of any output that does not depend on it.  What the
dependent elements hold is not asserted.  Observed on the MI355X: see the comment above the containment tests.
"""
import contextlib
import ctypes
import zlib

import numpy as np
import pytest
import torch

from tests import bf16_judge as J
from tests.test_model_gpu import _dense_to_pm, _pm_to_dense

pytestmark = pytest.mark.gpu
SENT = -7.0
ACT_NONE, ACT_RELU = 0, 1


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _rng(*parts):
    return np.random.default_rng(zlib.crc32(repr(parts).encode()))


def _pack(device, lay, wscale=None, bscale=None):
    """The layer on the device; wscale (scalar or (cin,1)) / bscale: exact power-of-two factors on the weights / the bias."""
    from captra_amd import fused
    w = lay.w if wscale is None else lay.w * np.asarray(wscale, np.float32)
    b = lay.b if bscale is None else lay.b * np.float32(bscale)
    return fused.pack(_dev(_f32(w), device), _dev(_f32(b), device))


def _poison(device, shape, dtype):
    """A freed block of the output's size, full of the sentinel, for the wrapper's torch.empty to pick up."""
    t = torch.full(tuple(shape), SENT, dtype=dtype, device=device)
    del t


@contextlib.contextmanager
def _launches(name, n):
    """The profiler's launch counter of `name` goes up by exactly n inside the block: no silent route to another kernel."""
    from captra_amd import _lib
    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        yield
    finally:
        _lib.prof_enable(False)
    assert _lib.prof_read(name)[1] == n, (name, _lib.prof_read(name)[1], n)


def _eq(got, ref, msg=""):
    np.testing.assert_array_equal(got, np.asarray(ref).astype(np.float32), err_msg=msg)


def _chunk_stats(y, P):
    """y integers (B,c,L) -> (B,T,c,2) int64: (sum, sum of squares) per chunk of P positions; every partial sum is below 2^24."""
    B, c, L = y.shape
    T = (L + P - 1) // P
    pad = np.zeros((B, c, T * P), np.int32)
    pad[:, :, :L] = y
    t = pad.reshape(B, c, T, P)
    out = np.stack([t.sum(-1, dtype=np.int64), (t * t).sum(-1, dtype=np.int64)], axis=-1).transpose(0, 2, 1, 3)
    assert np.abs(t).sum(-1, dtype=np.int64).max() < J.LIMIT and out[..., 1].max() < J.LIMIT
    return out


# ---- the entry points: numpy in, numpy out ------------------------------------------------------------------------------------------------
def run_pw(device, x, lay, act):
    """fused.pointwise_mlp in the bf16 mode (captra_pointwise_mlp_bf16): fp32 in, fp32 out."""
    from captra_amd import fused
    B, _, L = x.shape
    out = torch.full((B, lay.cout, L), SENT, device=device)
    with fused.use_mlp_dtype("bf16"), _launches("pointwise_mlp", 1):
        fused.pointwise_mlp(_dev(_f32(x), device), _pack(device, lay), act, out=out)
    return out.cpu().numpy()


def _ab(device, ab):
    return None if ab is None else _dev(_f32(np.stack([ab[0], ab[1]], axis=-1)), device)


def _pm_raw(t):
    """A point-major tensor as it lies in memory, (B,ceil32(c),L) fp32 in slot order, padding included (containment: the padding of
    a poisoned position is poisoned too, through 0 * NaN)."""
    return np.ascontiguousarray(t.float().cpu().numpy().transpose(0, 2, 1))


def run_pm(device, x, lay, in_pm, out_pm, act=ACT_NONE, ab=None, stats=False, bias_bc=None, raw=False):
    """fused.pointwise_mlp_bf16pm / _cloud_bias (csrc/dense_bf16.hip) -> (y (B,cout,L) fp32 numpy, stats (B,T,cout,2) or None)."""
    from captra_amd import fused
    B, _, L = x.shape
    xd = _dense_to_pm(_f32(x)).to(device) if in_pm else _dev(_f32(x), device)
    lin = _pack(device, lay)
    _poison(device, (B, L, fused.pm_channels(lay.cout)) if out_pm else (B, lay.cout, L), torch.bfloat16 if out_pm else torch.float32)
    st = None
    with _launches("pointwise_mlp", 1):
        if bias_bc is not None:
            assert not in_pm and ab is None and not stats
            y = fused.pointwise_mlp_bf16pm_cloud_bias(xd, lin, L, _dev(_f32(bias_bc), device), out_pm, act)
        elif stats:
            y, st = fused.pointwise_mlp_bf16pm(xd, lin, L, in_pm, True, ab=_ab(device, ab), act=act, with_stats=True)
            st = st.cpu().numpy()
        else:
            y = fused.pointwise_mlp_bf16pm(xd, lin, L, in_pm, out_pm, ab=_ab(device, ab), act=act)
    if raw:
        return _pm_raw(y), st
    return (_pm_to_dense(y, lay.cout) if out_pm else y.cpu().numpy()), st


def run_tile(device, x, lay, in_cm, out_mode, act=ACT_NONE, ab=None, stats=False, bias_bc=None, csplit=None):
    """fused.dense_bf16_tile (captra_dense_bf16_tile_ex) -> (y (B,cout,L) or (B,cout,1) fp32 numpy, stats or None)."""
    from captra_amd import fused
    B, _, L = x.shape
    lin = _pack(device, lay)
    x2 = None
    if in_cm:
        xa = _dev(_f32(x), device)
        xd = xa if csplit is None else xa[:, :csplit].contiguous()
        x2 = None if csplit is None else xa[:, csplit:].contiguous()
    else:
        xd = _dense_to_pm(_f32(x)).to(device)
        assert fused.dense_bf16_tile_supported(xd, lin)
    shape = {fused.OUT_PM: (B, L, fused.pm_channels(lay.cout)), fused.OUT_CM: (B, lay.cout, L), fused.OUT_MAX: (B, lay.cout, 1)}[out_mode]
    _poison(device, shape, torch.bfloat16 if out_mode == fused.OUT_PM else torch.float32)
    with _launches("pointwise_mlp", 1):
        res = fused.dense_bf16_tile(xd, lin, ab=_ab(device, ab), act=act, with_stats=stats, x2=x2, l=L, out_mode=out_mode,
                                    bias_bc=None if bias_bc is None else _dev(_f32(bias_bc), device))
    y, st = res if stats else (res, None)
    return (_pm_to_dense(y, lay.cout) if out_mode == fused.OUT_PM else y.cpu().numpy()), (None if st is None else st.cpu().numpy())


def run_gemv(device, v, lay):
    from captra_amd import fused
    _poison(device, (v.shape[0], lay.cout), torch.float32)
    return fused.gemv_bf16(_dev(_f32(v), device), _pack(device, lay)).cpu().numpy()


def run_chain(device, x, layers, fused_launch, heads=None, head_scale=None):
    """fused.mlp_chain_bf16 (layer by layer) or fused.mlp_chain_bf16_fused (one launch) -> the (B,128,L) feature map held by the bf16
    point-major tensor, or (seg, nocs) with heads."""
    from captra_amd import fused
    xd = _dev(_f32(x), device)
    packed = [_pack(device, lay) for lay in layers]
    with fused.use_mlp_dtype("bf16"):
        if not fused_launch:
            assert fused.chain_tile_bf16_supported(x.shape[1], x.shape[2], packed) == (x.shape[2] % 4 == 0)      # which kernels run it
            return _pm_to_dense(fused.mlp_chain_bf16(xd, packed, [ACT_RELU] * len(layers), out_pm=True), layers[-1].cout)
        hp = None if heads is None else [_pack(device, heads[0]), _pack(device, heads[1]), _pack(device, heads[2], head_scale, head_scale)]
        assert fused.chain_bf16_supported(xd, packed, hp)
        with _launches("mlp_chain3", 1):
            res = fused.mlp_chain_bf16_fused(xd, packed, hp)
    if heads is None:
        assert res.channels == 128
        return _pm_to_dense(res.data, 128)
    return res[0].cpu().numpy(), res[1].cpu().numpy()


def run_sa(device, feat, xyz_cn, new_xyz, idx, layers, xyz_scale, variant):
    """fused.sa_scale_bf16 -> (B,c3,M); the output tensor has four channels in front and five behind, which must stay untouched.
    xyz_scale: the factor on the first layer's xyz rows (the coordinates are the lattice's integers divided by it)."""
    from captra_amd import _lib, fused
    cfeat = 0 if feat is None else feat.shape[1]
    sc = np.ones((cfeat + 3, 1), np.float32)
    sc[cfeat:] = xyz_scale
    packed = [_pack(device, layers[0], sc), _pack(device, layers[1]), _pack(device, layers[2])]
    c3 = layers[2].cout
    B, M, K = idx.shape
    out = torch.full((B, c3 + 9, M), SENT, device=device)
    with fused.use_mlp_dtype("bf16"):
        assert fused.sa_scale_bf16_supported(cfeat, packed, K)
        _lib.lib().captra_sa_bf16_set_variant(ctypes.c_int(variant))
        try:
            with _launches("sa_scale_fused", 1):
                fused.sa_scale_bf16(None if feat is None else _dev(_f32(feat), device), _dev(_f32(xyz_cn), device), _dev(_f32(new_xyz), device),
                                    _dev(idx.astype(np.int32), device), packed, out, 4)
        finally:
            _lib.lib().captra_sa_bf16_set_variant(ctypes.c_int(0))
    got = out.cpu().numpy()
    assert (got[:, :4] == SENT).all() and (got[:, 4 + c3:] == SENT).all()
    return got[:, 4:4 + c3]


def run_neck(device, kind, x, layers, x2=None, nn=None, v=None, v_lay=None, csplit=None):
    from captra_amd import fused
    packed = [_pack(device, lay) for lay in layers]
    B, _, L = x.shape
    with fused.use_mlp_dtype("bf16"):
        assert fused.neck_chain_supported(layers[0].cin, L, packed, x.shape[1] if csplit is None else csplit, kind)
        _poison(device, (B, layers[-1].cout, 1 if kind == 0 else L), torch.float32)
        with _launches("neck_chain", 1):
            y = fused.neck_chain(kind, _dev(_f32(x), device), packed, x2=None if x2 is None else _dev(_f32(x2), device),
                                 nn=None if nn is None else (_dev(nn[0].astype(np.int32), device), _dev(_f32(nn[1]), device)),
                                 v=None if v is None else _dev(_f32(v), device), v_rows=None if v_lay is None else _pack(device, v_lay))
    return y.cpu().numpy()


# ---- shapes (the smallest that reach every code path) and case builders (numpy only: tests/test_bf16_judge_cpu.py runs them all) ----------
# (cin, cout, L, B): ragged L 77 / 129 / 333 and a multiple of 128; cin off the 16 / 32 grid; cout 3 and 70, below and above 64; 256
# and 512 outputs are the shared-operand forms of the on-load GroupNorm (8 and 16 row tiles)
DENSE = [(40, 70, 77, 2), (134, 3, 129, 1), (515, 64, 333, 3), (128, 256, 256, 1), (96, 512, 77, 2)]
TILE = [c for c in DENSE if c[1] >= 64]
TILE_CM = [(40, 17, 70, 76, 2), (515, 3, 64, 332, 3), (134, 134, 32, 128, 1), (128, 100, 256, 256, 1)]     # (cin, csplit, cout, L, B)
GEMV = [(1, 40, 70), (3, 515, 3), (2, 134, 256)]                                                           # (B, cin, cout)
HEAD12 = [(2, 96, 77), (1, 128, 256), (40, 128, 770), (10, 128, 3205), (3, 40, 10885)]   # (B, cin, l): from the third on, B * ceil(l / 128) > 256 CUs
CHAIN = [(128, 77, 2), (134, 333, 1), (134, 256, 3)]                                     # (c0, l, B): 8 and 9 input k-steps
CHAIN_HEADS = [(134, 2, 3, 333, 2), (128, 4, 12, 77, 1)]                                 # (c0, seg, nocs, l, B)
# (cfeat, (c1, c2, c3), K, B, N, M): all eight instantiated shapes; M = 37 does not fill a workgroup's waves, M = 1 a single centre
SA = [(0, (32, 32, 64), 32, 2, 300, 37), (3, (32, 32, 64), 32, 1, 512, 128), (0, (64, 64, 128), 64, 1, 256, 128),
      (3, (64, 64, 128), 64, 3, 300, 37), (0, (64, 96, 128), 128, 2, 256, 37), (3, (64, 96, 128), 128, 1, 200, 1),
      (320, (128, 128, 256), 64, 2, 333, 128), (320, (128, 196, 256), 128, 1, 200, 37)]
PERIOD = 331             # head12's long clouds repeat a base of 331 positions (prime: no alignment with the 128-position tiles)


def dense_case(family, cin, cout, L, B, relu, tag="dense"):
    """One layer: (lay, x, ref) with ref the fp32 result as int64; the share conditions of the family asserted."""
    rng = _rng(tag, family, cin, cout, L)
    (lay,), make_x = J.lattice(family, (cin, cout), 0, rng)
    x = make_x((B,), L)
    ref = J.forward([lay], x, [relu])[0]
    if family == "S":
        assert np.abs(ref).max() <= J.SMALL and np.abs(x).max() <= J.SMALL
    elif family == "T":
        J.assert_shares(ref, (tag, cin, cout))
    else:
        J.assert_shares(lay.vals, (tag, "w", cin, cout))
        J.assert_shares(x, (tag, "x", cin, cout))
    return lay, x, ref


def affine_dense_case(cin, cout, L, B, small=False, tag="affine"):
    """Family G in front of one layer of small weights: (lay, x, (a, b), ref)."""
    rng = _rng(tag, cin, cout, L, small)
    x, a, b = J.affine_case(rng, (B,), cin, L, small=small)
    if small:                                                  # |operand| <= 30: |y| <= 3 * 2 * 30 + 16
        lay = J.dense_small_layer(rng, cin, cout, nnz=3, wmax=2)
    else:                                                      # every input channel is read by some column
        lay = J.dense_small_layer(rng, cin, cout, nnz=max(2, -(-cin // cout)), wmax=2)
        op = J.affine_operand(x, a, b)
        J.assert_shares(op, (tag, cin, cout))
        assert (a < 0).mean() > 0.25 and ((op == 0) & (x > 0)).mean() > 0.02      # the ReLU kills positive x under a negative a
    ref = J.forward([lay], x, [False], ab=[(a, b)])[0]
    if small:
        assert np.abs(ref).max() <= J.SMALL
    return lay, x, (a, b), ref


def head12_case(B, cin, l, small):
    """x of small integers, W1, (a1, b1) of family G on y1 -- the hand-over under test -- and W2 a layer of small weights; small: every
    value stays below 256 instead (for the statistics).  Clouds longer than PERIOD repeat a base of PERIOD positions from an offset
    per cloud: -> (lay1, lay2, base x (cin,P), (a, b), y1 (512,P), y2 (B,512,P), pos (B,l))."""
    rng = _rng("head12", B, cin, l, small)
    P = min(l, PERIOD)
    shape = (B, 512)
    if small:
        lay1 = J.dense_small_layer(rng, cin, 512, nnz=4, wmax=2)           # |y1| <= 4 * 2 * 3 + 16 = 40
        base = rng.integers(-3, 4, (cin, P))
        a = J._signs(rng, shape)
        b = rng.integers(-8, 17, shape)                                     # operand <= 56, |y2| <= 2 * 2 * 56 + 16 = 240
    else:
        (lay1,), make_x = J.lattice("S", (cin, 512), 0, rng)
        base = make_x((), P)
        a = (1 << rng.integers(1, 3, shape)) * J._signs(rng, shape)
        b = rng.integers(300, 800, shape)
    lay2 = J.dense_small_layer(rng, 512, 512, nnz=2, wmax=2)
    y1 = J.forward([lay1], base, [False])[0]                                # (512, P)
    y1b = np.broadcast_to(y1, (B, 512, P))
    if not small:
        J.assert_shares(J.affine_operand(y1b, a, b), ("head12", B, cin, l))
        assert (a < 0).mean() > 0.25
    y2 = J.forward([lay2], y1b, [False], ab=[(a, b)])[0]                    # (B, 512, P)
    if small:
        assert np.abs(y1).max() <= J.SMALL and 8 < np.abs(y2).max() <= J.SMALL
    pos = (np.arange(l)[None, :] + 37 * np.arange(B)[:, None]) % P
    return lay1, lay2, base, (a, b), y1, y2, pos


def chain_case(family, c0, l, B, target):
    rng = _rng("chain", family, c0, l, target)
    layers, make_x = J.lattice(family, (c0, 128, 128, 128), target, rng, last_signed=False)
    x = make_x((B,), l)
    outs = J.forward(layers, x, [True] * 3)
    if family == "T":
        J.assert_shares(outs[target], ("chain", c0, l, target))
    elif family == "W":
        J.assert_shares(layers[target].vals, ("chain w", c0, target))
        if target == 0:
            J.assert_shares(x, ("chain x", c0))
    else:
        assert max(np.abs(o).max() for o in outs) <= J.SMALL
    return layers, x, outs


def chain_heads_case(family, c0, seg_dim, nocs_dim, l, B, target):
    """The trunk with the family's weights in layer `target` (0 .. 2), or -- target 3 -- in the segmentation head itself (trunk: S).
    The NOCS branch: hidden = a +1 selection, out = a +-1 selection times 2^-6 (its bias an integer times 2^-6)."""
    rng = _rng("chain-heads", family, c0, seg_dim, l, target)
    if target < 3:
        layers, make_x = J.lattice(family, (c0, 128, 128, 128), target, rng, last_signed=False)
        seg = J.dense_small_layer(rng, 128, seg_dim, nnz=4, wmax=3)
    else:
        layers, make_x = J.lattice("S", (c0, 128, 128, 128), 0, rng, last_signed=False)
        (seg,), _ = J.lattice(family if family == "W" else "S", (128, seg_dim), 0, rng)
    x = make_x((B,), l)
    outs = J.forward(layers, x, [True] * 3)
    feat = J.rne(outs[2])                                                   # the heads read the bf16 hand-over of layer 3
    seg_ref = J.forward([seg], feat, [False])[0]
    hid = J._select_layer(rng, 128, 128, signed=False)
    out = J._select_layer(rng, 128, nocs_dim, signed=True)
    out = J.LatticeLayer(128, nocs_dim, out.rows, out.vals, rng.integers(-64, 65, nocs_dim))
    raw = J.forward([hid, out], feat, [True, False])[1].astype(np.float64) * 2.0 ** -6
    return layers, (seg, hid, out), x, seg_ref, 1.0 / (1.0 + np.exp(-raw)) - 0.5


def sa_case(family, cfeat, chans, K, B, N, M, target):
    """Integer features, coordinates on the grid of multiples of 2^-6 (the lattice sees 64 (xyz[idx] - centre)), neighbour lists as
    given: random with repeats, and for every third centre a short list padded with its first entry (what the ball query writes).
    -> (layers, feat, xyz_cn, new_xyz, idx, ref (B,c3,M)); the first layer's xyz rows go to the device times 64."""
    rng = _rng("sa", family, cfeat, chans, K, M, target)
    layers, make_x = J.lattice(family, (cfeat + 3,) + chans, target, rng, last_signed=False)
    pts = make_x((B,), N)                                                    # (B, cfeat + 3, N): feature rows, then the grid coordinates
    r = int(min(32, max(1, (np.abs(pts).max() if family != "W" else 64) // 2)))
    pts[:, cfeat:] = rng.integers(-r, r + 1, (B, 3, N))
    ctr = rng.integers(-r, r + 1, (B, M, 3))
    idx = rng.integers(0, N, (B, M, K))
    short = np.arange(M) % 3 == 2
    fill = rng.integers(1, K, M)
    pad = short[None, :, None] & (np.arange(K)[None, None, :] >= fill[None, :, None])
    idx = np.where(pad, idx[:, :, :1], idx)
    g = np.stack([pts[b][:, idx[b]] for b in range(B)])                      # (B, cfeat + 3, M, K)
    g[:, cfeat:] -= np.moveaxis(ctr, 2, 1)[:, :, :, None]
    outs = J.forward(layers, g.reshape(B, cfeat + 3, M * K), [True] * 3)
    if family == "T":
        J.assert_shares(outs[target], ("sa", cfeat, chans, target))
    elif family == "W":
        J.assert_shares(layers[target].vals, ("sa w", cfeat, chans, target))
    else:
        assert max(np.abs(o).max() for o in outs) <= J.SMALL
    ref = J.pool(outs[2], K)
    feat = pts[:, :cfeat] if cfeat else None
    return layers, feat, pts[:, cfeat:] / 64.0, ctr / 64.0, idx, ref


NECK = [(0, "S"), (0, "T"), (1, "S"), (1, "T"), (2, "S"), (2, "T")]


def neck_case(kind, family):
    """kind 0 (SA3): [x (B,3,L); x2 (B,37,L)] -> 128 -> 384 -> 800, relu, max over L = 76 positions (two tiles of 64, the second ragged).
    kind 1 (FP3): x (B,40,132) -> 128 -> 96 with the first layer's bias of cloud b = b1 + W_v bf16(v[b]), v (B,70).
    kind 2 (FP2): [x (B,17,200); interpolated x2 (B,23,50)] -> 256 -> 64, weights (1/2, 1/4, 1/4) and (1, 0, 0) on multiples of 4.
    The family's weights sit in the first layer (T: its hand-over rounds)."""
    rng = _rng("neck", kind, family)
    if kind == 0:
        B, L, widths, csplit = 2, 76, (40, 128, 384, 800), 3
    elif kind == 1:
        B, L, widths, csplit = 3, 132, (40, 128, 96), 40
    else:
        B, L, widths, csplit = 2, 200, (40, 256, 64), 17
    layers, make_x = J.lattice(family, widths, 0, rng, last_signed=False)
    xc = make_x((B,), L)
    case = {"layers": layers, "csplit": csplit}
    bias_bc = None
    if kind == 1:
        v_lay = J.dense_small_layer(rng, 70, 128, nnz=2, wmax=1)
        v_lay = J.LatticeLayer(70, 128, v_lay.rows, v_lay.vals, layers[0].bias)          # (the rows of v share the layer's bias)
        v = rng.integers(-1, 2, (B, 70, 1)) if family == "S" else rng.integers(-31, 32, (B, 70, 1))
        bias_bc = J.forward([v_lay], v, [False])[0]                                      # (B,128,1) = b1 + W_v v
        case.update(v=v[:, :, 0], v_lay=v_lay)
    if kind == 2:
        S = 50
        known = 4 * rng.integers(-(np.abs(xc).max() // 4), np.abs(xc).max() // 4 + 1, (B, 40 - csplit, S))
        nidx = rng.integers(0, S, (B, L, 3))
        nw = np.where((np.arange(L) % 2 == 0)[None, :, None], np.float32([0.5, 0.25, 0.25]), np.float32([1.0, 0.0, 0.0]))
        nw = nw * np.ones((B, 1, 1), np.float32)
        f = np.stack([known[b][:, nidx[b]] for b in range(B)])                           # (B, c2, L, 3)
        interp = (f[..., 0] * 2 + f[..., 1] + f[..., 2]) // 4
        interp = np.where((np.arange(L) % 2 == 0)[None, None, :], interp, f[..., 0])
        assert ((f[..., 0] * 2 + f[..., 1] + f[..., 2]) % 4 == 0).all()
        xc[:, csplit:] = interp
        case.update(x2=known, nn=(nidx, nw))
    elif kind == 0:
        case.update(x2=xc[:, csplit:])
    case["x"] = xc[:, :csplit]
    n = len(layers)
    if bias_bc is None:
        outs = J.forward(layers, xc, [True] * n)
    else:
        l0 = J.LatticeLayer(widths[0], widths[1], layers[0].rows, layers[0].vals, np.zeros(widths[1], np.int64))
        y0 = J.forward([l0], xc, [False])[0]
        assert np.abs(y0).max() + np.abs(bias_bc).max() < J.LIMIT
        h0 = np.maximum(y0 + bias_bc, 0)
        outs = [h0] + J.forward(layers[1:], h0, [True] * (n - 1))
    if family == "T":
        J.assert_shares(outs[0], ("neck", kind))
    else:
        assert max(np.abs(o).max() for o in outs) <= J.SMALL
    case["ref"] = outs[-1].max(-1, keepdims=True) if kind == 0 else outs[-1]
    return case


def all_cases():
    """Every (builder, arguments) this file runs on the GPU -- for the CPU proof of the share conditions and the 2^24 bound."""
    for c in DENSE:
        for fam in "SWT":
            for relu in (False, True):
                yield dense_case, (fam,) + c + (relu,)
        yield affine_dense_case, c
        yield affine_dense_case, c + (True,)
    for cin, csplit, cout, L, B in TILE_CM:
        for fam in "SWT":
            yield dense_case, (fam, cin, cout, L, B, True, "tile-cm")
    for B, cin, cout in GEMV:
        for fam in "SW":
            yield dense_case, (fam, cin, cout, 1, B, False, "gemv")
    for c in HEAD12:
        for small in (False, True):
            yield head12_case, c + (small,)
    for c in CHAIN:
        yield chain_case, ("S",) + c + (0,)
        yield chain_case, ("W",) + c + (0,)
        for t in range(3):
            yield chain_case, ("T",) + c + (t,)
    for c in CHAIN_HEADS:
        for fam, t in (("S", 3), ("W", 3), ("T", 2), ("T", 0)):
            yield chain_heads_case, (fam,) + c + (t,)
    for c in SA:
        for fam, t in (("S", 0), ("T", 0), ("T", 1), ("W", 0), ("W", 2)):
            yield sa_case, (fam,) + c + (t,)
    for c in NECK:
        yield neck_case, c


# ==== captra_pointwise_mlp_bf16 (fused.pointwise_mlp in the bf16 mode) =================================================================
@pytest.mark.parametrize("family", "SW")
@pytest.mark.parametrize("cin,cout,L,B", DENSE)
def test_pointwise_mlp_bf16_lattice_bits(device, cin, cout, L, B, family):
    for relu in (False, True):
        lay, x, ref = dense_case(family, cin, cout, L, B, relu)
        _eq(run_pw(device, x, lay, ACT_RELU if relu else ACT_NONE), ref, f"relu={relu}")


# ==== csrc/dense_bf16.hip ==============================================================================================================
@pytest.mark.parametrize("family", "SWT")
@pytest.mark.parametrize("cin,cout,L,B", DENSE)
def test_bf16pm_layouts_lattice_bits(device, cin, cout, L, B, family):
    """captra_pointwise_mlp_bf16pm in its four layout combinations, ReLU off and on: the fp32 output == int64, the bf16 output == its
    RNE rounding (family T: ties of both parities among the stored values).  A bf16 input tensor holds the RNE rounding of the
    lattice's input, which is what the fp32 form rounds to on load: all four forms must give the same numbers."""
    for relu in (False, True):
        lay, x, ref = dense_case(family, cin, cout, L, B, relu)
        act = ACT_RELU if relu else ACT_NONE
        for in_pm in (False, True):
            xin = J.rne(x) if in_pm else x
            _eq(run_pm(device, xin, lay, in_pm, False, act)[0], ref, f"relu={relu} in_pm={in_pm} fp32 out")
            _eq(run_pm(device, xin, lay, in_pm, True, act)[0], J.rne(ref), f"relu={relu} in_pm={in_pm} bf16 out")


@pytest.mark.parametrize("cin,cout,L,B", DENSE)
def test_bf16pm_statistics_and_cloud_bias_bits(device, cin, cout, L, B):
    """Family S (outputs <= 255): the statistics epilogue's (sum, sum of squares) per chunk of 64 positions are integers below 2^24 --
    every order of adding them gives the same bits; captra_gn_stats_bf16pm on the stored input (chunks of 128); a bias per cloud."""
    from captra_amd import fused
    lay, x, ref = dense_case("S", cin, cout, L, B, False)
    for in_pm in (False, True):
        y, st = run_pm(device, x, lay, in_pm, True, stats=True)
        _eq(y, ref)
        _eq(st, _chunk_stats(ref, 64), f"in_pm={in_pm}")
    if 256 % (fused.pm_channels(cin) // 8) == 0:
        got = fused.gn_stats_bf16pm(_dense_to_pm(_f32(x)).to(device), cin).cpu().numpy()
        _eq(got, _chunk_stats(x, 128).transpose(0, 2, 1, 3))
    if cout % 32 == 0:
        rng = _rng("cloud-bias", cin, cout)
        bias_bc = rng.integers(-16, 17, (B, cout))
        for relu in (False, True):
            want = J.act(ref - lay.bias[None, :, None] + bias_bc[:, :, None], relu)
            for out_pm in (False, True):
                _eq(run_pm(device, x, lay, False, out_pm, ACT_RELU if relu else ACT_NONE, bias_bc=bias_bc)[0], want, f"relu={relu} out_pm={out_pm}")


@pytest.mark.parametrize("cin,cout,L,B", DENSE)
def test_bf16pm_groupnorm_on_load_bits(device, cin, cout, L, B):
    """Family G: the operand is bf16(relu(fma(a, x, b))) with a = +-2^e, ties of both parities among fma's results; fp32 and bf16
    outputs.  With small values (nothing rounds) the statistics epilogue is exact as well."""
    lay, x, ab, ref = affine_dense_case(cin, cout, L, B)
    _eq(run_pm(device, x, lay, True, False, ab=ab)[0], ref, "fp32 out")
    _eq(run_pm(device, x, lay, True, True, ab=ab)[0], J.rne(ref), "bf16 out")
    _eq(run_pm(device, x, lay, True, True, ACT_RELU, ab=ab)[0], J.rne(np.maximum(ref, 0)), "bf16 out, relu")
    lay, x, ab, ref = affine_dense_case(cin, cout, L, B, small=True)
    y, st = run_pm(device, x, lay, True, True, ab=ab, stats=True)
    _eq(y, ref)
    _eq(st, _chunk_stats(ref, 64))


# ==== csrc/tile_bf16.hip ===============================================================================================================
@pytest.mark.parametrize("family", "SWT")
@pytest.mark.parametrize("cin,cout,L,B", TILE)
def test_tile_point_major_input_lattice_bits(device, cin, cout, L, B, family):
    """captra_dense_bf16_tile_ex on a bf16 point-major input: OUT_PM / OUT_CM / OUT_MAX (L <= 128), ReLU off and on."""
    from captra_amd import fused
    for relu in (False, True):
        lay, x, ref = dense_case(family, cin, cout, L, B, relu)
        act = ACT_RELU if relu else ACT_NONE
        xin = J.rne(x)
        _eq(run_tile(device, xin, lay, False, fused.OUT_PM, act)[0], J.rne(ref), f"relu={relu} OUT_PM")
        _eq(run_tile(device, xin, lay, False, fused.OUT_CM, act)[0], ref, f"relu={relu} OUT_CM")
        if L <= 128:
            _eq(run_tile(device, xin, lay, False, fused.OUT_MAX, act)[0], ref.max(-1, keepdims=True), f"relu={relu} OUT_MAX")


@pytest.mark.parametrize("family", "SWT")
@pytest.mark.parametrize("cin,csplit,cout,L,B", TILE_CM)
def test_tile_channel_major_input_lattice_bits(device, cin, csplit, cout, L, B, family):
    """... on an fp32 channel-major input, as one tensor and as two tensors standing for their concat (`x2=`), all three outputs."""
    from captra_amd import fused
    lay, x, ref = dense_case(family, cin, cout, L, B, True, "tile-cm")
    for cs in (None, csplit) if csplit < cin else (None,):
        _eq(run_tile(device, x, lay, True, fused.OUT_PM, ACT_RELU, csplit=cs)[0], J.rne(ref), f"csplit={cs} OUT_PM")
        _eq(run_tile(device, x, lay, True, fused.OUT_CM, ACT_RELU, csplit=cs)[0], ref, f"csplit={cs} OUT_CM")
        if L <= 128:
            _eq(run_tile(device, x, lay, True, fused.OUT_MAX, ACT_RELU, csplit=cs)[0], ref.max(-1, keepdims=True), f"csplit={cs} OUT_MAX")


@pytest.mark.parametrize("cin,cout,L,B", TILE)
def test_tile_groupnorm_statistics_and_cloud_bias_bits(device, cin, cout, L, B):
    """Family G on load (bf16 output, with ties), `with_stats=` on small outputs (chunks of 128 positions), `bias_bc=`."""
    from captra_amd import fused
    lay, x, ab, ref = affine_dense_case(cin, cout, L, B)
    _eq(run_tile(device, x, lay, False, fused.OUT_PM, ab=ab)[0], J.rne(ref), "G")
    _eq(run_tile(device, x, lay, False, fused.OUT_PM, ACT_RELU, ab=ab)[0], J.rne(np.maximum(ref, 0)), "G relu")
    lay, x, ab, ref = affine_dense_case(cin, cout, L, B, small=True)
    y, st = run_tile(device, x, lay, False, fused.OUT_PM, ab=ab, stats=True)
    _eq(y, ref)
    _eq(st, _chunk_stats(ref, 128), "G small stats")
    lay, x, ref = dense_case("S", cin, cout, L, B, False)
    y, st = run_tile(device, x, lay, False, fused.OUT_PM, stats=True)
    _eq(y, ref)
    _eq(st, _chunk_stats(ref, 128), "S stats")
    if cout % 32 == 0:
        bias_bc = _rng("tile-cb", cin, cout).integers(-16, 17, (B, cout))
        want = np.maximum(ref - lay.bias[None, :, None] + bias_bc[:, :, None], 0)
        _eq(run_tile(device, x, lay, False, fused.OUT_PM, ACT_RELU, bias_bc=bias_bc)[0], want, "bias_bc")
        if L % 4 == 0:
            _eq(run_tile(device, x, lay, True, fused.OUT_CM, ACT_RELU, bias_bc=bias_bc)[0], want, "bias_bc, channel-major")


@pytest.mark.parametrize("family", "SW")
@pytest.mark.parametrize("B,cin,cout", GEMV)
def test_gemv_lattice_bits(device, B, cin, cout, family):
    lay, v, ref = dense_case(family, cin, cout, 1, B, False, "gemv")
    _eq(run_gemv(device, v[:, :, 0], lay), ref[:, :, 0])


@pytest.mark.parametrize("B,cin,l", HEAD12)
def test_head12_lattice_bits(device, B, cin, l):
    """captra_head12_bf16: y1 = W1 x + b1 (never stored) -> bf16(relu(fma(a1, y1, b1'))) -> y2, stored bf16.  Family G on the hand-over
    (y2's bits exact, ties included), then small values: y1's statistics (the statistics pass), y2 and y2's statistics all exact.
    The last three shapes have more tiles than the MI355X has CUs: the persistent form (asserted below through the knob: with it
    switched off the result must not change, and the launcher's own rule B * ceil(l / 128) > CUs is restated)."""
    from captra_amd import _lib, fused
    bi = torch.arange(B, device=device)[:, None]
    for small in (False, True):
        lay1, lay2, base, ab, y1, y2, pos = head12_case(B, cin, l, small)
        lin1, lin2 = _pack(device, lay1), _pack(device, lay2)
        post = _dev(pos, device)
        xpm = _dense_to_pm(_f32(base[None])).to(device)[0][post].contiguous()                # (B, l, ceil32(cin))
        assert fused.head12_bf16_supported(xpm, lin1, lin2)
        _poison(device, (B, l, 512), torch.bfloat16)
        with _launches("pointwise_mlp", 1):
            y2pm, st2 = fused.head12_bf16(xpm, lin1, _ab(device, ab), lin2)
        want = _dense_to_pm(J.rne(y2).astype(np.float32)).to(device)[bi, post]               # (B, l, 512)
        assert torch.equal(y2pm.view(torch.int16), want.view(torch.int16)), f"small={small}"
        if small:
            expand = lambda t: np.take_along_axis(t.astype(np.int32), pos[:, None, :], axis=2)      # noqa: E731  (B,512,P) -> (B,512,l)
            _eq(fused.head12_bf16_stats(xpm, lin1).cpu().numpy(), _chunk_stats(expand(np.broadcast_to(y1, y2.shape)), 128), "y1 statistics")
            _eq(st2.cpu().numpy(), _chunk_stats(expand(y2), 128), "y2 statistics")
    if B * ((l + 127) // 128) > torch.cuda.get_device_properties(device).multi_processor_count:
        _lib.lib().captra_tile_bf16_set_persistent(ctypes.c_int(0))
        try:
            y2b, st2b = fused.head12_bf16(xpm, lin1, _ab(device, ab), lin2)
        finally:
            _lib.lib().captra_tile_bf16_set_persistent(ctypes.c_int(1))
        assert torch.equal(y2b.view(torch.int16), want.view(torch.int16)) and torch.equal(st2b, st2)


# ==== captra_mlp_chain_bf16 (csrc/sa_bf16.hip) and the layer-by-layer chain ============================================================
@pytest.mark.parametrize("fused_launch", [False, True])
@pytest.mark.parametrize("c0,l,B", CHAIN)
def test_chain_lattice_bits(device, c0, l, B, fused_launch):
    """fused.mlp_chain_bf16 (layer by layer: the LDS-tiled kernels where l % 4 == 0, else the streaming ones) and
    fused.mlp_chain_bf16_fused (one launch): S and W in the first layer, T with the rounding hand-over behind layer 1, 2 and 3 (the
    third is the bf16 store of the feature map)."""
    for family, target in (("S", 0), ("W", 0), ("T", 0), ("T", 1), ("T", 2)):
        layers, x, outs = chain_case(family, c0, l, B, target)
        _eq(run_chain(device, x, layers, fused_launch), J.rne(outs[2]), f"{family} target={target}")


@pytest.mark.parametrize("c0,seg_dim,nocs_dim,l,B", CHAIN_HEADS)
def test_chain_heads_lattice_bits(device, c0, seg_dim, nocs_dim, l, B):
    """... with CoordinateNet's heads: the segmentation logits == int64; sigmoid(raw) - 0.5 within 1e-6 of float64 with raw an exact
    multiple of 2^-6 (the tolerance of tests/test_x6_edges_gpu.py::test_coord_tail_lattice_bits)."""
    for family, target in (("S", 3), ("W", 3), ("T", 2), ("T", 0)):
        layers, heads, x, seg_ref, nocs_ref = chain_heads_case(family, c0, seg_dim, nocs_dim, l, B, target)
        seg, nocs = run_chain(device, x, layers, True, heads, head_scale=2.0 ** -6)
        _eq(seg, seg_ref, f"{family} target={target}")
        print(f"bf16 chain heads {family}/{target}: sigmoid head max error {np.abs(nocs - nocs_ref).max():.3e} (bound 1e-6)")
        np.testing.assert_allclose(nocs, nocs_ref, atol=1e-6, rtol=0)


# ==== captra_sa_scale_bf16 =============================================================================================================
@pytest.mark.parametrize("variant", [0, 9])
@pytest.mark.parametrize("cfeat,chans,K,B,N,M", SA)
def test_sa_lattice_bits(device, cfeat, chans, K, B, N, M, variant):
    """All eight instantiated shapes, both launch forms: S (gather, centre subtraction, slot order, max over K with repeated and
    padded neighbours), T with the rounding hand-over behind layer 1 and behind layer 2, W in layer 1 (feature inputs of 9 to 12 bits
    round at load) and in layer 3."""
    for family, target in (("S", 0), ("T", 0), ("T", 1), ("W", 0), ("W", 2)):
        layers, feat, xyz_cn, new_xyz, idx, ref = sa_case(family, cfeat, chans, K, B, N, M, target)
        _eq(run_sa(device, feat, xyz_cn, new_xyz, idx, layers, 64.0, variant), ref, f"{family} target={target}")


# ==== captra_neck_chain_bf16 ===========================================================================================================
@pytest.mark.parametrize("kind,family", NECK)
def test_neck_lattice_bits(device, kind, family):
    c = neck_case(kind, family)
    got = run_neck(device, kind, c["x"], c["layers"], x2=c.get("x2"), nn=c.get("nn"), v=c.get("v"), v_lay=c.get("v_lay"), csplit=c["csplit"])
    _eq(got, c["ref"])


# ==== (e) containment ==================================================================================================================
# Observed on the MI355X (not asserted): behind a ReLU a poisoned position does not stay NaN.  With one NaN (either sign) in x, every
# real output channel of that position reads 0 -- in the fp32 stores (fmaxf(NaN, 0) = 0) and in the bf16 stores, where the packed ReLU
# on bf16 bits (a signed 16-bit max with 0) turns a NaN whose sign bit is set into +0; it keeps a NaN whose sign bit is clear, which
# showed in the PADDING channels of the poisoned position (zero weights: 0 * NaN) of the first shape below.  One +-Inf gives +Inf
# in the channels whose weight has its sign and 0 in the others after one layer, and all zeros behind the three layers of the chain
# (Inf - Inf = NaN in the second layer, then as above).  So a NaN in the input can come out as a plausible 0 at its own position;
# what the tests assert is that it never reaches another one.
POISON = [np.float32(np.nan), np.float32(np.inf)]


def _same_bits(a, b, msg=""):
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32), err_msg=msg)


def _random_layer(rng, cin, cout):
    w = (rng.standard_normal((cin, cout)) / np.sqrt(cin)).astype(np.float32)
    lay = J.LatticeLayer(cin, cout, np.zeros((1, cout), np.int64), np.zeros((1, cout), np.int64), np.zeros(cout, np.int64))
    lay.w, lay.b = w, rng.standard_normal(cout).astype(np.float32)
    return lay


def _positions_kept(y, yp, b0, p0, msg=""):
    B, _, L = y.shape
    keep = np.ones((B, L), bool)
    keep[b0, p0] = False
    _same_bits(yp.transpose(0, 2, 1)[keep], y.transpose(0, 2, 1)[keep], msg)


@pytest.mark.parametrize("cin,cout,L,B", [DENSE[0], DENSE[2]])
def test_dense_containment(device, cin, cout, L, B):
    """One poisoned input element: every other position and cloud keeps its bits -- captra_pointwise_mlp_bf16, the streaming kernel
    (fp32 and bf16 inputs and outputs; the statistics of every other chunk) and the tiled kernel (bf16 input; fp32 input on the
    whole quads of positions it takes)."""
    from captra_amd import fused
    rng = _rng("dense-poison", cin, cout, L)
    x = rng.standard_normal((B, cin, L)).astype(np.float32)
    lay = _random_layer(rng, cin, cout)
    b0, k0, p0 = B - 1, cin - 3, L - 2
    Lt = L // 4 * 4
    runs = {"pw": lambda v: run_pw(device, v, lay, ACT_RELU),
            "pm fp32": lambda v: run_pm(device, v, lay, False, False, ACT_RELU)[0],
            "pm bf16": lambda v: run_pm(device, v, lay, False, True, ACT_RELU, raw=True)[0],
            "pm in": lambda v: run_pm(device, J.bf16_rne(v), lay, True, True, ACT_RELU, raw=True)[0],
            "tile pm in": lambda v: run_tile(device, J.bf16_rne(v), lay, False, fused.OUT_CM, ACT_RELU)[0],
            "tile": lambda v: run_tile(device, v[:, :, :Lt], lay, True, fused.OUT_CM, ACT_RELU)[0]}
    for name, run in runs.items():
        y = run(x)
        for bad in POISON:
            xp = x.copy()
            xp[b0, k0, p0 if name != "tile" else Lt - 2] = bad
            _positions_kept(y, run(xp), b0, p0 if name != "tile" else Lt - 2, f"{name} {bad}")
    y, st = run_pm(device, x, lay, False, True, stats=True, raw=True)
    for bad in POISON:
        xp = x.copy()
        xp[b0, k0, p0] = bad
        _, stp = run_pm(device, xp, lay, False, True, stats=True, raw=True)
        keep = np.ones((B, st.shape[1]), bool)
        keep[b0, p0 // 64] = False
        _same_bits(stp[keep], st[keep], f"stats {bad}")


def test_gemv_containment(device):
    rng = _rng("gemv-poison")
    v = rng.standard_normal((3, 134)).astype(np.float32)
    lay = _random_layer(rng, 134, 70)
    y = run_gemv(device, v, lay)
    for bad in POISON:
        vp = v.copy()
        vp[1, 77] = bad
        _same_bits(run_gemv(device, vp, lay)[[0, 2]], y[[0, 2]])


@pytest.mark.parametrize("B,cin,l", HEAD12[:1])
def test_head12_containment(device, B, cin, l):
    from captra_amd import fused
    rng = _rng("head12-poison", B, cin, l)
    lin1, lin2 = _pack(device, _random_layer(rng, cin, 512)), _pack(device, _random_layer(rng, 512, 512))
    x = J.bf16_rne(rng.standard_normal((B, cin, l)).astype(np.float32))
    ab = _dev(np.stack([rng.uniform(0.5, 1.5, (B, 512)), rng.standard_normal((B, 512)) * 0.3], axis=-1).astype(np.float32), device)
    y = fused.head12_bf16(_dense_to_pm(x).to(device), lin1, ab, lin2)[0].view(torch.int16).cpu().numpy()      # (B, l, 512), slot order
    b0, p0 = B - 1, l - 5
    keep = np.ones((B, l), bool)
    keep[b0, p0] = False
    for bad in POISON:
        xp = x.copy()
        xp[b0, cin - 1, p0] = bad
        yp = fused.head12_bf16(_dense_to_pm(xp).to(device), lin1, ab, lin2)[0].view(torch.int16).cpu().numpy()
        np.testing.assert_array_equal(yp[keep], y[keep], err_msg=str(bad))


@pytest.mark.parametrize("c0,seg_dim,nocs_dim,l,B", CHAIN_HEADS[:1])
def test_chain_containment(device, c0, seg_dim, nocs_dim, l, B):
    rng = _rng("chain-poison", c0, l)
    x = rng.standard_normal((B, c0, l)).astype(np.float32)
    layers = [_random_layer(rng, c, 128) for c in (c0, 128, 128)]
    heads = [_random_layer(rng, 128, seg_dim), _random_layer(rng, 128, 128), _random_layer(rng, 128, nocs_dim)]
    feat = run_chain(device, x, layers, True)
    seg, nocs = run_chain(device, x, layers, True, heads)
    lbl = run_chain(device, x, layers, False)
    b0, k0, p0 = B - 1, c0 - 1, l - 33
    for bad in POISON:
        xp = x.copy()
        xp[b0, k0, p0] = bad
        _positions_kept(feat, run_chain(device, xp, layers, True), b0, p0, f"feat {bad}")
        _positions_kept(lbl, run_chain(device, xp, layers, False), b0, p0, f"layer by layer {bad}")
        segp, nocsp = run_chain(device, xp, layers, True, heads)
        _positions_kept(seg, segp, b0, p0, f"seg {bad}")
        _positions_kept(nocs, nocsp, b0, p0, f"nocs {bad}")


@pytest.mark.parametrize("cfeat,chans,K,B,N,M", [SA[0], SA[3], SA[6]])
def test_sa_containment(device, cfeat, chans, K, B, N, M):
    """One poisoned coordinate (and, with features, one poisoned feature) of one point: every centre whose neighbour list does not
    name the point, and every other cloud, keeps its bits."""
    rng = _rng("sa-poison", cfeat, chans, K, M)
    xyz_cn = (rng.random((B, 3, N)) - 0.5).astype(np.float32)
    feat = rng.standard_normal((B, cfeat, N)).astype(np.float32) if cfeat else None
    new_xyz = (rng.random((B, M, 3)) - 0.5).astype(np.float32)
    idx = rng.integers(0, N, (B, M, K))
    dims = (cfeat + 3,) + chans
    layers = [_random_layer(rng, dims[i], dims[i + 1]) for i in range(3)]
    b0, n0 = B - 1, N // 3
    y = run_sa(device, feat, xyz_cn, new_xyz, idx, layers, 1.0, 0)
    keep = np.ones((B, M), bool)
    keep[b0] = ~(idx[b0] == n0).any(-1)
    assert keep[b0].any()
    for bad in POISON:
        for where in (("xyz",) if feat is None else ("xyz", "feat")):
            xp, fp = xyz_cn.copy(), None if feat is None else feat.copy()
            if where == "xyz":
                xp[b0, 1, n0] = bad
            else:
                fp[b0, cfeat - 1, n0] = bad
            yp = run_sa(device, fp, xp, new_xyz, idx, layers, 1.0, 0)
            _same_bits(yp.transpose(0, 2, 1)[keep], y.transpose(0, 2, 1)[keep], f"{where} {bad}")


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_neck_containment(device, kind):
    """kind 0: the pooled vector of every other cloud; kinds 1, 2: every other position (kind 1 with the poison in x; a poisoned
    element of the cloud's vector stays in its cloud; kind 2 with the poison in a known feature: the positions that do not
    interpolate from it)."""
    rng = _rng("neck-poison", kind)
    c = neck_case(kind, "S")
    widths = (40,) + tuple(lay.cout for lay in c["layers"])
    layers = [_random_layer(rng, widths[i], widths[i + 1]) for i in range(len(widths) - 1)]
    x = rng.standard_normal(c["x"].shape).astype(np.float32)
    kw = {"csplit": c["csplit"]}
    if kind == 0:
        kw["x2"] = rng.standard_normal(c["x2"].shape).astype(np.float32)
    elif kind == 1:
        kw["v"], kw["v_lay"] = rng.standard_normal(c["v"].shape).astype(np.float32), _random_layer(rng, 70, widths[1])
        kw["v_lay"].b = layers[0].b
    else:
        kw["x2"], kw["nn"] = rng.standard_normal(c["x2"].shape).astype(np.float32), (c["nn"][0], c["nn"][1])
    y = run_neck(device, kind, x, layers, **kw)
    B, L = x.shape[0], x.shape[2]
    b0, p0 = B - 1, L - 3
    for bad in POISON:
        xp = x.copy()
        xp[b0, 1, p0] = bad
        yp = run_neck(device, kind, xp, layers, **kw)
        if kind == 0:
            _same_bits(yp[:b0], y[:b0], str(bad))
        else:
            _positions_kept(y, yp, b0, p0, str(bad))
        if kind == 1:
            vp = kw["v"].copy()
            vp[b0, 5] = bad
            _same_bits(run_neck(device, kind, x, layers, **dict(kw, v=vp))[:b0], y[:b0], f"v {bad}")
        if kind == 2:
            x2p = kw["x2"].copy()
            x2p[b0, 2, 7] = bad
            nidx, nw = kw["nn"]
            keep = np.ones((B, L), bool)
            keep[b0] = ~(nidx[b0] == 7).any(-1)
            assert keep[b0].any()
            yq = run_neck(device, kind, x, layers, **dict(kw, x2=x2p))
            _same_bits(yq.transpose(0, 2, 1)[keep], y.transpose(0, 2, 1)[keep], f"x2 {bad}")
