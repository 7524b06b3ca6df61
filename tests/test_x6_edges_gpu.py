"""The f32x6 kernels (csrc/sa_x6.hip, csrc/dense_x6.hip, csrc/chain_x6.hip, the cloud-bias form of FP3) held to bit-exact and
per-product checks; tests/test_x6_gpu.py holds them to 2e-6 of a layer's largest output on N(0,1) data, which cannot see one cross
product dropped, doubled or fed the wrong piece.  The judge is tests/x6_judge.py (proven by tests/test_x6_judge_cpu.py).  Every entry
point of the mode runs five families:

(a) integer lattices A / B / C: every piece, product and partial sum is an integer below 2^24, so every fp32 summation order gives
    the bits int64 gives -- assert_array_equal;
(b) one product at a time: a single non-zero input channel per position holding a probe value (every kept product >= 32 U |w x|,
    U = 2^-24), bias 0: |got - w x| <= (8 + 2 p) U |w x| against float64, p = the number of power-of-two "permutation" layers the value
    is passed through in a fused kernel (each within 2 U).  The 8 is derived (three dropped products + five fp32 additions, each
    <= 1 U), not tuned.  Measured on the MI355X (comment below the imports): 2.71 U dense, 2.37 U SA (p = 1), 2.38 U chain3 (p = 2),
    2.30 U coord_tail logits (p = 3), 1.00 U cloud bias (exact fp32) -- the MFMA's own rounding of a k-step's partial sums does not show;
(c) power-of-two rescaling of input channels (2^a_k on x, 2^-a_k on the weight rows) and output channels (2^g_c), a, g in [-40, 40]:
    identical bits after the exact rescaling of the first run's result.  Conditioned on every piece being a normal number (asserted
    on the CPU: smallest third piece >= 2^-120, largest value <= 2^100); what the bf16 MFMA does with SUBNORMAL pieces has not been
    measured and is deliberately out of scope;
(d) cancellation and small channels: half the output channels at 2^-14 of the rest, every position cancelling to
    |y| <= 1e-3 sum |w||x|: per ELEMENT no further from float64 than twice the exact k-ascending chain's own error + 4 U sum_k |w_k x_k|
    (in the fused kernels the layer in question is the last one, behind exact pass-through layers);
(e) containment: one NaN / one +Inf at a single (cloud, channel, position) changes no bit of any output that does not depend on it.
"""
import zlib

import numpy as np
import pytest
import torch

from oracle import ops as O
from tests import x6_judge as J

pytestmark = pytest.mark.gpu
U = J.U

# Family (b), worst |got - w x| / (U |w x|) per kernel on the first run of this file on an MI355X (gfx950), bound 8 + 2 p: dense 2.71,
# SA (p = 1) 2.37, chain3 (p = 2) 2.38, coord_tail logits (p = 3) 2.30, cloud bias (exact fp32) 1.00.  On the CPU the worst of the 720
# fp32 orders of the six products alone is 3.57 U, the float64 model 0.67 U (tests/test_x6_judge_cpu.py).  Family (d), worst error
# as a fraction of its bound: dense 0.12 (0.48 U of sum |w||x|, the exact chain 0.39 U), cloud bias 0.04, chain3 0.30 (1.60 U, the chain
# 2.38 U), coord_tail 0.32, SA 0.34.  Every test prints its figure before it asserts.


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _rng(*parts):
    return np.random.default_rng(zlib.crc32(repr(parts).encode()))


# ---- the entry points: numpy in, numpy out ----------------------------------------------------------------------------------------
def run_dense(device, x, w, b, ab=None, act=0, stats=False):
    from captra_amd import fused
    lin = fused.pack(_dev(_f32(w), device), _dev(_f32(b), device))
    with fused.use_mlp_dtype("f32x6"):
        assert fused.dense_x6_supported(x.shape[1], w.shape[1], x.shape[2])
        res = fused.pointwise_mlp_gn(_dev(_f32(x), device), lin, None if ab is None else _dev(_f32(ab), device), act, want_stats=stats)
    return (res[0].cpu().numpy(), res[1].cpu().numpy()) if stats else (res.cpu().numpy(), None)


def _pack_layers(device, layers):
    from captra_amd import fused
    return [fused.pack(_dev(_f32(w), device), _dev(_f32(b), device)) for w, b in layers]


def run_chain3(device, x, layers, act3):
    from captra_amd import fused
    with fused.use_mlp_dtype("f32x6"):
        assert fused.chain_x6_supported(x.shape[1], [128] * 3, x.shape[0] * x.shape[2])
        return fused.mlp_chain3(_dev(_f32(x), device), _pack_layers(device, layers), act3).cpu().numpy()


def run_tail(device, x, layers):
    from captra_amd import fused
    packed = _pack_layers(device, layers)
    xd = _dev(_f32(x), device)
    with fused.use_mlp_dtype("f32x6"):
        assert fused.coord_tail_supported(xd, packed) and fused.chain_x6_supported(x.shape[1], [128] * 3, x.shape[0] * x.shape[2])
        seg, nocs = fused.coord_tail(xd, packed)
    return seg.cpu().numpy(), nocs.cpu().numpy()


def run_cb(device, x, v, w, b, act):
    from captra_amd import fused
    lin = fused.pack(_dev(_f32(w), device), _dev(_f32(b), device))
    with fused.use_mlp_dtype("f32x6"):
        got = fused.pointwise_mlp_cloud_bias(_dev(_f32(x), device), _dev(_f32(v), device), lin, act)
    assert got is not None
    return got.cpu().numpy()


def run_sa(device, feat, xyz_cn, new_xyz, idx, layers):
    """-> (B,c3,M); the output tensor has four channels in front and five behind, which must stay untouched."""
    from captra_amd import fused
    packed = _pack_layers(device, layers)
    cfeat = 0 if feat is None else feat.shape[1]
    c3 = layers[2][0].shape[1]
    B, M, K = idx.shape
    with fused.use_mlp_dtype("f32x6"):
        assert fused.sa_scale_x6_supported(cfeat, packed, K)
        out = torch.full((B, c3 + 9, M), -1.0, device=device)
        fused.sa_scale_x6(None if feat is None else _dev(_f32(feat), device), _dev(_f32(xyz_cn), device), _dev(_f32(new_xyz), device),
                          _dev(idx.astype(np.int32), device), packed, out, 4)
    got = out.cpu().numpy()
    assert (got[:, :4] == -1).all() and (got[:, 4 + c3:] == -1).all()
    return got[:, 4:4 + c3]


# ---- shapes (the smallest that reach every code path) ---------------------------------------------------------------------------------
DENSE = [(16, 256, 128, 1), (48, 256, 256, 2), (176, 512, 256, 1), (512, 512, 512, 1), (1024, 256, 1024, 1)]     # (cin, cout, L, B)
CHAINS = [(131, 4, 4096), (134, 3, 5477)]                    # (c0, B, l): 16384 positions the router requires; 5477: ragged slices
TAILS = [(134, 2, 3, 4, 4096), (134, 4, 12, 3, 5477)]        # (c0, seg, nocs, B, l)
CLOUD_BIAS = [(3, 64, 96, 128, 200), (1, 32, 40, 384, 1)]    # (B, c, c2, cout, l)
# (cfeat, (c1, c2, c3), K, B, N, M): all eight instantiated shapes with the K the backbone uses; M = 37 does not fill a workgroup's waves
SA = [(0, (32, 32, 64), 32, 2, 300, 37), (3, (32, 32, 64), 32, 1, 512, 128), (0, (64, 64, 128), 64, 1, 512, 128),
      (3, (64, 64, 128), 64, 2, 300, 37), (0, (64, 96, 128), 128, 2, 256, 37), (3, (64, 96, 128), 128, 1, 512, 128),
      (320, (128, 128, 256), 64, 2, 333, 37), (320, (128, 128, 256), 32, 1, 512, 128), (320, (128, 196, 256), 128, 1, 512, 128),
      (320, (128, 196, 256), 128, 1, 200, 1)]
PERIOD = 1021            # chains: the 16384 positions repeat a base of 1021 (prime: no alignment with the 32-position slices)


def _tile(base, B, l):
    """base (c, P) -> x (B, c, l) with cloud b reading the base from offset 37 b on, and pos (B, l), the base position of every
    position: a reference computed on the base alone is expanded with `_expand`."""
    pos = (np.arange(l)[None, :] + 37 * np.arange(B)[:, None]) % base.shape[-1]
    return _expand(base, pos), pos


def _expand(base, pos):
    return np.ascontiguousarray(np.moveaxis(base[:, pos], 0, 1))


# ==== (a) integer lattices ===========================================================================================================
@pytest.mark.parametrize("family", "ABC")
@pytest.mark.parametrize("cin,cout,L,B", DENSE)
def test_dense_lattice_bits(device, cin, cout, L, B, family):
    """captra_pointwise_mlp_x6 == int64, bit for bit: plain input and relu(fmaf(a, x, b)) input (a = 2^-s on 2^s x, b a small
    integer: exact), ReLU off and on."""
    rng = _rng("dense-lattice", cin, cout, L, family)
    (lay,), make_x = J.lattice(family, (cin, cout), 0, rng)
    x = make_x((B,), L)
    for gn_in in (False, True):
        if gn_in:
            s = rng.integers(0, 3, (B, cin))
            bb = rng.integers(-3, 4, (B, cin)) * (rng.random((B, cin)) < 0.5)
            if family == "C":
                bb = -np.abs(bb)                               # (|x + b| <= 7 keeps the one-piece side inside the lattice's bound)
            ab = np.stack([np.exp2(-s), bb], axis=-1)
            xin, xeff = x * (1 << s)[:, :, None], np.maximum(x + bb[:, :, None], 0)
        else:
            ab, xin, xeff = None, x, x
        for relu in (False, True):
            ref = J.lattice_forward([lay], xeff, [relu])[0]
            got, _ = run_dense(device, xin, lay.w, lay.b, ab, 1 if relu else 0)
            np.testing.assert_array_equal(got, ref.astype(np.float32), err_msg=f"gn_in={gn_in} relu={relu}")


@pytest.mark.parametrize("family", "AB")
@pytest.mark.parametrize("cin,cout,L,B", DENSE)
def test_dense_lattice_stats_bits(device, cin, cout, L, B, family):
    """Statistics: the outputs are integers <= 256, so the sum and the sum of squares over 128 positions are integers <= 2^23 and
    every order of adding them gives the same bits."""
    rng = _rng("dense-stats", cin, cout, L, family)
    (lay,), make_x = J.lattice(family, (cin, cout), 0, rng, out_max=256)
    x = make_x((B,), L)
    for gn_in in (False, True):
        ab = np.stack([np.ones((B, cin)), np.zeros((B, cin))], axis=-1) if gn_in else None
        ref = J.lattice_forward([lay], np.maximum(x, 0) if gn_in else x, [False])[0]
        assert np.abs(ref).max() <= 256
        got, st = run_dense(device, x, lay.w, lay.b, ab, 0, stats=True)
        np.testing.assert_array_equal(got, ref.astype(np.float32))
        t = ref.reshape(B, cout, L // 128, 128)
        assert (t * t).sum(-1).max() < J.LIMIT
        np.testing.assert_array_equal(st[..., 0], t.sum(-1).astype(np.float32))
        np.testing.assert_array_equal(st[..., 1], (t * t).sum(-1).astype(np.float32))


@pytest.mark.parametrize("family", "ABC")
@pytest.mark.parametrize("c0,B,l", CHAINS)
def test_chain3_lattice_bits(device, c0, B, l, family):
    """captra_mlp_chain3_x6 == int64 with the family's weights in each of the three layers in turn (selections elsewhere: the
    in-register ReLU + split hand-over carries integers of up to 24 bits), last activation off and on."""
    rng = _rng("chain-lattice", c0, l, family)
    for target in range(3):
        layers, make_x = J.lattice(family, (c0, 128, 128, 128), target, rng)
        base = make_x((), PERIOD)
        x, pos = _tile(base, B, l)
        for act3 in (0, 1):
            ref = J.lattice_forward(layers, base, [True, True, bool(act3)])[-1]
            got = run_chain3(device, x, [(lay.w, lay.b) for lay in layers], act3)
            np.testing.assert_array_equal(got, _expand(ref, pos).astype(np.float32), err_msg=f"target={target} act3={act3}")


@pytest.mark.parametrize("family", "ABC")
@pytest.mark.parametrize("c0,seg_dim,nocs_dim,B,l", TAILS)
def test_coord_tail_lattice_bits(device, c0, seg_dim, nocs_dim, B, l, family):
    """captra_coord_tail_x6: the segmentation logits == int64 with the family's weights in layers 1, 2, 3 and in the segmentation head
    in turn; the NOCS head (random weights on the integer feat, behind the sigmoid) within the 1e-6 of tests/test_x6_gpu.py."""
    rng = _rng("tail-lattice", c0, seg_dim, l, family)
    for target in range(4):
        layers, make_x = J.lattice(family, (c0, 128, 128, 128, seg_dim), target, rng)
        base = make_x((), PERIOD)
        x, pos = _tile(base, B, l)
        outs = J.lattice_forward(layers, base, [True, True, True, False])
        # the NOCS head on unit-scale numbers, as in tests/test_x6_gpu.py: its first layer takes feat down by a power of two
        down = 2.0 ** -np.ceil(np.log2(np.sqrt((outs[2].astype(np.float64) ** 2).mean()) + 1))
        nocs_layers = [((rng.standard_normal((128, 128)) / np.sqrt(128) * down).astype(np.float32), rng.standard_normal(128).astype(np.float32)),
                       ((rng.standard_normal((128, nocs_dim)) / np.sqrt(128)).astype(np.float32), rng.standard_normal(nocs_dim).astype(np.float32))]
        seg, nocs = run_tail(device, x, [(lay.w, lay.b) for lay in layers] + nocs_layers)
        np.testing.assert_array_equal(seg, _expand(outs[3], pos).astype(np.float32), err_msg=f"target={target}")
        if target == 3:
            feat = outs[2].astype(np.float32)[None]
            raw = O.pointwise_mlp(O.pointwise_mlp(feat, *nocs_layers[0], 1), *nocs_layers[1], 0)[0]
            np.testing.assert_allclose(nocs, _expand(1.0 / (1.0 + np.exp(-raw.astype(np.float64))) - 0.5, pos), atol=1e-6, rtol=0)


@pytest.mark.parametrize("family", "ABC")
@pytest.mark.parametrize("B,c,c2,cout,l", CLOUD_BIAS)
def test_cloud_bias_lattice_bits(device, B, c, c2, cout, l, family):
    """act(W1 x + (W2 v + b)) is exact fp32 arithmetic: all three lattices bit for bit, ReLU off and on."""
    rng = _rng("cb-lattice", B, c, cout, l, family)
    (lay,), make_x = J.lattice(family, (c + c2, cout), 0, rng)
    xc = make_x((B,), l)
    xc[:, c:, :] = xc[:, c:, :1]                              # one vector per cloud
    for relu in (False, True):
        ref = J.lattice_forward([lay], xc, [relu])[0]
        got = run_cb(device, xc[:, :c], xc[:, c:, :1], lay.w, lay.b, 1 if relu else 0)
        np.testing.assert_array_equal(got, ref.astype(np.float32), err_msg=f"relu={relu}")


def _sa_lattice_case(rng, family, cfeat, chans, target, B, N, M, K):
    """Integer points, centres and neighbour lists for one SA scale, the lattice's layers and the grouped input (B,cfeat+3,M*K)."""
    layers, make_x = J.lattice(family, (cfeat + 3,) + chans, target, rng)
    pts = make_x((B,), N)                                     # (B, cfeat + 3, N): feature rows, then xyz
    if family == "C":
        pts[:, cfeat:] = np.clip(pts[:, cfeat:], -6, 6)       # |xyz - centre| <= 7: one piece, inside the lattice's bound
    new_xyz = rng.integers(-1, 2, (B, M, 3))
    idx = rng.integers(0, N, (B, M, K))
    g = np.stack([pts[b][:, idx[b]] for b in range(B)])       # (B, cfeat + 3, M, K)
    g[:, cfeat:] -= np.moveaxis(new_xyz, 2, 1)[:, :, :, None]
    return layers, pts, new_xyz, idx, g.reshape(B, cfeat + 3, M * K)


@pytest.mark.parametrize("family", "ABC")
@pytest.mark.parametrize("cfeat,chans,K,B,N,M", SA)
def test_sa_lattice_bits(device, cfeat, chans, K, B, N, M, family):
    """captra_sa_scale_x6 == int64: integer coordinates, centres and features, the first layer (exact fp32, or the point-major
    pre-transform) a selection, the family's weights in layer 2 and in layer 3 in turn; the max over the neighbours is a max of
    integers."""
    rng = _rng("sa-lattice", cfeat, chans, K, M, family)
    for target in (1, 2):
        layers, pts, new_xyz, idx, g = _sa_lattice_case(rng, family, cfeat, chans, target, B, N, M, K)
        ref = J.lattice_forward(layers, g, [True, True, True])[-1].reshape(B, chans[2], M, K).max(-1)
        got = run_sa(device, pts[:, :cfeat] if cfeat else None, pts[:, cfeat:], new_xyz, idx, [(lay.w, lay.b) for lay in layers])
        np.testing.assert_array_equal(got, ref.astype(np.float32), err_msg=f"target={target}")


# ==== (b) one product at a time ======================================================================================================
def _check_probe(kernel, got, expect, p, zero_exact=True):
    """|got - expect| <= (8 + 2 p) U |expect| per element (expect float64); where expect is 0 the output is 0."""
    got = got.astype(np.float64)
    nz = expect != 0
    assert nz.any()
    ratio = (np.abs(got - expect)[nz] / np.abs(expect[nz])).max() / U
    print(f"x6 probe ratio {kernel}: {ratio:.3f} U (bound {J.PROBE_TOL + 2 * p})")
    if zero_exact:
        assert (got[~nz] == 0).all()
    assert ratio <= J.PROBE_TOL + 2 * p, (kernel, ratio)


def _one_hot(vals, cin):
    """vals (B, L) -> x (B, cin, L) with position p holding vals[:, p] in channel p mod cin, zeros elsewhere."""
    B, L = vals.shape
    x = np.zeros((B, cin, L), np.float32)
    x[:, np.arange(L) % cin, np.arange(L)] = vals
    return x


@pytest.mark.parametrize("cin,cout,L,B", DENSE)
def test_dense_one_product_at_a_time(device, cin, cout, L, B):
    """captra_pointwise_mlp_x6, every (k, c) of the layer as a single six-product sum: plain input, and relu(fmaf(a, x, 0)) input with
    a a power of two; zero input gives act(bias) bit for bit."""
    rng = _rng("dense-probe", cin, cout, L)
    w = J.probe_values(rng, (cin, cout))
    k = np.arange(L) % cin
    zero_b = np.zeros(cout, np.float32)
    for gn_in in (False, True):
        vals = J.probe_values(rng, (B, L), signed=not gn_in)
        x = _one_hot(vals, cin)
        ab, xin = None, x
        if gn_in:
            s = rng.integers(-3, 4, (B, cin))
            ab = np.stack([np.exp2(s), np.zeros((B, cin))], axis=-1)
            xin = x * np.exp2(-s)[:, :, None].astype(np.float32)
        expect = w.astype(np.float64).T[None, :, k] * vals.astype(np.float64)[:, None, :]
        got, _ = run_dense(device, xin, w, zero_b, ab, 0)
        _check_probe("dense", got, expect, 0)
        got, _ = run_dense(device, xin, w, zero_b, ab, 1)
        _check_probe("dense", got, np.maximum(expect, 0), 0)
    b = rng.standard_normal(cout).astype(np.float32)
    for actv in (0, 1):
        got, _ = run_dense(device, np.zeros((B, cin, L), np.float32), w, b, None, actv)
        np.testing.assert_array_equal(got, np.broadcast_to((np.maximum(b, 0) if actv else b)[None, :, None], got.shape))


def _perm_chain(rng, dims, target, last_signed):
    """Layers of a fused chain of widths `dims` with probe weights at `target` and positive power-of-two permutations elsewhere (the
    last layer signed when it has no ReLU): returns (weights, srcs) with srcs[i][c] = the input channel output c of layer i copies."""
    ws, srcs = [], []
    for i in range(len(dims) - 1):
        if i == target:
            ws.append(J.probe_values(rng, (dims[i], dims[i + 1])))
            srcs.append(None)
        else:
            w, src = J.pow2_perm(rng, dims[i], dims[i + 1], negate=(last_signed and i == len(dims) - 2))
            ws.append(w)
            srcs.append(src)
    return ws, srcs


def _probe_chain_expect(ws, srcs, target, relu, x):
    """float64 expectation of a chain with one-hot inputs: exact permutation layers, the probe layer's single product."""
    h = x.astype(np.float64)                                   # (B, c, L)
    for i, w in enumerate(ws):
        h = np.einsum("kc,bkl->bcl", w.astype(np.float64), h)  # one non-zero term per output: exact in float64 up to the probe product
        if relu[i]:
            h = np.maximum(h, 0)
    return h


def _chain_probe_input(rng, ws, srcs, target, c0, L):
    """One-hot input (1, c0, L): position p feeds channel p mod cin_target of the probe layer, through the permutations in front
    (positive weights: the value arrives positive); for target 0 the input is the signed probe itself."""
    if target == 0:
        return _one_hot(J.probe_values(rng, (1, L)), c0)
    vals = J.probe_values(rng, (1, L), signed=False)
    cin_t = ws[target].shape[0]
    ch = np.arange(L) % cin_t                                   # channel of the target layer's input
    ok = np.ones(L, bool)
    for i in range(target - 1, -1, -1):                         # back through the permutations
        nxt = srcs[i][ch]
        ok &= nxt >= 0
        ch = np.where(nxt >= 0, nxt, 0)
    x = np.zeros((1, c0, L), np.float32)
    p = np.nonzero(ok)[0]
    x[0, ch[p], p] = vals[0, p]
    return x


@pytest.mark.parametrize("c0,B,l", CHAINS)
def test_chain3_one_product_at_a_time(device, c0, B, l):
    """captra_mlp_chain3_x6: each layer in turn holds probe weights, the other two are positive power-of-two permutations (p = 2), with
    W and with -W so that every (k, c) is seen once on the positive side of the ReLU; zero input with zero inner biases gives
    act3(b3) bit for bit."""
    rng = _rng("chain-probe", c0, l)
    dims = (c0, 128, 128, 128)
    zb = [np.zeros(128, np.float32)] * 3
    for target in range(3):
        for act3 in ((0, 1) if target == 2 else (1,)):
            ws, srcs = _perm_chain(rng, dims, target, last_signed=(act3 == 0))
            base = _chain_probe_input(rng, ws, srcs, target, c0, PERIOD)[0]
            x, pos = _tile(base, B, l)
            for sign in (1.0, -1.0):
                wl = [w * np.float32(sign) if i == target else w for i, w in enumerate(ws)]
                expect = _probe_chain_expect(wl, srcs, target, [True, True, bool(act3)], base[None])[0]
                got = run_chain3(device, x, list(zip(wl, zb)), act3)
                _check_probe("chain3", got, _expand(expect, pos), 2)
    b3 = rng.standard_normal(128).astype(np.float32)
    ws = [J.probe_values(rng, (dims[i], dims[i + 1])) for i in range(3)]
    for act3 in (0, 1):
        got = run_chain3(device, np.zeros((B, c0, l), np.float32), list(zip(ws, [zb[0], zb[0], b3])), act3)
        np.testing.assert_array_equal(got, np.broadcast_to((np.maximum(b3, 0) if act3 else b3)[None, :, None], got.shape))


@pytest.mark.parametrize("c0,seg_dim,nocs_dim,B,l", TAILS)
def test_coord_tail_one_product_at_a_time(device, c0, seg_dim, nocs_dim, B, l):
    """captra_coord_tail_x6, the segmentation branch: probe weights in the head itself (p = 3: every (k, c) of the head) and in layers
    1 / 2 / 3 -- those seen through the head's seg_dim permutation outputs only, i.e. 2 or 4 of each probed layer's 128 output
    columns (all of its input channels), not every (k, c): the full sweep of the inner layers is test_chain3_one_product_at_a_time's,
    on the three-layer instantiation of the same kernel template.  The NOCS branch sits behind the sigmoid and is held by the
    lattices and tests/test_x6_gpu.py."""
    rng = _rng("tail-probe", c0, seg_dim, l)
    dims = (c0, 128, 128, 128, seg_dim)
    zb = [np.zeros(128, np.float32)] * 3 + [np.zeros(seg_dim, np.float32)]
    nocs_layers = [((rng.standard_normal((128, 128)) / np.sqrt(128)).astype(np.float32), np.zeros(128, np.float32)),
                   ((rng.standard_normal((128, nocs_dim)) / np.sqrt(128)).astype(np.float32), rng.standard_normal(nocs_dim).astype(np.float32))]
    for target in (3, 0, 1, 2):
        ws, srcs = _perm_chain(rng, dims, target, last_signed=True)
        base = _chain_probe_input(rng, ws, srcs, target, c0, PERIOD)[0]
        x, pos = _tile(base, B, l)
        for sign in (1.0, -1.0):
            wl = [w * np.float32(sign) if i == target else w for i, w in enumerate(ws)]
            expect = _probe_chain_expect(wl, srcs, target, [True, True, True, False], base[None])[0]
            seg, _ = run_tail(device, x, list(zip(wl, zb)) + nocs_layers)
            _check_probe("coord_tail", seg, _expand(expect, pos), 3)
    bs = rng.standard_normal(seg_dim).astype(np.float32)
    ws = [J.probe_values(rng, (dims[i], dims[i + 1])) for i in range(4)]
    seg, nocs = run_tail(device, np.zeros((B, c0, l), np.float32), list(zip(ws, zb[:3] + [bs])) + nocs_layers)
    np.testing.assert_array_equal(seg, np.broadcast_to(bs[None, :, None], seg.shape))
    raw = nocs_layers[1][1].astype(np.float64)
    np.testing.assert_allclose(nocs, np.broadcast_to((1.0 / (1.0 + np.exp(-raw)) - 0.5)[None, :, None], nocs.shape), atol=1e-6, rtol=0)


@pytest.mark.parametrize("B,c,c2,cout,l", CLOUD_BIAS)
def test_cloud_bias_one_product_at_a_time(device, B, c, c2, cout, l):
    """act(W1 x + (W2 v + 0)) with v = 0: every position one exact fp32 product (<= 1 U, held to the family's 8); and with x = 0, one
    non-zero channel of v per cloud."""
    rng = _rng("cb-probe", B, c, cout, l)
    w = J.probe_values(rng, (c + c2, cout))
    zero_b = np.zeros(cout, np.float32)
    vals = J.probe_values(rng, (B, l))
    x = _one_hot(vals, c)
    expect = w.astype(np.float64).T[None, :, np.arange(l) % c] * vals.astype(np.float64)[:, None, :]
    got = run_cb(device, x, np.zeros((B, c2, 1), np.float32), w, zero_b, 0)
    _check_probe("cloud_bias", got, expect, 0)
    got = run_cb(device, x, np.zeros((B, c2, 1), np.float32), w, zero_b, 1)
    _check_probe("cloud_bias", got, np.maximum(expect, 0), 0)
    for kv in rng.permutation(c2)[:4]:
        vv = J.probe_values(rng, (B,))
        v = np.zeros((B, c2, 1), np.float32)
        v[:, kv, 0] = vv
        expect = np.broadcast_to((w[c + kv].astype(np.float64)[None, :] * vv.astype(np.float64)[:, None])[:, :, None], (B, cout, l))
        got = run_cb(device, np.zeros((B, c, l), np.float32), v, w, zero_b, 0)
        _check_probe("cloud_bias", got, expect, 0)
    b = rng.standard_normal(cout).astype(np.float32)
    got = run_cb(device, np.zeros((B, c, l), np.float32), np.zeros((B, c2, 1), np.float32), w, b, 1)
    np.testing.assert_array_equal(got, np.broadcast_to(np.maximum(b, 0)[None, :, None], got.shape))


def _fib_sphere(n):
    i = np.arange(n) + 0.5
    phi = np.arccos(1 - 2 * i / n)
    th = np.pi * (1 + 5 ** 0.5) * i
    return np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], axis=1)


def _sa_probe_case(rng, cfeat, c1, K, B, N, M):
    """One probe point per centre whose first-layer output h1 is one-hot (channel j = (b M + m) mod c1), in a slot that varies across
    the centres (all K / 32 slices), the other K - 1 slots holding a point whose h1 is zero.  Returns feat, xyz_cn, new_xyz, idx, the
    first layer (w1, b1) and hv (B, M), jv (B, M): the value and channel of the centre's one-hot h1 as the ORACLE's exact chain
    computes it."""
    assert N >= 2 * M
    jv = (np.arange(B)[:, None] * M + np.arange(M)[None, :]) % c1
    slot = (np.arange(M) * 37 + 5) % K
    idx = np.tile(np.arange(M)[None, :, None], (B, 1, K))                   # point m: the zero point of centre m
    idx[:, np.arange(M), slot] = M + np.arange(M)                           # point M + m: its probe point
    new_xyz = rng.uniform(-0.5, 0.5, (B, M, 3)).astype(np.float32)
    xyz = np.zeros((B, N, 3), np.float32)
    xyz[:, :M] = new_xyz
    if cfeat == 320:
        # layer 1 through the exact point-major pre-transform: a 0 / 1 selection of feature rows, xyz rows and b1 zero
        rows = rng.permutation(cfeat)[:c1]
        w1 = np.zeros((cfeat + 3, c1), np.float32)
        w1[rows, np.arange(c1)] = 1.0
        b1 = np.zeros(c1, np.float32)
        feat = np.zeros((B, cfeat, N), np.float32)
        hv = J.probe_values(rng, (B, M), signed=False)
        feat[np.arange(B)[:, None], rows[jv], M + np.arange(M)[None, :]] = hv
        xyz[:, M:2 * M] = new_xyz + rng.uniform(-0.1, 0.1, (B, M, 3)).astype(np.float32)
        return feat, np.ascontiguousarray(xyz.transpose(0, 2, 1)), new_xyz, idx, (w1, b1), hv, jv
    # layer 1 is the exact fp32 MFMA on the 3 .. 6 inputs: h1[j] = relu(u_j . (p - centre) - t), u_j the c1 directions of a Fibonacci sphere
    # (nearest neighbours >= 20 degrees apart for c1 <= 64), the probe point of channel j at distance s along u_j: only channel j is above t.
    u = _fib_sphere(c1)
    gram = u @ u.T - 2 * np.eye(c1)
    t = np.float32(0.5 * (1 + gram.max()))
    w1 = np.zeros((cfeat + 3, c1), np.float32)
    w1[cfeat:] = u.T
    b1 = np.full(c1, -t, np.float32)
    feat = None
    if cfeat:
        # the feature rows carry the threshold instead of the bias: feature 0 is the constant one, the others are noise under zero weights
        feat = rng.standard_normal((B, cfeat, N)).astype(np.float32)
        feat[:, 0] = 1.0
        w1[0], b1[:] = -t, 0.0
    zero_ok = False
    xyz_cn = None
    todo = np.ones((B, M), bool)
    hv = np.zeros((B, M), np.float32)
    for _ in range(200):                                                    # rejection-sample the scale per point
        s = rng.uniform(1.0, 1.02, (B, M)).astype(np.float32)
        cand = new_xyz + (s[..., None] * u[jv]).astype(np.float32)
        xyz[:, M:2 * M][todo] = cand[todo]
        xyz_cn = np.ascontiguousarray(xyz.transpose(0, 2, 1))
        h1 = O.pointwise_mlp(O.sa_group(feat, xyz_cn, new_xyz, idx.astype(np.int32)), w1, b1, 1)       # (B, c1, M, K)
        hp = h1[:, :, np.arange(M), slot]                                   # the probe slots (B, c1, M)
        hv = np.take_along_axis(hp, jv[:, None, :], 1)[:, 0]
        todo = ~J.is_probe(hv)
        zero_ok = True
        if not todo.any():
            break
    assert zero_ok and not todo.any()
    onehot = np.zeros_like(h1)
    onehot[np.arange(B)[:, None], jv, np.arange(M)[None, :], slot[None, :]] = hv
    np.testing.assert_array_equal(h1, onehot)                               # one-hot, and zero in every other slot
    return feat, xyz_cn, new_xyz, idx, (w1, b1), hv, jv


@pytest.mark.parametrize("cfeat,chans,K,B,N,M", [c for c in SA if c[5] > 1])
def test_sa_one_product_at_a_time(device, cfeat, chans, K, B, N, M):
    """captra_sa_scale_x6: every centre has ONE neighbour whose first-layer output is one-hot with a probe value (the exact first
    layer, checked with the oracle on the CPU), all others zero.  Probe weights in layer 2 (layer 3 a positive permutation) and in
    layer 3 (layer 2 a permutation -- two complementary ones where c2 > c1), with W and -W: p = 1.  All-zero first-layer
    weights and zero inner biases give relu(b3) bit for bit."""
    c1, c2, c3 = chans
    rng = _rng("sa-probe", cfeat, chans, K, M)
    feat, xyz_cn, new_xyz, idx, l1, hv, jv = _sa_probe_case(rng, cfeat, c1, K, B, N, M)
    h1 = np.zeros((B, c1, M))
    h1[np.arange(B)[:, None], jv, np.arange(M)[None, :]] = hv.astype(np.float64)
    cases = []
    w3p, _ = J.pow2_perm(rng, c2, c3, negate=False)
    cases.append((J.probe_values(rng, (c1, c2)), w3p, 1))
    w2p, src = J.pow2_perm(rng, c1, c2, negate=False)
    cases.append((w2p, J.probe_values(rng, (c2, c3)), 2))
    if c2 > c1:                                                             # the channels of layer 3's input the first permutation left out
        free = np.nonzero(src < 0)[0]
        w2q = np.zeros((c1, c2), np.float32)
        w2q[np.arange(len(free)), free] = 1.0                               # (c2 - c1 <= c1: one non-zero per row here too)
        cases.append((w2q, J.probe_values(rng, (c2, c3)), 2))
    for w2, w3, target in cases:
        for sign in (1.0, -1.0):
            w2s, w3s = (w2 * np.float32(sign), w3) if target == 1 else (w2, w3 * np.float32(sign))
            h2 = np.maximum(np.einsum("kc,bkm->bcm", w2s.astype(np.float64), h1), 0)
            expect = np.maximum(np.einsum("kc,bkm->bcm", w3s.astype(np.float64), h2), 0)
            got = run_sa(device, feat, xyz_cn, new_xyz, idx, [l1, (w2s, np.zeros(c2, np.float32)), (w3s, np.zeros(c3, np.float32))])
            _check_probe("sa", got, expect, 1)
    # zero input to layer 2: no first-layer weights, no inner biases -> relu(b3) for every centre, bit for bit
    b3 = rng.standard_normal(c3).astype(np.float32)
    got = run_sa(device, feat, xyz_cn, new_xyz, idx, [(np.zeros_like(l1[0]), np.zeros(c1, np.float32)),
                                                      (J.probe_values(rng, (c1, c2)), np.zeros(c2, np.float32)), (J.probe_values(rng, (c2, c3)), b3)])
    np.testing.assert_array_equal(got, np.broadcast_to(np.maximum(b3, 0)[None, :, None], got.shape))


# ==== (c) power-of-two rescaling =====================================================================================================
def _floor(v, lim=2.0 ** -10):
    """N(0,1)-type data without its tiniest values, so that every piece stays a normal number after 2^-80."""
    v = np.asarray(v, np.float32).copy()
    v[np.abs(v) < lim] = 0
    return v


def _scales(rng, n):
    return rng.integers(-40, 41, n)


def _assert_range(*arrays):
    lo, hi = J.piece_range(*arrays)
    assert lo >= 2.0 ** -120 and hi <= 2.0 ** 100, (lo, hi)


def _scaled(y, g, axis=1):
    shape = [1] * y.ndim
    shape[axis] = -1
    out = y.astype(np.float64) * np.exp2(g).reshape(shape)
    assert np.abs(out).max() <= 2.0 ** 100 and (np.abs(out[out != 0]).min() >= 2.0 ** -120)
    return out.astype(np.float32)


@pytest.mark.parametrize("cin,cout,L,B", DENSE)
def test_dense_rescaling_bits(device, cin, cout, L, B):
    """captra_pointwise_mlp_x6 on N(0,1) data, as is and with 2^a_k on the input channels / 2^-a_k on the weight rows / 2^g_c on the
    output channels: all products and all sums scale exactly, so 2^g_c times the first run == the second, bit for bit -- output and
    statistics, plain and GroupNorm-coefficient input (the coefficients' b scales with its channel)."""
    rng = _rng("dense-rescale", cin, cout, L)
    x = _floor(rng.standard_normal((B, cin, L)))
    w = _floor(rng.standard_normal((cin, cout)) / np.sqrt(cin))
    b = _floor(rng.standard_normal(cout))
    a, g = _scales(rng, cin), _scales(rng, cout)
    w2, x2 = J.rescale_in(w, x, a)
    w2, b2 = J.rescale_out(w2, b, g)
    _assert_range(x, w, b, x2, w2, b2)
    for gn_in in (False, True):
        ab = ab2 = None
        if gn_in:
            ab = np.stack([np.exp2(rng.integers(-1, 2, (B, cin))), _floor(rng.standard_normal((B, cin)) * 0.3)], axis=-1).astype(np.float32)
            ab2 = ab.copy()
            ab2[..., 1] = (ab[..., 1].astype(np.float64) * np.exp2(a)[None, :]).astype(np.float32)
        y1, s1 = run_dense(device, x, w, b, ab, 0, stats=True)
        y2, s2 = run_dense(device, x2, w2, b2, ab2, 0, stats=True)
        np.testing.assert_array_equal(y2, _scaled(y1, g))
        np.testing.assert_array_equal(s2[..., 0], _scaled(s1[..., 0], g))
        np.testing.assert_array_equal(s2[..., 1], _scaled(s1[..., 1], 2 * g))
        r2, _ = run_dense(device, x2, w2, b2, ab2, 1)
        np.testing.assert_array_equal(r2, np.maximum(y2, 0))


def _chain_data(rng, dims, B, l):
    x = _floor(rng.standard_normal((B, dims[0], l)))
    layers = [(_floor(rng.standard_normal((dims[i], dims[i + 1])) / np.sqrt(dims[i])), _floor(rng.standard_normal(dims[i + 1])))
              for i in range(len(dims) - 1)]
    return x, layers


@pytest.mark.parametrize("c0,B,l", CHAINS)
def test_chain3_rescaling_bits(device, c0, B, l):
    """captra_mlp_chain3_x6: the first layer's input channels and the last layer's output channels rescaled (scales on inner layers
    pass through ReLU unchanged and are not a separate case)."""
    rng = _rng("chain-rescale", c0, l)
    x, layers = _chain_data(rng, (c0, 128, 128, 128), B, l)
    a, g = _scales(rng, c0), _scales(rng, 128)
    w0, x2 = J.rescale_in(layers[0][0], x, a)
    w3, b3 = J.rescale_out(layers[2][0], layers[2][1], g)
    layers2 = [(w0, layers[0][1]), layers[1], (w3, b3)]
    _assert_range(x, x2, *[t for lay in layers + layers2 for t in lay])
    for act3 in (0, 1):
        y1 = run_chain3(device, x, layers, act3)
        y2 = run_chain3(device, x2, layers2, act3)
        np.testing.assert_array_equal(y2, _scaled(y1, g))


@pytest.mark.parametrize("c0,seg_dim,nocs_dim,B,l", TAILS)
def test_coord_tail_rescaling_bits(device, c0, seg_dim, nocs_dim, B, l):
    """captra_coord_tail_x6: input channels and the segmentation head's outputs rescaled; the NOCS branch sees the input scaling only
    and repeats its bits."""
    rng = _rng("tail-rescale", c0, seg_dim, l)
    x, layers = _chain_data(rng, (c0, 128, 128, 128), B, l)
    layers += [(_floor(rng.standard_normal((128, seg_dim)) / np.sqrt(128)), _floor(rng.standard_normal(seg_dim))),
               (_floor(rng.standard_normal((128, 128)) / np.sqrt(128)), _floor(rng.standard_normal(128))),
               (_floor(rng.standard_normal((128, nocs_dim)) / np.sqrt(128)), _floor(rng.standard_normal(nocs_dim)))]
    a, g = _scales(rng, c0), _scales(rng, seg_dim)
    w0, x2 = J.rescale_in(layers[0][0], x, a)
    ws, bs = J.rescale_out(layers[3][0], layers[3][1], g)
    layers2 = [(w0, layers[0][1]), layers[1], layers[2], (ws, bs), layers[4], layers[5]]
    _assert_range(x, x2, *[t for lay in layers + layers2 for t in lay])
    seg1, nocs1 = run_tail(device, x, layers)
    seg2, nocs2 = run_tail(device, x2, layers2)
    np.testing.assert_array_equal(seg2, _scaled(seg1, g))
    np.testing.assert_array_equal(nocs2, nocs1)


@pytest.mark.parametrize("B,c,c2,cout,l", CLOUD_BIAS)
def test_cloud_bias_rescaling_bits(device, B, c, c2, cout, l):
    """act(W1 x + (W2 v + b)): input channels of x and of v, and the output channels, rescaled."""
    rng = _rng("cb-rescale", B, c, cout, l)
    xc = _floor(rng.standard_normal((B, c + c2, l)))
    w = _floor(rng.standard_normal((c + c2, cout)) / np.sqrt(c + c2))
    b = _floor(rng.standard_normal(cout))
    a, g = _scales(rng, c + c2), _scales(rng, cout)
    w2, xc2 = J.rescale_in(w, xc, a)
    w2, b2 = J.rescale_out(w2, b, g)
    _assert_range(xc, w, b, xc2, w2, b2)
    for actv in (0, 1):
        y1 = run_cb(device, xc[:, :c], xc[:, c:, :1], w, b, actv)
        y2 = run_cb(device, xc2[:, :c], xc2[:, c:, :1], w2, b2, actv)
        np.testing.assert_array_equal(y2, _scaled(y1, g))


def _sa_random_case(rng, cfeat, chans, K, B, N, M):
    xyz_cn = _floor(rng.random((B, 3, N), dtype=np.float32) - 0.5)
    feat = _floor(rng.standard_normal((B, cfeat, N))) if cfeat else None
    new_xyz = _floor(rng.random((B, M, 3), dtype=np.float32) - 0.5)
    idx = rng.integers(0, N, (B, M, K)).astype(np.int32)
    dims = (cfeat + 3,) + chans
    layers = [(_floor(rng.standard_normal((dims[i], dims[i + 1])) / np.sqrt(dims[i])), _floor(rng.standard_normal(dims[i + 1]))) for i in range(3)]
    return xyz_cn, feat, new_xyz, idx, layers


@pytest.mark.parametrize("cfeat,chans,K,B,N,M", SA)
def test_sa_rescaling_bits(device, cfeat, chans, K, B, N, M):
    """captra_sa_scale_x6: feature channels and coordinates (points AND centres: the difference scales exactly) by 2^a_k with 2^-a_k
    on the first layer's rows -- its fmaf chain sees the same products -- and 2^g_c on the last layer (bias and ReLU behind the max)."""
    rng = _rng("sa-rescale", cfeat, chans, K, M)
    xyz_cn, feat, new_xyz, idx, layers = _sa_random_case(rng, cfeat, chans, K, B, N, M)
    a, g = _scales(rng, cfeat + 3), _scales(rng, chans[2])
    pts = xyz_cn if feat is None else np.concatenate([feat, xyz_cn], axis=1)
    w1, pts2 = J.rescale_in(layers[0][0], pts, a)
    new2 = (new_xyz.astype(np.float64) * np.exp2(a[cfeat:])[None, None, :]).astype(np.float32)
    w3, b3 = J.rescale_out(layers[2][0], layers[2][1], g)
    layers2 = [(w1, layers[0][1]), layers[1], (w3, b3)]
    _assert_range(pts, pts2, new_xyz, new2, *[t for lay in layers + layers2 for t in lay])
    y1 = run_sa(device, feat, xyz_cn, new_xyz, idx, layers)
    y2 = run_sa(device, None if feat is None else pts2[:, :cfeat], pts2[:, cfeat:], new2, idx, layers2)
    np.testing.assert_array_equal(y2, _scaled(y1, g))


# ==== (d) cancellation and small channels ============================================================================================
def _cancelling(rng, cin, cout, B, L):
    """x, w whose terms cancel in pairs (channels 2 i and 2 i + 1: opposite inputs, nearly equal weights) to |y| <= 1e-3 sum |w||x| at
    every position and output channel; the odd output channels' weights are 2^-14 of the even ones'."""
    x = rng.standard_normal((B, cin, L))
    x[:, 1::2] = -x[:, 0::2] * (1 + 1e-4 * rng.standard_normal((B, cin // 2, L)))
    w = rng.standard_normal((cin, cout)) / np.sqrt(cin)
    w[1::2] = w[0::2] * (1 + 1e-4 * rng.standard_normal((cin // 2, cout)))
    w[:, 1::2] *= 2.0 ** -14
    return x.astype(np.float32), w.astype(np.float32)


def _cancel_report(got, ref, mass, chain):
    """got within 2 x the exact chain's own error + 4 U sum |w x| of the float64 result, per element; the data cancel as promised."""
    assert (np.abs(ref) <= 1e-3 * mass).all() and (mass > 0).all()
    e_got, e_chain = np.abs(got.astype(np.float64) - ref), np.abs(chain.astype(np.float64) - ref)
    bound = 2.0 * e_chain + 4 * U * mass
    worst = (e_got / bound).max()
    print(f"x6 cancellation: worst error / bound = {worst:.3f}; in U of sum|w||x|: got {(e_got / mass).max() / U:.2f}, chain {(e_chain / mass).max() / U:.2f}")
    assert (e_got <= bound).all(), worst


def _check_cancel(got, x, w, b, B):
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    ref = np.einsum("kc,bkl->bcl", w64, x64) + b.astype(np.float64)[None, :, None]
    mass = np.einsum("kc,bkl->bcl", np.abs(w64), np.abs(x64))
    _cancel_report(got, ref, mass, O.pointwise_mlp(x, w, b, 0))


@pytest.mark.parametrize("cin,cout,L,B", DENSE)
def test_dense_cancellation_and_small_channels(device, cin, cout, L, B):
    rng = _rng("dense-cancel", cin, cout, L)
    x, w = _cancelling(rng, cin, cout, B, L)
    b = np.zeros(cout, np.float32)
    got, _ = run_dense(device, x, w, b, None, 0)
    _check_cancel(got, x, w, b, B)


@pytest.mark.parametrize("B,c,c2,cout,l", CLOUD_BIAS)
def test_cloud_bias_cancellation_and_small_channels(device, B, c, c2, cout, l):
    rng = _rng("cb-cancel", B, c, cout, l)
    xc, w = _cancelling(rng, c + c2, cout, B, l)
    xc[:, c:, :] = xc[:, c:, :1]
    # (c is even: the pairs of the per-cloud vector are position 0's pairs and cancel at every position)
    b = np.zeros(cout, np.float32)
    got = run_cb(device, xc[:, :c], xc[:, c:, :1], w, b, 0)
    _check_cancel(got, xc, w, b, B)


# The fused kernels: the cancelling pairs and the 2^-14 columns sit in the LAST layer, whose input is what positive power-of-two
# permutations (and, for SA, the exact first layer) hand on.  Behind a ReLU that input is non-negative, so the pairs cancel through
# the weights: h[q] = h[p] (1 + d), w[q, :] = -w[p, :] (1 + e) for paired channels (p, q).  A permutation layer is exact in these
# kernels as in the exact chain (one piece of w times x0 + x1 + x2, whose partial sums x1 + x2 and x0 + x1 are fp32 numbers), so the
# issue's single-layer bound is asked of the whole kernel unchanged, against the chained O.pointwise_mlp.
def _cancel_pairs(rng, cin, cout, live, tail):
    """h (cin,) + tail >= 0, fp32, non-zero on the channels `live` (an even number, paired in order), and w (cin, cout)."""
    p, q = live[0::2], live[1::2]
    h = np.zeros((cin,) + tuple(tail))
    h[p] = np.abs(rng.standard_normal((len(p),) + tuple(tail))) + 0.1
    h[q] = h[p] * (1 + 1e-4 * rng.standard_normal(h[p].shape))
    w = rng.standard_normal((cin, cout)) / np.sqrt(len(live))
    w[q] = -w[p] * (1 + 1e-4 * rng.standard_normal((len(p), cout)))
    w[:, 1::2] *= 2.0 ** -14
    return h.astype(np.float32), w.astype(np.float32)


def _back_through(ws, srcs, h):
    """The input (c0, L) that the positive permutations ws hand on as h (c_last, L): exact divisions by powers of two."""
    ch, val = np.arange(h.shape[0]), h.astype(np.float64)
    for w, src in zip(ws[::-1], srcs[::-1]):
        assert (src[ch] >= 0).all()
        val, ch = val / w[src[ch], ch].astype(np.float64)[:, None], src[ch]
    x = np.zeros((ws[0].shape[0], h.shape[1]), np.float32)
    x[ch] = val
    return x


def _fused_cancel_case(rng, dims):
    """Layers of widths dims: positive permutations, then the cancelling last layer; the base input (c0, PERIOD) and the references
    on it: float64 result, sum |w||h|, and the exact chain's result."""
    n = len(dims) - 1
    perms = [J.pow2_perm(rng, dims[i], dims[i + 1], negate=False) for i in range(n - 1)]
    ws, srcs = [w for w, _ in perms], [src for _, src in perms]
    h, wl = _cancel_pairs(rng, dims[-2], dims[-1], rng.permutation(dims[-2]), (PERIOD,))
    base = _back_through(ws, srcs, h)
    zb = [np.zeros(d, np.float32) for d in dims[1:]]
    h64, chain = base.astype(np.float64), base[None]
    for w, b in zip(ws, zb):
        h64 = np.maximum(w.astype(np.float64).T @ h64, 0)
        chain = O.pointwise_mlp(chain, w, b, 1)
    np.testing.assert_array_equal(h64, h.astype(np.float64))              # the permutations hand on exactly what was planned
    ref, mass = wl.astype(np.float64).T @ h64, np.abs(wl).astype(np.float64).T @ h64
    chain = O.pointwise_mlp(chain, wl, zb[-1], 0)[0]
    return list(zip(ws + [wl], zb)), base, ref, mass, chain


@pytest.mark.parametrize("c0,B,l", CHAINS)
def test_chain3_cancellation_and_small_channels(device, c0, B, l):
    """captra_mlp_chain3_x6 with the cancelling, small-channel layer as its third (no activation)."""
    rng = _rng("chain-cancel", c0, l)
    layers, base, ref, mass, chain = _fused_cancel_case(rng, (c0, 128, 128, 128))
    x, pos = _tile(base, B, l)
    got = run_chain3(device, x, layers, 0)
    _cancel_report(got, _expand(ref, pos), _expand(mass, pos), _expand(chain, pos))


@pytest.mark.parametrize("c0,seg_dim,nocs_dim,B,l", TAILS)
def test_coord_tail_cancellation_and_small_channels(device, c0, seg_dim, nocs_dim, B, l):
    """captra_coord_tail_x6 with the cancelling, small-channel layer as the segmentation head (the NOCS head sits behind the sigmoid)."""
    rng = _rng("tail-cancel", c0, seg_dim, l)
    layers, base, ref, mass, chain = _fused_cancel_case(rng, (c0, 128, 128, 128, seg_dim))
    nocs_layers = [((rng.standard_normal((128, 128)) / np.sqrt(128)).astype(np.float32), np.zeros(128, np.float32)),
                   ((rng.standard_normal((128, nocs_dim)) / np.sqrt(128)).astype(np.float32), rng.standard_normal(nocs_dim).astype(np.float32))]
    x, pos = _tile(base, B, l)
    seg, _ = run_tail(device, x, layers + nocs_layers)
    _cancel_report(seg, _expand(ref, pos), _expand(mass, pos), _expand(chain, pos))


def _sa_cancel_case(rng, cfeat, c1, K, B, N, M):
    """One neighbour per centre (its slot varies) whose first-layer output h1 is positive on every channel, channels 2 i and 2 i + 1
    in the ratio 1 + d_i; the other K - 1 neighbours give h1 = 0.  cfeat = 320: the first layer selects feature rows (xyz rows and b1
    zero).  cfeat = 0 / 3: h1[j] = relu(s_j (u . (p - centre) - t)) with the probe point along u and the other points AT the centre."""
    assert N >= 2 * M
    slot = (np.arange(M) * 37 + 5) % K
    idx = np.tile(np.arange(M)[None, :, None], (B, 1, K))
    idx[:, np.arange(M), slot] = M + np.arange(M)
    new_xyz = rng.uniform(-0.5, 0.5, (B, M, 3)).astype(np.float32)
    xyz = np.zeros((B, N, 3), np.float32)
    xyz[:, :M] = new_xyz
    w1 = np.zeros((cfeat + 3, c1), np.float32)
    b1 = np.zeros(c1, np.float32)
    if cfeat == 320:
        rows = rng.permutation(cfeat)[:c1]
        w1[rows, np.arange(c1)] = 1.0
        h, _ = _cancel_pairs(rng, c1, 2, np.arange(c1), (B, M))
        feat = np.zeros((B, cfeat, N), np.float32)
        feat[:, rows, M:2 * M] = np.moveaxis(h, 0, 1)
        xyz[:, M:2 * M] = new_xyz + rng.uniform(-0.1, 0.1, (B, M, 3)).astype(np.float32)
    else:
        u = np.ones(3) / np.sqrt(3.0)
        sc = rng.uniform(0.5, 1.5, c1)
        sc[1::2] = sc[0::2] * (1 + 1e-4 * rng.standard_normal(c1 // 2))
        w1[cfeat:] = u[:, None] * sc[None, :]
        b1[:] = -0.25 * sc
        feat = rng.standard_normal((B, cfeat, N)).astype(np.float32) if cfeat else None      # (noise under zero weights)
        xyz[:, M:2 * M] = new_xyz + (rng.uniform(1.0, 2.0, (B, M, 1)) * u).astype(np.float32)
    xyz_cn = np.ascontiguousarray(xyz.transpose(0, 2, 1))
    h1 = O.pointwise_mlp(O.sa_group(feat, xyz_cn, new_xyz, idx.astype(np.int32)), w1, b1, 1)      # (B, c1, M, K): the exact first layer
    h1p = h1[:, :, np.arange(M), slot]
    assert (h1p > 0).all() and (h1.sum(-1) == h1p).all()                   # positive in the probe slot, zero in every other
    return feat, xyz_cn, new_xyz, idx, (w1, b1), np.ascontiguousarray(h1p)


@pytest.mark.parametrize("cfeat,chans,K,B,N,M", [c for c in SA if c[5] > 1])
def test_sa_cancellation_and_small_channels(device, cfeat, chans, K, B, N, M):
    """captra_sa_scale_x6 with the cancelling, small-channel layer as its third: one non-zero neighbour per centre, so that the max
    selects it; layer 2 a permutation with unit weights; W and -W, since the ReLU behind the max hides the negative side."""
    c1, c2, c3 = chans
    rng = _rng("sa-cancel", cfeat, chans, K, M)
    feat, xyz_cn, new_xyz, idx, l1, h1 = _sa_cancel_case(rng, cfeat, c1, K, B, N, M)
    w2, src = J.pow2_perm(rng, c1, c2, emin=0, emax=0, negate=False)
    live = np.argsort(np.where(src >= 0, src, c2), kind="stable")[:c1]      # live[j] = the channel of h2 that carries h1[j]
    _, w3 = _cancel_pairs(rng, c2, c3, live, (1,))
    z2, z3 = np.zeros(c2, np.float32), np.zeros(c3, np.float32)
    h2 = np.maximum(np.einsum("kc,bkm->bcm", w2.astype(np.float64), h1.astype(np.float64)), 0)
    for sign in (1.0, -1.0):
        w3s = w3 * np.float32(sign)
        ref = np.einsum("kc,bkm->bcm", w3s.astype(np.float64), h2)
        mass = np.einsum("kc,bkm->bcm", np.abs(w3s).astype(np.float64), h2)
        assert (np.abs(ref) <= 1e-3 * mass).all()
        chain = O.pointwise_mlp(O.pointwise_mlp(h1, w2, z2, 1), w3s, z3, 1)
        got = run_sa(device, feat, xyz_cn, new_xyz, idx, [l1, (w2, z2), (w3s, z3)])
        # behind the ReLU (1-Lipschitz: the bound holds for the clipped values as for the raw ones); the raw sum is what must cancel
        e_got, e_chain = np.abs(got.astype(np.float64) - np.maximum(ref, 0)), np.abs(chain.astype(np.float64) - np.maximum(ref, 0))
        bound = 2.0 * e_chain + 4 * U * mass
        print(f"x6 cancellation (sa): worst error / bound = {(e_got / bound).max():.3f}")
        assert (ref > 0).mean() > 0.2 and (e_got <= bound).all(), (e_got / bound).max()


# ==== (e) containment ===============================================================================================================
POISON = [np.float32(np.nan), np.float32(np.inf)]


def _assert_same_bits(a, b, msg=""):
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=msg)


@pytest.mark.parametrize("cin,cout,L,B", DENSE)
def test_dense_containment(device, cin, cout, L, B):
    """One NaN / +Inf at one (cloud, channel, position): every other position and cloud keeps its bits; every statistics tile but
    the one holding the position keeps its bits."""
    rng = _rng("dense-poison", cin, cout, L)
    x = rng.standard_normal((B, cin, L)).astype(np.float32)
    w = (rng.standard_normal((cin, cout)) / np.sqrt(cin)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    ab = np.stack([rng.uniform(0.5, 1.5, (B, cin)), rng.standard_normal((B, cin)) * 0.3], axis=-1).astype(np.float32)
    b0, k0, p0 = B - 1, cin - 3, L - 77
    for abi in (None, ab):
        y, st = run_dense(device, x, w, b, abi, 0, stats=True)
        for bad in POISON:
            xp = x.copy()
            xp[b0, k0, p0] = bad
            yp, stp = run_dense(device, xp, w, b, abi, 0, stats=True)
            keep = np.ones((B, L), bool)
            keep[b0, p0] = False
            _assert_same_bits(yp.transpose(0, 2, 1)[keep], y.transpose(0, 2, 1)[keep])
            keep_t = np.ones((B, L // 128), bool)
            keep_t[b0, p0 // 128] = False
            _assert_same_bits(stp.transpose(0, 2, 1, 3)[keep_t], st.transpose(0, 2, 1, 3)[keep_t])


@pytest.mark.parametrize("c0,B,l", CHAINS)
def test_chain3_containment(device, c0, B, l):
    rng = _rng("chain-poison", c0, l)
    x, layers = _chain_data(rng, (c0, 128, 128, 128), B, l)
    y = run_chain3(device, x, layers, 1)
    b0, k0, p0 = 1, c0 - 1, l - 33
    for bad in POISON:
        xp = x.copy()
        xp[b0, k0, p0] = bad
        yp = run_chain3(device, xp, layers, 1)
        keep = np.ones((B, l), bool)
        keep[b0, p0] = False
        _assert_same_bits(yp.transpose(0, 2, 1)[keep], y.transpose(0, 2, 1)[keep])


@pytest.mark.parametrize("c0,seg_dim,nocs_dim,B,l", TAILS)
def test_coord_tail_containment(device, c0, seg_dim, nocs_dim, B, l):
    rng = _rng("tail-poison", c0, seg_dim, l)
    x, layers = _chain_data(rng, (c0, 128, 128, 128), B, l)
    layers += [(_floor(rng.standard_normal((128, seg_dim)) / np.sqrt(128)), _floor(rng.standard_normal(seg_dim))),
               (_floor(rng.standard_normal((128, 128)) / np.sqrt(128)), _floor(rng.standard_normal(128))),
               (_floor(rng.standard_normal((128, nocs_dim)) / np.sqrt(128)), _floor(rng.standard_normal(nocs_dim)))]
    seg, nocs = run_tail(device, x, layers)
    b0, k0, p0 = B - 1, 5, 31
    for bad in POISON:
        xp = x.copy()
        xp[b0, k0, p0] = bad
        segp, nocsp = run_tail(device, xp, layers)
        keep = np.ones((B, l), bool)
        keep[b0, p0] = False
        _assert_same_bits(segp.transpose(0, 2, 1)[keep], seg.transpose(0, 2, 1)[keep])
        _assert_same_bits(nocsp.transpose(0, 2, 1)[keep], nocs.transpose(0, 2, 1)[keep])


@pytest.mark.parametrize("B,c,c2,cout,l", CLOUD_BIAS)
def test_cloud_bias_containment(device, B, c, c2, cout, l):
    """A poisoned element of x stays at its position; a poisoned element of a cloud's vector stays in its cloud."""
    rng = _rng("cb-poison", B, c, cout, l)
    x = rng.standard_normal((B, c, l)).astype(np.float32)
    v = rng.standard_normal((B, c2, 1)).astype(np.float32)
    w = (rng.standard_normal((c + c2, cout)) / np.sqrt(c + c2)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    y = run_cb(device, x, v, w, b, 1)
    b0, p0 = B - 1, l // 2
    for bad in POISON:
        xp = x.copy()
        xp[b0, c - 2, p0] = bad
        yp = run_cb(device, xp, v, w, b, 1)
        keep = np.ones((B, l), bool)
        keep[b0, p0] = False
        _assert_same_bits(yp.transpose(0, 2, 1)[keep], y.transpose(0, 2, 1)[keep])
        if B > 1:
            vp = v.copy()
            vp[b0, 3, 0] = bad
            yv = run_cb(device, x, vp, w, b, 1)
            _assert_same_bits(yv[:b0], y[:b0])


@pytest.mark.parametrize("cfeat,chans,K,B,N,M", SA)
def test_sa_containment(device, cfeat, chans, K, B, N, M):
    """One poisoned coordinate (and, with features, one poisoned feature) of one point: every centre whose neighbour list does not
    name the point, and every other cloud, keeps its bits."""
    rng = _rng("sa-poison", cfeat, chans, K, M)
    xyz_cn, feat, new_xyz, idx, layers = _sa_random_case(rng, cfeat, chans, K, B, N, M)
    b0, n0 = B - 1, N // 3
    if M == 1:
        idx[idx == n0] = n0 + 1                                  # the single centre must stay clean to be asserted at all
    y = run_sa(device, feat, xyz_cn, new_xyz, idx, layers)
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
            yp = run_sa(device, fp, xp, new_xyz, idx, layers)
            _assert_same_bits(yp.transpose(0, 2, 1)[keep], y.transpose(0, 2, 1)[keep], msg=f"{where} {bad}")
