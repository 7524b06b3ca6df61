"""GPU parity of the fused kernels, the backbone, the networks and the track loop.

Three layers of evidence:
  1. fused kernels vs the C oracle on the same inputs — BIT-EXACT for the MFMA shared-MLP layers
     (both are the k-ascending fmaf chain), canonicalisation and FP interpolation; 1e-5 for the
     pose-fit reductions (different summation order);
  2. captra_amd modules vs the golden vectors captured from the reference (1e-4, the north-star
     tolerance on NOCS coordinates and rotation matrices);
  3. the EvalTrackModel / Trainer loop vs the golden trajectories, teacher-forced per step and
     free-running.
"""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import model as OM
from oracle import ops as O
from tests import clouds
from tests.weights import make_state_dict

pytestmark = pytest.mark.gpu
G = Path(__file__).resolve().parent / "golden"
TOL = 1e-4


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def nocs_batch(ids):
    return np.stack([clouds.s_nocs(i)[0] for i in ids]).astype(np.float32)


# ------------------------------------------------------------------------------ fused kernels
@pytest.mark.parametrize("cin,cout,L,act", [(3, 32, 4096, 1), (6, 64, 1000, 1), (64, 96, 2048, 1), (128, 128, 512, 1),
                                             (323, 128, 8192, 1), (515, 256, 128, 1), (1536, 256, 128, 1),
                                             (128, 2, 4096, 0), (128, 3, 777, 2), (256, 6, 4096, 0), (134, 128, 4100, 1),
                                             (196, 256, 640, 1), (1, 1, 1, 0), (33, 200, 130, 1)])
def test_pointwise_mlp_bit_exact(device, cin, cout, L, act):
    from captra_amd import fused
    rng = np.random.default_rng(cin * 1000 + cout)
    x = rng.standard_normal((2, cin, L)).astype(np.float32)
    wt = (rng.standard_normal((cin, cout)) / np.sqrt(cin)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    got = fused.pointwise_mlp(_dev(x, device), fused.pack(_dev(wt, device), _dev(b, device)), act).cpu().numpy()
    ref = O.pointwise_mlp(x, wt, b, act)
    if act == 2:
        np.testing.assert_allclose(got, ref, atol=2e-7, rtol=0)      # expf differs in the last ulp
    else:
        np.testing.assert_array_equal(got, ref)


@pytest.mark.parametrize("cfeat,cout,n,m,k", [(0, 32, 4096, 512, 32), (3, 64, 4096, 512, 64), (3, 64, 4096, 512, 128),
                                               (320, 128, 512, 128, 64), (320, 128, 512, 128, 128), (5, 40, 300, 37, 32)])
def test_sa_group_mlp_bit_exact(device, cfeat, cout, n, m, k):
    from captra_amd import fused
    rng = np.random.default_rng(cfeat + cout + k)
    B = 2
    xyz_cn = (rng.random((B, 3, n), dtype=np.float32) - 0.5)
    feat = rng.standard_normal((B, cfeat, n)).astype(np.float32) if cfeat else None
    new_xyz = (rng.random((B, m, 3), dtype=np.float32) - 0.5)
    idx = rng.integers(0, n, (B, m, k)).astype(np.int32)
    wt = (rng.standard_normal((cfeat + 3, cout)) / np.sqrt(cfeat + 3)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    got = fused.sa_group_mlp(None if feat is None else _dev(feat, device), _dev(xyz_cn, device), _dev(new_xyz, device),
                             _dev(idx, device), fused.pack(_dev(wt, device), _dev(b, device))).cpu().numpy()
    ref = O.pointwise_mlp(O.sa_group(feat, xyz_cn, new_xyz, idx), wt, b, 1)
    np.testing.assert_array_equal(got, ref)


@pytest.mark.parametrize("cin,cout,m,k", [(32, 64, 512, 32), (64, 128, 512, 64), (96, 128, 512, 128), (128, 256, 128, 64),
                                           (196, 256, 128, 128), (512, 1024, 1, 128), (16, 40, 37, 32)])
def test_mlp_max_bit_exact(device, cin, cout, m, k):
    from captra_amd import fused
    rng = np.random.default_rng(cin + cout + m)
    x = rng.standard_normal((2, cin, m, k)).astype(np.float32)
    wt = (rng.standard_normal((cin, cout)) / np.sqrt(cin)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    out = torch.full((2, cout + 7, m), -1.0, device=device)
    fused.mlp_max(_dev(x, device), fused.pack(_dev(wt, device), _dev(b, device)), out, 5)
    ref = O.max_over_k(O.pointwise_mlp(x, wt, b, 1))
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got[:, 5:5 + cout], ref)
    assert (got[:, :5] == -1).all() and (got[:, 5 + cout:] == -1).all()     # neighbours untouched


@pytest.mark.parametrize("cfeat,chans,n,m,k", [(0, (32, 32, 64), 4096, 512, 32), (3, (64, 64, 128), 4096, 512, 64),
                                                (0, (64, 96, 128), 4096, 512, 128), (320, (128, 128, 256), 512, 128, 64),
                                                (320, (128, 196, 256), 512, 128, 128), (5, (34, 62, 250), 300, 37, 32),
                                                (2, (33, 47, 35), 100, 3, 64), (3, (32, 32, 64), 300, 37, 32),
                                                (3, (64, 96, 128), 700, 41, 128), (320, (128, 196, 256), 200, 5, 64)])
@pytest.mark.parametrize("mode", [0, 1])
def test_sa_scale_fused_bit_exact(device, cfeat, chans, n, m, k, mode):
    """The one-launch SA scale equals gather -> 3 x (conv+BN+ReLU) -> max of the oracle, bit for bit,
    including odd channel counts, a ragged last tile and channel offsets in the output.  mode 0 = production
    dispatch (register-resident sa_wave_kernel for the CAPTRA channel shapes, generic LDS kernel otherwise),
    mode 1 = the generic LDS kernel for every shape."""
    import ctypes
    from captra_amd import _lib, fused
    _lib.lib().captra_sa_fused_set_mode(ctypes.c_int(mode))
    try:
        _sa_scale_fused_case(device, cfeat, chans, n, m, k)
    finally:
        _lib.lib().captra_sa_fused_set_mode(ctypes.c_int(0))


@pytest.mark.parametrize("chans,n,m,k", [((128, 128, 256), 512, 128, 64), ((128, 196, 256), 512, 128, 128),
                                         ((128, 196, 256), 200, 5, 64), ((128, 128, 256), 333, 37, 32)])
def test_sa_scale_pre_bit_exact(device, chans, n, m, k):
    """First layer's feature part computed once per source point (captra_pointwise_mlp on the feature rows) + the
    scale kernel continuing the chain with the xyz rows == the oracle's gather -> 3 layers -> max, bit for bit."""
    from captra_amd import fused
    cfeat = 320
    rng = np.random.default_rng(sum(chans) + n + k)
    B = 2
    xyz_cn = (rng.random((B, 3, n), dtype=np.float32) - 0.5)
    feat = rng.standard_normal((B, cfeat, n)).astype(np.float32)
    new_xyz = (rng.random((B, m, 3), dtype=np.float32) - 0.5)
    idx = rng.integers(0, n, (B, m, k)).astype(np.int32)
    dims = (cfeat + 3,) + chans
    layers = [((rng.standard_normal((dims[i], dims[i + 1])) / np.sqrt(dims[i])).astype(np.float32),
               rng.standard_normal(dims[i + 1]).astype(np.float32)) for i in range(3)]
    packed = [fused.pack(_dev(w, device), _dev(b, device)) for w, b in layers]
    assert fused.sa_scale_pre_supported(cfeat, packed, k)
    out = torch.full((B, chans[2] + 9, m), -1.0, device=device)
    v1 = fused.sa_first_layer_pre(_dev(feat, device), packed[0])
    fused.sa_scale_pre(v1, _dev(xyz_cn, device), _dev(new_xyz, device), _dev(idx, device), packed, out, 4, cfeat)
    x = O.sa_group(feat, xyz_cn, new_xyz, idx)
    for w, b in layers:
        x = O.pointwise_mlp(x, w, b, 1)
    ref = O.max_over_k(x)
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got[:, 4:4 + chans[2]], ref)
    assert (got[:, :4] == -1).all() and (got[:, 4 + chans[2]:] == -1).all()


@pytest.mark.parametrize("chans,n,m,k,B", [((128, 128, 256), 512, 128, 64, 2), ((128, 196, 256), 512, 128, 128, 2),
                                           ((128, 196, 256), 512, 128, 128, 5), ((128, 128, 256), 512, 128, 64, 33),
                                           ((128, 196, 256), 200, 6, 64, 3), ((128, 128, 256), 333, 36, 32, 2),
                                           ((128, 196, 256), 700, 1, 128, 1)])
def test_sa_scale_pipe_bit_exact(device, chans, n, m, k, B):
    """The pipelined SA2 kernel (csrc/sa_pipe.hip: a wave per centre walking K/32 slices, next slice's gather prefetched,
    deferred epilogues, weight ring of three, running maximum in registers) on the point-major pre-transformed first layer
    == the oracle's gather -> 3 layers -> max, bit for bit: one, two and four slices per centre, several centres per wave,
    batches that do not fill the chip, channel offsets in the output; and the point-major dense layer == the channel-major
    one, transposed."""
    from captra_amd import fused
    cfeat = 320
    rng = np.random.default_rng(sum(chans) + n + k + B)
    xyz_cn = (rng.random((B, 3, n), dtype=np.float32) - 0.5)
    feat = rng.standard_normal((B, cfeat, n)).astype(np.float32)
    new_xyz = (rng.random((B, m, 3), dtype=np.float32) - 0.5)
    idx = rng.integers(0, n, (B, m, k)).astype(np.int32)
    dims = (cfeat + 3,) + chans
    layers = [((rng.standard_normal((dims[i], dims[i + 1])) / np.sqrt(dims[i])).astype(np.float32),
               rng.standard_normal(dims[i + 1]).astype(np.float32)) for i in range(3)]
    packed = [fused.pack(_dev(w, device), _dev(b, device)) for w, b in layers]
    assert fused.sa_scale_pipe_supported(cfeat, packed, m, k)
    v1pm = fused.sa_first_layer_pre_pm(_dev(feat, device), packed[0])
    v1 = fused.sa_first_layer_pre(_dev(feat, device), packed[0])
    assert torch.equal(v1pm, v1.transpose(1, 2))
    out = torch.full((B, chans[2] + 9, m), -1.0, device=device)
    fused.sa_scale_pre_pm(v1pm, _dev(xyz_cn, device), _dev(new_xyz, device), _dev(idx, device), packed, out, 4, cfeat)
    x = O.sa_group(feat, xyz_cn, new_xyz, idx)
    for w, b in layers:
        x = O.pointwise_mlp(x, w, b, 1)
    ref = O.max_over_k(x)
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got[:, 4:4 + chans[2]], ref)
    assert (got[:, :4] == -1).all() and (got[:, 4 + chans[2]:] == -1).all()
    # and against the previous-generation kernel on the same inputs
    out2 = torch.full_like(out, -1.0)
    fused.sa_scale_pre(v1, _dev(xyz_cn, device), _dev(new_xyz, device), _dev(idx, device), packed, out2, 4, cfeat)
    assert torch.equal(out, out2)


@pytest.mark.parametrize("n,s,B,dup", [(4096, 512, 3, False), (512, 128, 5, False), (700, 37, 2, True), (130, 2, 2, False), (64, 1, 1, False),
                                        (4096, 512, 1, True)])
def test_three_nn_weights_four_lanes_per_point_equals_one_lane(device, n, s, B, dup):
    """captra_three_nn_weights with four lanes per unknown point (quarter chains merged by (distance, index)) == the one-lane scan,
    indices and weights bit for bit -- also under exact distance ties (duplicated known points: the earlier index wins), fewer than
    three known points and tile tails that are not multiples of four."""
    import ctypes
    from captra_amd import _lib, fused
    rng = np.random.default_rng(n + s + B)
    unknown = (rng.random((B, n, 3), dtype=np.float32) - 0.5)
    known = (rng.random((B, s, 3), dtype=np.float32) - 0.5)
    if dup and s >= 8:
        known[:, s // 2:] = known[:, :s - s // 2]                  # every point twice: ties everywhere
        unknown[:, :s // 2] = known[:, :s // 2]                     # and exact zeros
    res = []
    for knob in (0, 1):
        _lib.lib().captra_three_nn_set_split(ctypes.c_int(knob))
        try:
            res.append(fused.three_nn_weights(_dev(unknown, device), _dev(known, device)))
        finally:
            _lib.lib().captra_three_nn_set_split(ctypes.c_int(1))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


@pytest.mark.parametrize("c1,c2,cout,l,bcast,B", [(3, 512, 256, 128, False, 4), (512, 1024, 256, 128, True, 4), (3, 512, 256, 128, False, 40),
                                                   (7, 130, 70, 77, False, 2), (320, 256, 256, 512, True, 3)])
def test_pointwise_mlp_two_sources_equals_concat_bit_for_bit(device, c1, c2, cout, l, bcast, B):
    """captra_pointwise_mlp2: the dense layer on [x; x2] read from the two tensors as they are (SA3's [xyz, feat], FP3's
    [points1, repeat(points2)]: pointnet_utils.py:171-188, 265-270) == captra_pointwise_mlp on the concatenated tensor, bit for bit
    (the operand rows are consumed in the concat's order), small- and large-launch shapes, and == the oracle's chain."""
    from captra_amd import fused
    rng = np.random.default_rng(c1 + c2 + cout + l)
    x = rng.standard_normal((B, c1, l)).astype(np.float32)
    x2 = rng.standard_normal((B, c2, 1 if bcast else l)).astype(np.float32)
    w = (rng.standard_normal((c1 + c2, cout)) / np.sqrt(c1 + c2)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    lin = fused.pack(_dev(w, device), _dev(b, device))
    cat = np.concatenate([x, np.broadcast_to(x2, (B, c2, l))], axis=1)
    want = fused.pointwise_mlp(_dev(cat, device), lin, fused.ACT_RELU)
    # (the two tensors must lie within 2^30 bytes of each other for the one buffer descriptor -- the wrapper returns None otherwise
    # and the caller concatenates; here both are carved out of one allocation)
    flat = torch.empty(x.size + x2.size, dtype=torch.float32, device=device)
    xd, x2d = flat[:x.size].view(x.shape), flat[x.size:].view(x2.shape)
    xd.copy_(torch.from_numpy(x)); x2d.copy_(torch.from_numpy(x2))
    got = fused.pointwise_mlp2(xd, x2d, lin, fused.ACT_RELU)
    assert got is not None and torch.equal(got, want)
    far = fused.pointwise_mlp2(_dev(x, device), _dev(x2, device), lin, fused.ACT_RELU)       # wherever the allocator put them
    assert far is None or torch.equal(far, want)
    np.testing.assert_array_equal(got.cpu().numpy(), O.pointwise_mlp(cat, w, b, 1))


@pytest.mark.parametrize("cfeat,chans,n,m,k,B", [(0, (64, 96, 128), 4096, 512, 128, 9), (3, (64, 64, 128), 4096, 512, 64, 5),
                                                  (320, (128, 196, 256), 512, 128, 128, 33), (320, (128, 128, 256), 512, 128, 64, 17),
                                                  (0, (64, 96, 128), 700, 41, 128, 1)])
def test_sa_scale_dynamic_centre_hand_out_bit_exact(device, cfeat, chans, n, m, k, B):
    """captra_launch_opts::dyn_slot (host layer: _lib.launch_options(dyn_pool=...)): the persistent SA kernels take their centres from a zeroed counter instead of the static walk
    (a workgroup that becomes resident late finds the work done).  Which wave computes a centre changes nothing: the launch
    with the counter, the static launch and (through the other tests) the oracle agree bit for bit; every launch takes a
    fresh slot of the caller's pool and leaves the number of hand-outs in it (>= the centres)."""
    import ctypes
    from captra_amd import _lib, fused
    rng = np.random.default_rng(cfeat + sum(chans) + k + B)
    xyz_cn = _dev(rng.random((B, 3, n), dtype=np.float32) - 0.5, device)
    feat = _dev(rng.standard_normal((B, cfeat, n)).astype(np.float32), device) if cfeat else None
    new_xyz = _dev(rng.random((B, m, 3), dtype=np.float32) - 0.5, device)
    idx = _dev(rng.integers(0, n, (B, m, k)).astype(np.int32), device)
    dims = (cfeat + 3,) + chans
    packed = [fused.pack(_dev((rng.standard_normal((dims[i], dims[i + 1])) / np.sqrt(dims[i])).astype(np.float32), device),
                         _dev(rng.standard_normal(dims[i + 1]).astype(np.float32), device)) for i in range(3)]

    def run():
        out = torch.full((B, chans[2] + 9, m), -1.0, device=device)
        if cfeat == 320:
            v1pm = fused.sa_first_layer_pre_pm(feat, packed[0])
            fused.sa_scale_pre_pm(v1pm, xyz_cn, new_xyz, idx, packed, out, 4, cfeat)
        else:
            fused.sa_scale_fused(feat, xyz_cn, new_xyz, idx, packed, out, 4)
        return out

    _lib.lib().captra_sa_fused_set_split(ctypes.c_int(0))            # (never the slice-per-wave form: it has no centre walk)
    pool = torch.full((4,), 12345, dtype=torch.int32, device=device)
    try:
        want = run()
        with _lib.launch_options(dyn_pool=(pool.data_ptr(), 4)):
            got = [run() for _ in range(3)]
    finally:
        _lib.lib().captra_sa_fused_set_split(ctypes.c_int(1))
    for g in got:
        assert torch.equal(g, want)
    counts = pool.cpu().tolist()
    assert counts[3] == 12345 and all(c >= B * m for c in counts[:3]), counts


@pytest.mark.parametrize("cfeat,chans,n,m,k,B", [(0, (64, 96, 128), 4096, 512, 128, 1), (3, (64, 64, 128), 4096, 512, 64, 1),
                                                  (3, (64, 96, 128), 700, 41, 128, 3), (320, (128, 196, 256), 512, 128, 128, 1),
                                                  (320, (128, 128, 256), 512, 128, 64, 1), (320, (128, 196, 256), 200, 6, 64, 3)])
def test_sa_scale_split_slices_bit_exact_at_batch_one(device, cfeat, chans, n, m, k, B):
    """Small batches (the reference's own speed convention is --batch_size 1, README.md:267): a wave owns ONE 32-neighbour slice of
    a centre instead of the whole centre, the slices' maxima meet in an integer atomic max on the zeroed output.  Same chain per
    position, exact max: the forced-split launch, the never-split launch and the oracle agree bit for bit, and rows outside the
    scale's channel block are untouched."""
    import ctypes
    from captra_amd import _lib, fused
    rng = np.random.default_rng(cfeat + sum(chans) + k + B)
    xyz_cn = (rng.random((B, 3, n), dtype=np.float32) - 0.5)
    feat = rng.standard_normal((B, cfeat, n)).astype(np.float32) if cfeat else None
    new_xyz = (rng.random((B, m, 3), dtype=np.float32) - 0.5)
    idx = rng.integers(0, n, (B, m, k)).astype(np.int32)
    dims = (cfeat + 3,) + chans
    layers = [((rng.standard_normal((dims[i], dims[i + 1])) / np.sqrt(dims[i])).astype(np.float32),
               rng.standard_normal(dims[i + 1]).astype(np.float32)) for i in range(3)]
    packed = [fused.pack(_dev(w, device), _dev(b, device)) for w, b in layers]
    outs = []
    for knob in (0, 2, 1):
        _lib.lib().captra_sa_fused_set_split(ctypes.c_int(knob))
        try:
            out = torch.full((B, chans[2] + 9, m), -1.0, device=device)
            if cfeat == 320:
                v1pm = fused.sa_first_layer_pre_pm(_dev(feat, device), packed[0])
                fused.sa_scale_pre_pm(v1pm, _dev(xyz_cn, device), _dev(new_xyz, device), _dev(idx, device), packed, out, 4, cfeat)
            else:
                fused.sa_scale_fused(None if feat is None else _dev(feat, device), _dev(xyz_cn, device), _dev(new_xyz, device), _dev(idx, device), packed, out, 4)
            outs.append(out)
        finally:
            _lib.lib().captra_sa_fused_set_split(ctypes.c_int(1))
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    x = O.sa_group(feat, xyz_cn, new_xyz, idx)
    for w, b in layers:
        x = O.pointwise_mlp(x, w, b, 1)
    got = outs[1].cpu().numpy()
    np.testing.assert_array_equal(got[:, 4:4 + chans[2]], O.max_over_k(x))
    assert (got[:, :4] == -1).all() and (got[:, 4 + chans[2]:] == -1).all()


def _sa_scale_fused_case(device, cfeat, chans, n, m, k):
    from captra_amd import fused
    rng = np.random.default_rng(cfeat + sum(chans) + k)
    B = 2
    xyz_cn = (rng.random((B, 3, n), dtype=np.float32) - 0.5)
    feat = rng.standard_normal((B, cfeat, n)).astype(np.float32) if cfeat else None
    new_xyz = (rng.random((B, m, 3), dtype=np.float32) - 0.5)
    idx = rng.integers(0, n, (B, m, k)).astype(np.int32)
    dims = (cfeat + 3,) + chans
    layers = [((rng.standard_normal((dims[i], dims[i + 1])) / np.sqrt(dims[i])).astype(np.float32),
               rng.standard_normal(dims[i + 1]).astype(np.float32)) for i in range(3)]
    out = torch.full((B, chans[2] + 9, m), -1.0, device=device)
    fused.sa_scale_fused(None if feat is None else _dev(feat, device), _dev(xyz_cn, device), _dev(new_xyz, device),
                         _dev(idx, device), [fused.pack(_dev(w, device), _dev(b, device)) for w, b in layers], out, 4)
    x = O.sa_group(feat, xyz_cn, new_xyz, idx)
    for w, b in layers:
        x = O.pointwise_mlp(x, w, b, 1)
    ref = O.max_over_k(x)
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got[:, 4:4 + chans[2]], ref)
    assert (got[:, :4] == -1).all() and (got[:, 4 + chans[2]:] == -1).all()


@pytest.mark.parametrize("c0,l,act3", [(134, 4096, 1), (131, 1000, 1), (134, 77, 0), (131, 4096, 2), (100, 256, 1)])
def test_mlp_chain3_bit_exact(device, c0, l, act3):
    """Three dense layers in one launch == the oracle's layer-by-layer fmaf chains == three captra_pointwise_mlp
    launches, bit for bit; ragged L, every final activation, and the fallback for a shape that is not instantiated."""
    from captra_amd import fused
    rng = np.random.default_rng(c0 + l + act3)
    B = 3
    x = rng.standard_normal((B, c0, l)).astype(np.float32)
    dims = (c0, 128, 128, 128)
    layers = [((rng.standard_normal((dims[i], dims[i + 1])) / np.sqrt(dims[i])).astype(np.float32),
               rng.standard_normal(dims[i + 1]).astype(np.float32)) for i in range(3)]
    packed = [fused.pack(_dev(w, device), _dev(b, device)) for w, b in layers]
    got = fused.mlp_chain3(_dev(x, device), packed, act3).cpu().numpy()
    ref = x
    for i, (w, b) in enumerate(layers):
        ref = O.pointwise_mlp(ref, w, b, 1 if i < 2 else act3)
    if act3 == 2:   # sigmoid: device expf vs libm expf, not an exactness contract
        np.testing.assert_allclose(got, ref, rtol=0, atol=2e-7)
    else:
        np.testing.assert_array_equal(got, ref)
    fused.USE_MLP_CHAIN = False
    try:
        layered = fused.mlp_chain3(_dev(x, device), packed, act3).cpu().numpy()
    finally:
        fused.USE_MLP_CHAIN = True
    np.testing.assert_array_equal(got, layered)


def test_backbone_layer_by_layer_kernels_equal_fused_scale(device):
    """USE_SA_FUSED off routes the SA scales through sa_group_mlp / pointwise_mlp / mlp_max: same bits."""
    from captra_amd import fused
    from captra_amd.backbones import PointNet2Msg
    from captra_amd.configs import make_config
    cfg = make_config("1")
    net = PointNet2Msg(cfg, 128, use_xyz_feat=True)
    net.load_state_dict(make_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=4))
    net = net.to(device).eval()
    cloud_cn = _dev(nocs_batch([3]).transpose(0, 2, 1), device)
    with torch.no_grad():
        a = net(cloud_cn).cpu().numpy()
        fused.USE_SA_FUSED = False
        fused.USE_MLP_CHAIN = False
        try:
            b = net(cloud_cn).cpu().numpy()
        finally:
            fused.USE_SA_FUSED = True
            fused.USE_MLP_CHAIN = True
        fused.USE_SA_PRE = False                      # full gather-GEMM first layer instead of the pre-transformed one
        try:
            c = net(cloud_cn).cpu().numpy()
        finally:
            fused.USE_SA_PRE = True
    np.testing.assert_array_equal(a, c)
    with torch.no_grad():
        pass
    np.testing.assert_array_equal(a, b)


def test_mlp_max_rejects_unsupported_k(device):
    from captra_amd import _lib, fused
    with pytest.raises(_lib.CaptraHipError):
        fused.mlp_max(torch.zeros(1, 4, 3, 48, device=device), fused.pack(torch.zeros(4, 8, device=device),
                      torch.zeros(8, device=device)), torch.zeros(1, 8, 3, device=device), 0)


@pytest.mark.parametrize("P", [1, 4])
def test_canonicalize_bit_exact(device, P):
    from captra_amd import fused
    rng = np.random.default_rng(P)
    B, N = 3, 4096
    pts = (rng.random((B, 3, N), dtype=np.float32) - 0.5)
    mean = rng.standard_normal((B, 3)).astype(np.float32)
    rot = np.stack([clouds._rot_y(0.1 * i) @ clouds._rot_x(0.2 * i) for i in range(B * P)]).astype(np.float32)
    trans = rng.standard_normal((B * P, 3)).astype(np.float32)
    scale = (0.2 + rng.random(B * P)).astype(np.float32)
    cn, n3 = fused.canonicalize(_dev(pts, device), _dev(mean, device), _dev(rot, device), _dev(trans, device), _dev(scale, device), P)
    rcn, rn3 = O.canonicalize(pts, mean, rot, trans, scale, P)
    np.testing.assert_array_equal(cn.cpu().numpy(), rcn)
    np.testing.assert_array_equal(n3.cpu().numpy(), rn3)


@pytest.mark.parametrize("n,s,c1,c2", [(512, 128, 320, 256), (4096, 512, 3, 128), (4096, 512, 6, 128), (300, 7, 0, 5), (1500, 6000, 2, 9)])
def test_fp_interpolate_concat_bit_exact(device, n, s, c1, c2):
    from captra_amd import fused
    rng = np.random.default_rng(n + s)
    B = 2
    unknown = (rng.random((B, n, 3), dtype=np.float32) - 0.5)
    known = (rng.random((B, s, 3), dtype=np.float32) - 0.5)
    known[:, : min(s, n) // 2] = unknown[:, : min(s, n) // 2]          # exact coincidences (d = 0)
    skip = rng.standard_normal((B, c1, n)).astype(np.float32) if c1 else None
    fk = rng.standard_normal((B, c2, s)).astype(np.float32)
    got = fused.fp_interpolate_concat(_dev(unknown, device), _dev(known, device), None if skip is None else _dev(skip, device),
                                      _dev(fk, device)).cpu().numpy()
    np.testing.assert_array_equal(got, O.fp_interpolate_concat(unknown, known, skip, fk))


@pytest.mark.parametrize("B,C,N,groups,relu", [(2, 512, 4096, 256, True), (3, 256, 4096, 128, True), (2, 8, 100, 4, False),
                                                (1, 6, 64, 1, True)])
def test_group_norm_relu_vs_torch(device, B, C, N, groups, relu):
    from captra_amd import fused
    rng = np.random.default_rng(C + N)
    x = _dev((rng.standard_normal((B, C, N)) * 3 + 1).astype(np.float32), device)
    gamma = _dev(rng.uniform(0.5, 1.5, C).astype(np.float32), device)
    beta = _dev(rng.normal(0, 0.3, C).astype(np.float32), device)
    got = fused.group_norm_relu(x, groups, gamma, beta, 1e-5, relu)
    ref = torch.nn.functional.group_norm(x.double(), groups, gamma.double(), beta.double(), 1e-5)
    if relu:
        ref = torch.relu(ref)
    np.testing.assert_allclose(got.cpu().numpy(), ref.float().cpu().numpy(), atol=2e-6, rtol=2e-6)


@pytest.mark.parametrize("tag", ["bottle", "camera"])
def test_shared_geometry_is_bit_identical(device, tag):
    """For single-part objects RotationNet reuses CoordNet's FPS / ball-query / 3-NN results: same poses."""
    trainer, cfg, sd, data = _trainer(tag, device)
    model = trainer.model.eval()
    outs = []
    for share in (True, False):
        model.share_geometry = share
        torch.manual_seed(7)
        trainer.test(data, save=False, no_eval=True)
        outs.append([{k: v.cpu().numpy() for k, v in p.items()} for p in model.pred_dict["poses"]])
    for a, b in zip(*outs):
        for k in a:
            np.testing.assert_array_equal(a[k], b[k])


@pytest.mark.parametrize("tag", ["bottle", "drawers"])
def test_hipgraph_replay_equals_eager(device, tag):
    """The captured step replays to exactly the poses of the eager step, frame after frame."""
    from captra_amd.graph import TrackStepGraph
    trainer, cfg, sd, data = _trainer(tag, device)
    model = trainer.model.eval()
    model.track_cfg["gt_label"] = False
    model.set_data(data)
    pose0 = {k: v.clone() for k, v in model.feed_dict[0]["gt_part"].items()}
    g = TrackStepGraph(model, model.feed_dict[1]["points"], model.feed_dict[1]["points_mean"], pose0)
    pe, pg = pose0, pose0
    for i in range(1, len(data)):
        f, nf = model.feed_dict[i], model.npcs_feed_dict[i]
        with torch.no_grad():
            _, pe = model.track_step(f, nf, pe)
        pg = {k: v.clone() for k, v in g.replay(f["points"], f["points_mean"], pg).items()}
        for k in pe:
            np.testing.assert_array_equal(pe[k].cpu().numpy(), pg[k].cpu().numpy(), err_msg=f"frame {i} {k}")
    # the inputs go into the captured buffers in ONE launch (captra_copy_multi) when they are plain contiguous tensors, through
    # torch copies otherwise: a strided view of the same values replays to the same pose
    f = model.feed_dict[1]
    want = {k: v.clone() for k, v in g.replay(f["points"], f["points_mean"], pose0).items()}
    wide = torch.stack([f["points"], f["points"]], dim=-1)
    pose_nc = dict(pose0, rotation=pose0["rotation"].transpose(-1, -2).contiguous().transpose(-1, -2))
    assert not wide[..., 0].is_contiguous() and not pose_nc["rotation"].is_contiguous()
    got = g.replay(wide[..., 0], f["points_mean"], pose_nc)
    for k in want:
        assert torch.equal(got[k], want[k]), k


@pytest.mark.parametrize("tag", ["bottle", "drawers"])
def test_free_running_lanes_equal_eager(device, tag):
    """TrackLanes: the batch as two sub-batches, each replaying its own captured step on its own stream and handing its pose
    over to itself — every frame's gathered record equals the eager whole-batch step bit for bit (ring of 2: slots reused)."""
    from captra_amd.graph import TrackLanes
    trainer, cfg, sd, data = _trainer(tag, device)
    model = trainer.model.eval()
    model.track_cfg["gt_label"] = False
    model.set_data(data)
    pose0 = {k: v.clone() for k, v in model.feed_dict[0]["gt_part"].items()}
    lanes = TrackLanes(model, model.feed_dict[1]["points"], model.feed_dict[1]["points_mean"], pose0, lanes=2, ring=2)
    eager, pe = [], pose0
    for rep in range(2):                      # the second pass restarts the trajectories through set_pose
        got = []
        for i in range(1, len(data)):
            f = model.feed_dict[i]
            got.append({k: v.clone() for k, v in lanes.gather(lanes.step(f["points"], f["points_mean"])).items()})
        if rep == 0:
            # (lanes never take the few-trajectory split-k form -- a sub-batch must compute what the whole batch computes at any
            # size --, so the eager comparand of this small test batch is run without it too)
            for i in range(1, len(data)):
                with torch.no_grad():
                    _, pe = model.track_step(model.feed_dict[i], model.npcs_feed_dict[i], pe, allow_split_k=False)
                eager.append(pe)
        for i, (a, b) in enumerate(zip(eager, got)):
            for k in a:
                np.testing.assert_array_equal(a[k].cpu().numpy(), b[k].cpu().numpy(), err_msg=f"pass {rep} frame {i + 1} {k}")
        torch.cuda.synchronize()
        lanes.set_pose(pose0)
    with pytest.raises(ValueError):
        TrackLanes(model, model.feed_dict[1]["points"], model.feed_dict[1]["points_mean"], pose0, lanes=3)


def test_track_loop_with_graph_and_lanes_equals_eager(device):
    """Trainer.test with cfg['hipgraph']: 2 trajectories replay one captured step, 32 run as two free-running lanes
    (EvalTrackModel._lanes_usable) — poses and CoordinateNet maps of every frame equal the eager loop's, twice in a row
    (the second call restarts the lanes through set_pose)."""
    from captra_amd.graph import TrackLanes, TrackStepGraph
    trainer, cfg, sd, _ = _trainer("bottle", device)
    model = trainer.model
    for B, kind in ((2, TrackStepGraph), (32, TrackLanes)):
        data = clouds.make_trajectory("nocs", B, 4, seed=5)
        runs = []
        for use_graph in (False, True, True):
            model.use_graph = use_graph
            torch.manual_seed(11)
            pred, _ = trainer.test(data, save=False, no_eval=True)
            runs.append(([{k: v.cpu().numpy() for k, v in p.items()} for p in pred["poses"]],
                         [None if n is None else {k: v.cpu().numpy() for k, v in n.items()} for n in pred["npcs_pred"]]))
        assert isinstance(model._graph, kind)
        for poses, npcs in runs[1:]:
            for i, (a, b) in enumerate(zip(runs[0][0], poses)):
                for k in a:
                    np.testing.assert_array_equal(a[k], b[k], err_msg=f"B={B} frame {i} {k}")
            for i, (a, b) in enumerate(zip(runs[0][1], npcs)):
                if a is not None:
                    for k in b:
                        np.testing.assert_array_equal(a[k], b[k], err_msg=f"B={B} frame {i} npcs {k}")
    model.use_graph = False


def test_captured_graph_stays_valid_when_another_model_refolds(device):
    """the weights version is a process-wide counter, staleness is per model -- a second model that loads new
    weights (or flips train / eval) must not invalidate this model's captured step, while this model's own reload does."""
    from tests.weights import make_physical_state_dict
    trainer, cfg, sd, _, _ = _trainer_physical("bottle", device)
    model = trainer.model
    model.use_graph = True
    data = clouds.make_trajectory("nocs", 2, 3, seed=5)
    torch.manual_seed(3)
    first, _ = trainer.test(data, save=False, no_eval=True)
    g = model._graph
    other, _, _, _, _ = _trainer_physical("bottle", device)                   # a second model object of the process ...
    other.model.load_state_dict(make_physical_state_dict({k: tuple(v.shape) for k, v in other.model.state_dict().items()}, 9, 1, True, "nocs"))
    other.model.train()
    other.model.eval()                                                       # ... re-folding its own weights
    assert not g.stale()
    torch.manual_seed(3)
    second, _ = trainer.test(data, save=False, no_eval=True)
    assert model._graph is g
    for a, b in zip(first["poses"], second["poses"]):
        for k in a:
            np.testing.assert_array_equal(a[k].cpu().numpy(), b[k].cpu().numpy())
    model.load_state_dict(make_physical_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, 8, 1, True, "nocs"))
    assert g.stale()
    model.use_graph = False


def test_captured_graph_owns_its_weights_and_is_recaptured_when_they_change(device):
    """a captured step reads the folded weights through raw device pointers.  (a) Trainer.test() calls
    model.eval() every time -- on a model already in eval mode that must NOT drop the folded tensors (same tensor objects
    before and after), and the graph holds references to them in any case; (b) after load_state_dict() the graph is stale:
    the loop recaptures and the poses are the NEW weights' (equal to an eager run), a direct replay of the old graph raises."""
    from captra_amd.fold import collect_folded
    from captra_amd.graph import TrackStepGraph
    from tests.weights import make_physical_state_dict
    trainer, cfg, sd, _, _ = _trainer_physical("bottle", device)
    model = trainer.model
    model.use_graph = True
    data = clouds.make_trajectory("nocs", 2, 3, seed=5)
    torch.manual_seed(3)
    first, _ = trainer.test(data, save=False, no_eval=True)
    g = model._graph
    assert isinstance(g, TrackStepGraph) and len(g.weights) > 40 and not g.stale()
    ptrs = sorted(w.wt.data_ptr() for w in collect_folded(model))
    filler = [torch.full((1 << 20,), float("nan"), device=device) for _ in range(8)]      # would land in freed weight blocks
    torch.manual_seed(3)
    second, _ = trainer.test(data, save=False, no_eval=True)                              # model.eval() again, same graph
    assert model._graph is g and sorted(w.wt.data_ptr() for w in collect_folded(model)) == ptrs
    for a, b in zip(first["poses"], second["poses"]):
        for k in a:
            np.testing.assert_array_equal(a[k].cpu().numpy(), b[k].cpu().numpy())
    del filler
    # new weights: stale graph, recapture, results of the new weights
    sd2 = make_physical_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, 8, 1, True, "nocs")
    model.load_state_dict(sd2)
    assert g.stale()
    with pytest.raises(RuntimeError):
        g.replay(model.feed_dict[1]["points"], model.feed_dict[1]["points_mean"], first["poses"][0])
    torch.manual_seed(3)
    third, _ = trainer.test(data, save=False, no_eval=True)
    assert model._graph is not g and not model._graph.stale()
    model.use_graph = False
    torch.manual_seed(3)
    eager, _ = trainer.test(data, save=False, no_eval=True)
    changed = False
    for a, b, c in zip(third["poses"][1:], eager["poses"][1:], first["poses"][1:]):
        for k in a:
            np.testing.assert_array_equal(a[k].cpu().numpy(), b[k].cpu().numpy())
            changed |= not np.array_equal(a[k].cpu().numpy(), c[k].cpu().numpy())
    assert changed


def test_saved_result_corners_are_the_reference_symmetric_extent(device, tmp_path):
    """pred['corners'] of the result pickles = get_pred_nocs_corners of the own-part predicted NOCS
    ([-max|x|, +max|x|], reference model.py:489-493), i.e. the boxes compute_loss evaluates -- not a [min, max] box."""
    import pickle
    from captra_amd.loss import choose_coord_by_label
    from captra_amd.pose_utils.bbox_utils import get_pred_nocs_corners
    trainer, cfg, sd, data = _trainer("drawers", device)
    cfg["experiment_dir"] = trainer.model.cfg["experiment_dir"] = str(tmp_path)
    pred, _ = trainer.test(data, save=True, no_eval=True)
    files = sorted((tmp_path / "results" / "data").glob("*.pkl"))
    assert len(files) == 2
    for b, path in enumerate(files):
        with open(path, "rb") as fh:
            rec = pickle.load(fh)
        assert rec["pred"]["corners"][0] is None
        for i in range(1, len(data)):
            n = pred["npcs_pred"][i]
            labels = torch.max(n["seg"], dim=-2)[1]
            want = get_pred_nocs_corners(labels, choose_coord_by_label(n["nocs"].transpose(-1, -2), labels), cfg["num_parts"])[b]
            got = np.asarray(rec["pred"]["corners"][i])
            np.testing.assert_array_equal(got, want)
            np.testing.assert_array_equal(got[:, 0], -got[:, 1])            # symmetric about the origin


@pytest.mark.parametrize("sym", [False, True])
def test_part_fit_st_vs_oracle_and_golden(device, sym):
    from captra_amd.pose_utils.pose_fit import part_fit_st_cn, part_fit_st_no_ransac
    g = np.load(G / "g8_pose_fit.npz")
    rng = np.random.default_rng(88)
    B, P, N = 3, 2, 600
    src = (rng.random((B, P, N, 3)) - 0.5).astype(np.float32)
    Rgt = np.stack([clouds._rot_y(0.3 * (b + 1)) @ clouds._rot_x(0.2 * (p + 1)) for b in range(B) for p in range(P)]).reshape(B, P, 3, 3).astype(np.float32)
    tgt1 = (0.7 * np.einsum("bpij,bpnj->bpni", Rgt, src) + np.array([0.1, -0.2, 1.0])).astype(np.float32)
    tgt1 += rng.normal(0, 0.01, tgt1.shape).astype(np.float32)
    tgt = np.repeat(tgt1[:, :1], P, axis=1)
    labels = g["labels"].astype(np.int64)
    # reference-signature entry point
    model, valid = part_fit_st_no_ransac(_dev(labels, device), _dev(src, device), _dev(tgt, device), _dev(Rgt, device),
                                         {"num_parts": P, "sym": sym})
    ref_valid = g[f"fit_sym{int(sym)}_valid"]
    np.testing.assert_array_equal(valid.cpu().numpy(), ref_valid)
    np.testing.assert_allclose(model["scale"].cpu().numpy()[ref_valid], g[f"fit_sym{int(sym)}_scale"][ref_valid], atol=1e-5, rtol=1e-5)
    np.testing.assert_allclose(model["translation"].cpu().numpy()[ref_valid], g[f"fit_sym{int(sym)}_trans"][ref_valid], atol=1e-5, rtol=1e-5)
    # channel-major fast path vs the oracle
    src_cn = np.ascontiguousarray(src.transpose(0, 1, 3, 2))
    tgt_cn = np.ascontiguousarray(tgt1[:, 0].transpose(0, 2, 1))
    s, t, v = part_fit_st_cn(_dev(labels.astype(np.int32), device), _dev(src_cn, device), _dev(tgt_cn, device), _dev(Rgt, device), sym)
    so, to, vo = O.part_fit_st(labels, src_cn, tgt_cn, Rgt, sym)
    np.testing.assert_array_equal(v.cpu().numpy(), vo.astype(bool))
    np.testing.assert_allclose(s.cpu().numpy(), so, atol=1e-5, rtol=1e-5)
    np.testing.assert_allclose(t.cpu().numpy()[..., 0], to, atol=1e-5, rtol=1e-5)


def test_procrustes_rot3_vs_golden(device):
    from captra_amd.pose_utils.procrustes import rotate_pts_batch
    g = np.load(G / "g8_pose_fit.npz")
    rng = np.random.default_rng(88)
    B, P, N = 3, 2, 600
    src = (rng.random((B, P, N, 3)) - 0.5).astype(np.float32)
    Rgt = np.stack([clouds._rot_y(0.3 * (b + 1)) @ clouds._rot_x(0.2 * (p + 1)) for b in range(B) for p in range(P)]).reshape(B, P, 3, 3).astype(np.float32)
    tgt1 = (0.7 * np.einsum("bpij,bpnj->bpni", Rgt, src) + np.array([0.1, -0.2, 1.0])).astype(np.float32)
    tgt1 += rng.normal(0, 0.01, tgt1.shape).astype(np.float32)
    s3 = src[:, :, :200].reshape(B * P, 200, 3)
    t3 = tgt1[:, :, :200].reshape(B * P, 200, 3)
    sc, tc = s3 - s3.mean(1, keepdims=True), t3 - t3.mean(1, keepdims=True)
    got = rotate_pts_batch(_dev(sc, device), _dev(tc, device)).cpu().numpy()
    np.testing.assert_allclose(got, g["rot3"], atol=2e-5)
    tc_ref = tc.copy()
    tc_ref[..., 2] *= -1
    got = rotate_pts_batch(_dev(sc, device), _dev(tc_ref, device)).cpu().numpy()
    np.testing.assert_allclose(got, g["rot3_reflect"], atol=2e-5)
    assert np.allclose(np.linalg.det(got), 1.0, atol=1e-5)              # proper rotation even for det(M) < 0


# ---------------------------------------------------------------------------------- backbone
@pytest.mark.parametrize("tag,use_xyz,seed", [("rot", False, 12), ("coord", True, 11)])
def test_backbone_vs_golden_and_oracle(device, tag, use_xyz, seed):
    from captra_amd.backbones import PointNet2Msg
    from captra_amd.configs import make_config
    g = np.load(G / "g56_backbone.npz")
    cfg = make_config("1")
    net = PointNet2Msg(cfg, 128, use_xyz_feat=use_xyz)
    sd = make_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=seed)
    net.load_state_dict(sd)
    net = net.to(device).eval()
    cloud = nocs_batch([0, 1])
    cloud_cn = _dev(cloud.transpose(0, 2, 1), device)
    with torch.no_grad():
        l1_xyz, l1_points = net.sa1(cloud_cn, cloud_cn if use_xyz else None)
        l2_xyz, l2_points = net.sa2(l1_xyz, l1_points)
        _, l3_points = net.sa3(l2_xyz, l2_points)
        out = net(cloud_cn)
    for name, got in (("sa1", l1_points), ("sa2", l2_points), ("sa3", l3_points)):
        np.testing.assert_allclose(got.cpu().numpy(), g[f"{tag}_{name}"], atol=TOL, rtol=0)
    np.testing.assert_allclose(out.cpu().numpy()[:, :, ::8], g[f"{tag}_out"], atol=TOL, rtol=0)
    # and bit-exact against the oracle's exact-arithmetic mode
    ref = OM.backbone({"bb." + k: v for k, v in sd.items()}, "bb", cfg["pointnet"]["camera"],
                      np.ascontiguousarray(cloud.transpose(0, 2, 1)), use_xyz, mlp="exact")
    np.testing.assert_array_equal(out.cpu().numpy(), ref)


@pytest.mark.parametrize("use_xyz,batch", [(False, 1), (True, 2)])
def test_level_scales_in_one_launch_equal_one_launch_each(device, use_xyz, batch):
    """Few clouds: a level's three small-input scales handed over together (captra_sa_scales_multi ->
    sa_wave_lds3_kernel, every scale on its own range of workgroups) against one launch per scale: every bit of the level's
    output, with and without CoordinateNet's coordinate features."""
    from captra_amd import pointnet_utils as PU
    from captra_amd.backbones import PointNet2Msg
    from captra_amd.configs import make_config
    cfg = make_config("1")
    net = PointNet2Msg(cfg, 128, use_xyz_feat=use_xyz)
    net.load_state_dict(make_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=5))
    net = net.to(device).eval()
    cloud_cn = _dev(nocs_batch(list(range(batch))).transpose(0, 2, 1), device)
    outs = {}
    keep = PU.MULTI_SCALE_MAX_CLOUDS
    try:
        for limit in (0, 2):
            PU.MULTI_SCALE_MAX_CLOUDS = limit
            with torch.no_grad():
                l1_xyz, l1 = net.sa1(cloud_cn, cloud_cn if use_xyz else None)
                outs[limit] = (l1.clone(), net.sa2(l1_xyz, l1)[1].clone())        # (level 2: its two scales, sa_wave_pipe2_kernel)
    finally:
        PU.MULTI_SCALE_MAX_CLOUDS = keep
    assert outs[0][0].shape == (batch, 320, 512) and outs[0][1].shape == (batch, 512, 128) and float(outs[0][1].abs().max()) > 0
    assert torch.equal(outs[0][0], outs[2][0]) and torch.equal(outs[0][1], outs[2][1])


def test_sa_scales_multi_from_two_host_threads_concurrently(device):
    """The C ABI holds no state: two host threads, each with its own stream, tensors and job table, call the
    multi-scale path (captra_sa_scales_multi: a level's three small-input scales as one launch, and the second level's two) at
    the same time, many times over, one of them under other per-call options (a pre-zeroed output) -- every result equals the
    thread's own per-scale launches bit for bit."""
    import threading
    from captra_amd import _lib, fused
    rng = np.random.default_rng(99)

    def make(cfeat, shapes, n, m, B):
        xyz_cn = _dev(rng.random((B, 3, n), dtype=np.float32) - 0.5, device)
        feat = _dev(rng.standard_normal((B, cfeat, n)).astype(np.float32), device) if cfeat else None
        new_xyz = _dev(rng.random((B, m, 3), dtype=np.float32) - 0.5, device)
        scales = []
        for chans, k in shapes:
            dims = (cfeat + 3,) + chans
            packed = [fused.pack(_dev((rng.standard_normal((dims[i], dims[i + 1])) / np.sqrt(dims[i])).astype(np.float32), device),
                                 _dev(rng.standard_normal(dims[i + 1]).astype(np.float32), device)) for i in range(3)]
            scales.append((packed, _dev(rng.integers(0, n, (B, m, k)).astype(np.int32), device)))
        return xyz_cn, feat, new_xyz, scales

    work = {0: make(3, [((32, 32, 64), 32), ((64, 64, 128), 64), ((64, 96, 128), 128)], 1024, 128, 2),
            1: make(320, [((128, 128, 256), 64), ((128, 196, 256), 128)], 512, 128, 1)}
    errors, results = [], {}

    def run(tid, together):
        xyz_cn, feat, new_xyz, scales = work[tid]
        ctot = sum(p[-1].cout for p, _ in scales)
        out = torch.zeros(xyz_cn.shape[0], ctot, new_xyz.shape[1], device=device)
        jobs, keep, off = ([] if together else None), [], 0
        with _lib.launch_options(sa_prezeroed=1 if tid == 1 else 0):
            for packed, idx in scales:
                if feat is not None and feat.shape[1] > 3:
                    v1 = fused.sa_first_layer_pre_pm(feat, packed[0])
                    keep.append(v1)
                    fused.sa_scale_pre_pm(v1, xyz_cn, new_xyz, idx, packed, out, off, feat.shape[1], jobs=jobs)
                else:
                    fused.sa_scale_fused(feat, xyz_cn, new_xyz, idx, packed, out, off, jobs=jobs)
                off += packed[-1].cout
            if jobs:
                fused.sa_scales_multi(jobs, device)
        return out

    def worker(tid):
        try:
            with torch.cuda.stream(torch.cuda.Stream(device=device)):
                want = run(tid, False)
                for _ in range(25):
                    got = run(tid, True)
                    torch.cuda.current_stream().synchronize()
                    if not torch.equal(got, want):
                        errors.append((tid, float((got - want).abs().max())))
                results[tid] = True
        except Exception as e:              # noqa: BLE001
            errors.append((tid, repr(e)))

    threads = [threading.Thread(target=worker, args=(t,)) for t in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors and results == {0: True, 1: True}, errors


def test_backbone_16384_point_clouds_bit_exact_vs_oracle(device):
    """BASELINE.json configs[4] shape: S-uni16k clouds (16384 points uniform in a cube), sa1.npoint 2048,
    sa2.npoint 512, radii / nsample / MLPs unchanged.  FPS runs 2047 rounds over 16384 points,
    the ball query scans two LDS tiles, every SA scale has 4x the centres: the backbone output still equals the
    oracle's exact mode bit for bit."""
    import copy
    from captra_amd.backbones import PointNet2Msg
    from captra_amd.configs import make_config
    cfg = copy.deepcopy(make_config("1"))
    cfg["pointnet"]["camera"]["sa1"]["npoint"] = 2048
    cfg["pointnet"]["camera"]["sa2"]["npoint"] = 512
    net = PointNet2Msg(cfg, 128, use_xyz_feat=False)
    sd = make_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=21)
    net.load_state_dict(sd)
    net = net.to(device).eval()
    cloud = np.stack([clouds.s_uni(5, 16384)]).astype(np.float32)              # (1,N,3)
    cloud_cn = np.ascontiguousarray(cloud.transpose(0, 2, 1))
    with torch.no_grad():
        out = net(_dev(cloud_cn, device)).cpu().numpy()
    ref = OM.backbone({"bb." + k: v for k, v in sd.items()}, "bb", cfg["pointnet"]["camera"], cloud_cn, False, mlp="exact")
    assert out.shape == (1, 128, 16384)
    np.testing.assert_array_equal(out, ref)


def test_backbone_train_mode_path_matches_fused(device):
    """The layer-by-layer (autograd) path and the fused eval path agree in eval statistics."""
    from captra_amd.backbones import PointNet2Msg
    from captra_amd.configs import make_config
    cfg = make_config("1")
    net = PointNet2Msg(cfg, 128, use_xyz_feat=True)
    net.load_state_dict(make_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=3))
    net = net.to(device).eval()
    cloud_cn = _dev(nocs_batch([2]).transpose(0, 2, 1), device)
    with torch.no_grad():
        fused_out = net(cloud_cn)
        for m in net.modules():
            m.training = True
        # BatchNorm layers must keep using running statistics for the comparison
        for m in net.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                m.training = False
        layer_out = net(cloud_cn)
    np.testing.assert_allclose(layer_out.cpu().numpy(), fused_out.cpu().numpy(), atol=TOL, rtol=0)


# ------------------------------------------------------------------------------- track loop
SETUPS = {"bottle": ("1", "obj_info_nocs.yml", "nocs", 5), "camera": ("3", "obj_info_nocs.yml", "nocs", 3),
          "drawers": ("drawers", "obj_info_sapien.yml", "arti", 3)}


def _trainer(tag, device):
    from captra_amd.configs import make_config
    from captra_amd.trainer import Trainer
    cat, objcfg, kind, frames = SETUPS[tag]
    cfg = make_config(cat, objcfg, experiment_dir="/tmp/captra_test_exp")
    cfg["track_cfg"]["gt_label"] = (tag == "drawers")
    trainer = Trainer(cfg)
    shapes = {k: tuple(v.shape) for k, v in trainer.model.state_dict().items()}
    assert sorted(shapes) == json.load(open(G / "state_dict_keys.json"))[tag]
    sd = make_state_dict(shapes, seed=7)
    trainer.model.load_state_dict(sd)
    return trainer, cfg, sd, clouds.make_trajectory(kind, 2, frames, seed=0)


def _trainer_physical(tag, device, **cfg_over):
    """The G9p fixture (tests/golden/make_golden_track_physical.py): physical-regime weights, seed-7 trajectories."""
    from captra_amd.configs import make_config
    from captra_amd.trainer import Trainer
    from tests.weights import make_physical_state_dict
    cat, objcfg, kind, frames, batch, wseed, tseed = {**clouds.PHYSICAL_SETUPS, **clouds.PHYSICAL_SETUPS_MORE}[tag]
    cfg = make_config(cat, objcfg, experiment_dir="/tmp/captra_test_exp")
    cfg.update(cfg_over)
    trainer = Trainer(cfg)
    shapes = {k: tuple(v.shape) for k, v in trainer.model.state_dict().items()}
    sd = make_physical_state_dict(shapes, wseed, cfg["num_parts"], bool(cfg["obj_sym"]), kind)
    trainer.model.load_state_dict(sd)
    return trainer, cfg, sd, clouds.make_trajectory(kind, batch, frames, seed=7), tseed


@pytest.mark.parametrize("hipgraph", [False, True])
@pytest.mark.parametrize("tag", ["bottle", "camera", "laptop", "drawers"])
def test_track_loop_vs_golden(device, tag, hipgraph):
    """FREE-RUNNING Trainer.test against the reference's own EvalTrackModel loop (golden G9p): every pose of every frame
    of every trajectory within the 1e-4 contract -- predicted labels, no teacher forcing, no loosened frames; eager
    launches and the captured-hipGraph loop alike."""
    trainer, cfg, sd, data, tseed = _trainer_physical(tag, device, hipgraph=hipgraph)
    trainer.model.use_graph = hipgraph
    g = np.load(G / "g9p_track.npz")
    torch.manual_seed(tseed)
    pred_dict, loss_dict = trainer.test(data, save=False, no_eval=False)
    poses = pred_dict["poses"]
    assert len(poses) == len(data)
    for key in ("rotation", "translation", "scale"):      # initial (noisy) pose: same seed, same draw order as the reference
        np.testing.assert_allclose(poses[0][key].cpu().numpy(), g[f"{tag}_0_{key}"], atol=1e-6, rtol=0)
    for i in range(1, len(poses)):
        for key in ("rotation", "scale", "translation"):
            np.testing.assert_allclose(poses[i][key].cpu().numpy(), g[f"{tag}_{i}_{key}"], atol=TOL, rtol=0,
                                       err_msg=f"{tag} frame {i} {key}")
        lab = torch.argmax(pred_dict["npcs_pred"][i]["seg"], dim=-2)
        counts = [[int((lab[b] == p).sum()) for p in range(cfg["num_parts"])] for b in range(lab.shape[0])]
        np.testing.assert_array_equal(np.asarray(counts), g[f"{tag}_label_counts"][i - 1], err_msg=f"{tag} frame {i} label counts")
    assert "avg_pred" in loss_dict and any(k.startswith("5deg5cm") for k in loss_dict["avg_pred"])


@pytest.mark.parametrize("hipgraph", [False, True])
@pytest.mark.parametrize("tag", ["bowl", "can", "mug", "bottle5"])
def test_track_loop_vs_golden_more(device, tag, hipgraph):
    """The second G9p file: the reference's own free-running loop for the three rigid categories the first
    file lacks, and a FIVE-trajectory bottle batch -- above fused.SPLIT_K_MAX_TRAJECTORIES, so this run takes the large-batch
    kernels (wave-per-centre SA scales, 64x64-tile dense layers, no split-k) that the two-trajectory fixtures do not reach --
    every pose of every frame within 1e-4, eager and captured."""
    from captra_amd import fused
    trainer, cfg, sd, data, tseed = _trainer_physical(tag, device, hipgraph=hipgraph)
    if tag == "bottle5":
        assert len(data[0]["points"]) == 5 > fused.SPLIT_K_MAX_TRAJECTORIES
    trainer.model.use_graph = hipgraph
    g = np.load(G / "g9p_track_more.npz")
    torch.manual_seed(tseed)
    pred_dict, _ = trainer.test(data, save=False, no_eval=True)
    poses = pred_dict["poses"]
    assert len(poses) == len(data)
    for key in ("rotation", "translation", "scale"):
        np.testing.assert_allclose(poses[0][key].cpu().numpy(), g[f"{tag}_0_{key}"], atol=1e-6, rtol=0)
    for i in range(1, len(poses)):
        for key in ("rotation", "scale", "translation"):
            np.testing.assert_allclose(poses[i][key].cpu().numpy(), g[f"{tag}_{i}_{key}"], atol=TOL, rtol=0, err_msg=f"{tag} frame {i} {key}")
        lab = torch.argmax(pred_dict["npcs_pred"][i]["seg"], dim=-2)
        counts = [[int((lab[b] == p).sum()) for p in range(cfg["num_parts"])] for b in range(lab.shape[0])]
        np.testing.assert_array_equal(np.asarray(counts), g[f"{tag}_label_counts"][i - 1], err_msg=f"{tag} frame {i} label counts")


@pytest.mark.parametrize("tag", ["bottle", "camera", "drawers"])
def test_track_first_frame_vs_golden_random_weights(device, tag):
    """Purely random weights (goldens G7 / G9): the seeded initial pose, CoordinateNet's maps and the pose of frame 1.
    (Under random weights the reference's own loop leaves the physical regime after a frame or two -- negative scales on
    the drawers -- and amplifies rounding noise, so the FREE-RUNNING comparison lives on the physical-regime fixture above;
    every later frame of this fixture is held to 1e-4 teacher-forced below.)"""
    trainer, cfg, sd, data = _trainer(tag, device)
    g7, g9 = np.load(G / "g7_step.npz"), np.load(G / "g9_track.npz")
    torch.manual_seed(1234)
    pred_dict, _ = trainer.test(data[:2], save=False, no_eval=True)
    poses = pred_dict["poses"]
    for key in ("rotation", "translation", "scale"):
        np.testing.assert_allclose(poses[0][key].cpu().numpy(), g9[f"{tag}_0_{key}"], atol=1e-6, rtol=0)
    n1 = pred_dict["npcs_pred"][1]
    np.testing.assert_array_equal(torch.argmax(n1["seg"], dim=-2).cpu().numpy(), g7[f"{tag}_labels"].astype(np.int64))
    np.testing.assert_allclose(n1["nocs"].cpu().numpy(), g7[f"{tag}_nocs"], atol=TOL, rtol=0)
    np.testing.assert_allclose(n1["seg"].cpu().numpy(), g7[f"{tag}_seg"], atol=1e-3, rtol=0)
    for key in ("rotation", "scale", "translation"):
        np.testing.assert_allclose(poses[1][key].cpu().numpy(), g9[f"{tag}_1_{key}"], atol=TOL, rtol=1e-4, err_msg=f"{tag} frame 1 {key}")


@pytest.mark.parametrize("tag", ["bottle", "camera", "drawers"])
def test_track_step_teacher_forced_vs_golden_and_oracle(device, tag):
    trainer, cfg, sd, data = _trainer(tag, device)
    g9 = np.load(G / "g9_track.npz")
    model = trainer.model.eval()
    model.set_data(data)
    for i in range(1, len(data)):
        prev = {k: _dev(g9[f"{tag}_{i - 1}_{k}"], device) for k in ("rotation", "translation", "scale")}
        with torch.no_grad():
            _, pose = model.track_step(model.feed_dict[i], model.npcs_feed_dict[i], prev)
        for key in ("rotation", "scale", "translation"):
            np.testing.assert_allclose(pose[key].cpu().numpy(), g9[f"{tag}_{i}_{key}"], atol=TOL, rtol=1e-4,
                                       err_msg=f"{tag} frame {i} {key}")
        # oracle (exact arithmetic) on the same step
        prev_np = {k: g9[f"{tag}_{i - 1}_{k}"] for k in ("rotation", "translation", "scale")}
        gt_labels = data[i]["labels"].numpy() if tag == "drawers" else None
        opose, _ = OM.track_step(sd, cfg, data[i]["points"].numpy(), data[i]["meta"]["points_mean"].numpy(), prev_np, "exact",
                                 gt_labels=gt_labels)
        for key in ("rotation", "scale", "translation"):
            np.testing.assert_allclose(pose[key].cpu().numpy(), opose[key], atol=2e-5, rtol=1e-4, err_msg=f"oracle {key}")


def test_checkpoint_roundtrip_and_coordnet_key_mapping(device, tmp_path):
    """Trainer.save / resume incl. loading a CoordNet experiment under npcs_net.* (trainer.py:159-169)."""
    from captra_amd.configs import make_config
    from captra_amd.trainer import Trainer
    coord_dir, rot_dir = tmp_path / "coord", tmp_path / "rot"
    cfg = make_config("1", experiment_dir=str(rot_dir), **{"coord_exp/dir": str(coord_dir)})
    src = Trainer(cfg)
    sd = make_state_dict({k: tuple(v.shape) for k, v in src.model.state_dict().items()}, seed=5)
    # a CoordNet experiment stores its weights as net.* ; a RotationNet experiment as net.* too
    (coord_dir / "ckpt").mkdir(parents=True)
    (rot_dir / "ckpt").mkdir(parents=True)
    coord_state = {"net" + k[len("npcs_net"):]: v for k, v in sd.items() if k.startswith("npcs_net.")}
    rot_state = {k: v for k, v in sd.items() if k.startswith("net.")}
    torch.save({"epoch": 3, "iteration": 10, "model": coord_state}, coord_dir / "ckpt" / "model_0003.pt")
    torch.save({"epoch": 7, "iteration": 20, "model": rot_state, "optimizer": {}}, rot_dir / "ckpt" / "model_0007.pt")
    dst = Trainer(cfg)
    assert dst.resume() == 7
    for k, v in dst.model.state_dict().items():
        np.testing.assert_array_equal(v.cpu().numpy(), sd[k].numpy(), err_msg=k)


def test_track_cli_matches_trainer_and_writes_result_pickles(device, tmp_path):
    """`python -m captra_amd.track` (counterpart of network/test.py): trajectory .npz files -> resume both experiments
    -> Trainer.test per batch -> the reference's result pickles; its poses equal a direct Trainer.test call."""
    import pickle
    from captra_amd import track
    from captra_amd.configs import make_config
    from captra_amd.trainer import Trainer
    from captra_amd.trajectory_io import save_trajectory_npz
    coord_dir, rot_dir, data_dir = tmp_path / "coord", tmp_path / "rot", tmp_path / "data"
    for d in (coord_dir / "ckpt", rot_dir / "ckpt", data_dir):
        d.mkdir(parents=True)
    # zero pose-perturbation amplitudes: the initial pose is then independent of the RNG state at the draw
    zero_noise = {"pose_perturb/r": 0.0, "pose_perturb/t": 0.0, "pose_perturb/s": 0.0}
    cfg = make_config("1", experiment_dir=str(rot_dir), **{"coord_exp/dir": str(coord_dir)}, **zero_noise)
    src = Trainer(cfg)
    sd = make_state_dict({k: tuple(v.shape) for k, v in src.model.state_dict().items()}, seed=9)
    torch.save({"epoch": 1, "iteration": 1, "model": {"net" + k[len("npcs_net"):]: v for k, v in sd.items() if k.startswith("npcs_net.")}},
               coord_dir / "ckpt" / "model_0001.pt")
    torch.save({"epoch": 2, "iteration": 1, "model": {k: v for k, v in sd.items() if k.startswith("net.")}},
               rot_dir / "ckpt" / "model_0002.pt")
    frames = clouds.make_trajectory("nocs", 2, 4, seed=3)
    for b in range(2):
        save_trajectory_npz(str(data_dir / f"traj{b}.npz"), frames, b)
    torch.manual_seed(0)
    np.random.seed(0)
    res = track.main(["--obj_category", "1", "--experiment_dir", str(rot_dir), "--coord_exp/dir", str(coord_dir),
                      "--batch_size", "2", "--data", str(data_dir), "--save", "--hipgraph",
                      "--pose_perturb/r", "0", "--pose_perturb/t", "0", "--pose_perturb/s", "0"])
    assert res["frames"] == 8 and any(k.startswith("avg_pred/") for k in res["loss"]), res
    out = sorted((rot_dir / "results" / "data").glob("*.pkl"))
    assert len(out) == 2
    # the same trajectories through Trainer.test directly (same seeds -> same initial pose noise)
    ref = Trainer(cfg)
    ref.resume()
    torch.manual_seed(0)
    np.random.seed(0)
    pred, _ = ref.test(clouds.make_trajectory("nocs", 2, 4, seed=3))
    with open(out[0], "rb") as fh:
        saved = pickle.load(fh)
    assert set(saved) == {"pred", "gt", "frame_nums"} and len(saved["pred"]["poses"]) == 4
    for i in range(4):
        for key in ("rotation", "translation", "scale"):
            np.testing.assert_array_equal(np.asarray(saved["pred"]["poses"][i][key]).reshape(-1),
                                          pred["poses"][i][key][0].cpu().numpy().reshape(-1))


@pytest.mark.parametrize("sym,P", [(True, 1), (False, 1), (False, 4), (True, 3)])
def test_rot_pool_compose_vs_reference_algebra(device, sym, P):
    """The one-launch rotation read-out equals the reference's op sequence (per-point normalise / ortho6d, masked mean
    with default, from_3d / Gram-Schmidt, diagonal pick, R_prev @ dR) evaluated with the package's torch mirrors of
    rotations.py / part_dof_utils.py; a part without points takes the default; degenerate per-point vectors are included."""
    from captra_amd import fused
    from captra_amd.pose_utils.part_dof_utils import convert_pred_rtvec_to_matrix
    from captra_amd.pose_utils.rotations import compute_rotation_matrix_from_ortho6d, normalize_vector
    rng = np.random.default_rng(17 + P + int(sym))
    B, N, R = 3, 1000, (3 if sym else 6)
    raw = rng.standard_normal((B * P, P, R, N)).astype(np.float32)
    raw[0, 0, :, :5] = 0.0                                      # |v| = 0: the (1,0,0) fallback of normalize_vector
    labels = rng.integers(0, P + 1, (B, N)).astype(np.int32)    # label P = background
    if P > 1:
        labels[1][labels[1] == P - 1] = P                       # trajectory 1: last part has no points
    prev = np.stack([clouds._rot_y(0.3 * i) @ clouds._rot_x(0.1 * i) for i in range(B * P)]).reshape(B, P, 3, 3).astype(np.float32)
    rot, delta = fused.rot_pool_compose(_dev(raw, device), _dev(labels, device), _dev(prev, device), sym, want_delta=True)
    # the diagonal-only layout (head p on cloud (b,p)) gives the same read-out
    diag = np.ascontiguousarray(raw.reshape(B, P, P, R, N)[:, np.arange(P), np.arange(P)].reshape(B * P, R, N))
    rot_d, delta_d = fused.rot_pool_compose(_dev(diag, device), _dev(labels, device), _dev(prev, device), sym, want_delta=True)
    assert torch.equal(rot, rot_d) and torch.equal(delta, delta_d)
    # reference sequence on the CPU
    t = torch.from_numpy(raw).transpose(-1, -2)                 # (Q,P,N,R)
    if sym:
        per_point = normalize_vector(t.reshape(-1, 3)).reshape(t.shape).transpose(-1, -2)
    else:
        per_point = compute_rotation_matrix_from_ortho6d(t.reshape(-1, 6)).reshape(t.shape[:-1] + (9,)).transpose(-1, -2)
    lab = torch.from_numpy(labels).long().unsqueeze(1).expand(-1, P, -1).reshape(B * P, -1)
    mask = (lab.unsqueeze(1) == torch.arange(P).view(1, P, 1)).float().unsqueeze(-2)
    valid = (mask.sum(dim=(-1, -2)) > 0).float().unsqueeze(-1)
    pooled = (per_point * mask).sum(-1) / torch.clamp_min(mask.sum(-1), 1.0)
    default = (torch.tensor((0.0, 1.0, 0.0)) if sym else torch.eye(3).reshape(-1)).reshape(1, 1, -1)
    pooled = valid * pooled + (1.0 - valid) * default
    d_all = convert_pred_rtvec_to_matrix(pooled, sym).reshape(B, P, P, 3, 3)
    idx = torch.arange(P)
    d_ref = d_all[:, idx, idx]
    r_ref = torch.matmul(torch.from_numpy(prev), d_ref)
    np.testing.assert_allclose(delta.cpu().numpy(), d_ref.numpy(), atol=2e-6, rtol=0)
    np.testing.assert_allclose(rot.cpu().numpy(), r_ref.numpy(), atol=2e-6, rtol=0)


@pytest.mark.parametrize("sym,P", [(True, 1), (False, 1), (False, 4), (True, 3)])
def test_rot_pool_compose_vs_oracle(device, sym, P):
    """The one-launch rotation read-out against the ORACLE's restatement of the reference (oracle/model.py rot_pool_compose:
    networks.py:127-138, rotations.py:302-387, part_dof_utils.py:124-141 -- the function the oracle's track_step runs, pinned to the
    reference's poses by goldens G9 / G9p), not against this package's own mirrors: empty parts (default axis / identity),
    zero-length per-point vectors ((1,0,0) fallback), parallel ortho6d columns, background labels, one to four parts."""
    from captra_amd import fused
    rng = np.random.default_rng(170 + P + int(sym))
    B, N, R = 4, 1500, (3 if sym else 6)
    raw = rng.standard_normal((B, P, R, N)).astype(np.float32)
    raw[0, 0, :, :7] = 0.0                                       # |v| = 0
    if not sym:
        raw[1, 0, 3:6, 7:12] = 2.5 * raw[1, 0, 0:3, 7:12]       # second ortho6d column parallel to the first: cross product 0
    labels = rng.integers(0, P + 1, (B, N)).astype(np.int32)     # label P = background
    if P > 1:
        labels[1][labels[1] == P - 1] = P                        # trajectory 1: the last part has no points
    labels[2][:] = P                                             # trajectory 2: every part empty
    prev = np.stack([clouds._rot_y(0.3 * i) @ clouds._rot_x(0.1 * i) for i in range(B * P)]).reshape(B, P, 3, 3).astype(np.float32)
    rot, delta = fused.rot_pool_compose(_dev(np.ascontiguousarray(raw.reshape(B * P, R, N)), device), _dev(labels, device), _dev(prev, device),
                                        sym, want_delta=True)
    r_ref, d_ref = OM.rot_pool_compose(raw, labels, prev, sym)
    np.testing.assert_allclose(delta.cpu().numpy(), d_ref, atol=2e-6, rtol=0)
    np.testing.assert_allclose(rot.cpu().numpy(), r_ref, atol=2e-6, rtol=0)
    assert np.array_equal(d_ref[2], np.broadcast_to(np.eye(3, dtype=np.float32), (P, 3, 3)))       # (all parts empty: the default is the identity either way)


@pytest.mark.parametrize("b,cin,cout,l,csplit,bcast,act", [(1, 515, 256, 128, 3, False, 1), (2, 1536, 512, 128, 512, True, 1), (1, 832, 512, 512, 320, False, 1),
                                                          (1, 256, 512, 128, 0, False, 1), (2, 320, 128, 512, 0, False, 0), (1, 130, 70, 77, 0, False, 2)])
def test_split_k_dense_layers_close_to_the_bit_exact_chain(device, b, cin, cout, l, csplit, bcast, act):
    """fused.split_k (captra_launch_opts::splitk_positions): the dense layers of few-position launches with k dealt to a workgroup's four waves and
    the partial tiles added in wave order -- within 1e-5 of the k-ascending chain (relative to the largest output), for the one-
    and two-source layers of the 128- / 512-point levels (SA3's [xyz, feat], FP3's [points1, repeat(points2)], FP2's concat, SA2's
    point-major pre-transform), odd shapes included; outside the context, and for launches above the position limit inside it,
    the chain itself (bit-identical)."""
    from captra_amd import fused, _lib as L
    g = torch.Generator().manual_seed(cin + cout + l)
    lin = fused.pack((torch.randn(cin, cout, generator=g) / cin ** 0.5).to(device), torch.randn(cout, generator=g).to(device))
    if csplit:
        n1, n2 = b * csplit * l, b * (cin - csplit) * (1 if bcast else l)
        flat = torch.randn(n1 + n2, generator=g).to(device)          # (one allocation: the two sources within one buffer descriptor's reach)
        x1, x2 = flat[:n1].view(b, csplit, l), flat[n1:].view(b, cin - csplit, 1 if bcast else l)
        run = lambda: fused.pointwise_mlp2(x1, x2, lin, act)
    else:
        x = torch.randn(b, cin, l, generator=g).to(device)
        run = lambda: fused.pointwise_mlp(x, lin, act)
    ref = run()
    if ref is None:       # (pointwise_mlp2 declines when the allocator placed its two tensors more than 2^30 bytes apart: the caller concatenates)
        pytest.skip("the two source tensors lie too far apart for one buffer descriptor in this process")
    with fused.split_k(True):
        got = run()
        big = fused.pointwise_mlp(torch.randn(3, cin, 512, generator=g).to(device), lin, act) if not csplit else None    # 1536 positions: above the limit
    again = run()
    assert torch.equal(again, ref)
    scale = float(ref.abs().max())
    assert float((got - ref).abs().max()) <= 1e-5 * max(scale, 1.0)
    assert not torch.equal(got, ref) or cin < 256          # (it IS another summation order)
    if big is not None:
        assert big.shape == (3, cout, 512)
    if not csplit and cout % 4 == 0:                        # the point-major form (SA2's pre-transformed first layer)
        out_ref = torch.empty(b, l, cout, device=device)
        out_got = torch.empty(b, l, cout, device=device)
        with torch.cuda.device(device):
            L.call("captra_pointwise_mlp_pm", b, cin, cout, l, L.ptr(x), L.ptr(lin.wt), L.ptr(lin.bias), 0, L.ptr(out_ref))
            with fused.split_k(True):
                L.call("captra_pointwise_mlp_pm", b, cin, cout, l, L.ptr(x), L.ptr(lin.wt), L.ptr(lin.bias), 0, L.ptr(out_got))
        assert float((out_got - out_ref).abs().max()) <= 1e-5 * max(float(out_ref.abs().max()), 1.0)


def test_split_k_head_output_layer(device):
    """A head's last layer (256 -> 3, GroupNorm + ReLU on load, no statistics) in the split-k form against the chain form: 1e-5."""
    from captra_amd import fused
    g = torch.Generator().manual_seed(9)
    x = torch.randn(1, 256, 4096, generator=g).to(device)
    lin = fused.pack((torch.randn(256, 3, generator=g) / 16).to(device), torch.randn(3, generator=g).to(device))
    ab = torch.stack([torch.rand(1, 256, generator=g) + 0.5, torch.randn(1, 256, generator=g) * 0.3], -1).to(device).contiguous()
    ref = fused.pointwise_mlp_gn(x, lin, ab, fused.ACT_NONE, False)
    with fused.split_k(True):
        got = fused.pointwise_mlp_gn(x, lin, ab, fused.ACT_NONE, False)
    assert got.shape == ref.shape == (1, 3, 4096) and not torch.equal(got, ref)
    assert float((got - ref).abs().max()) <= 1e-5 * max(float(ref.abs().max()), 1.0)


@pytest.mark.parametrize("cin,cout,l,batch,with_ab", [(128, 512, 4096, 1, False), (512, 256, 4096, 1, True), (512, 512, 1000, 2, True), (130, 96, 75, 3, False)])
def test_split_k_gn_chain_layers(device, cin, cout, l, batch, with_ab):
    """The GroupNorm-chain layers (relu(a x + b) on load, raw-output statistics per 32-column tile) in the split-k form against the
    chain form of the same launch shape: y within 1e-5, the (sum, sum of squares) partials within 1e-5 of the tile's absolute sum --
    ragged tails and an odd number of 32-column tiles included (the table's padding tile is written, as zeros)."""
    from captra_amd import fused
    g = torch.Generator().manual_seed(cin + cout + l)
    x = torch.randn(batch, cin, l, generator=g).to(device)
    lin = fused.pack((torch.randn(cin, cout, generator=g) / cin ** 0.5).to(device), torch.randn(cout, generator=g).to(device))
    ab = torch.stack([torch.rand(batch, cin, generator=g) + 0.5, torch.randn(batch, cin, generator=g) * 0.3], -1).to(device).contiguous() if with_ab else None
    y0, s0 = fused.pointwise_mlp_gn(x, lin, ab, fused.ACT_NONE, True)
    with fused.split_k(True):
        s_probe = torch.full_like(s0, float("nan"))
        y1, s1 = fused.pointwise_mlp_gn(x, lin, ab, fused.ACT_NONE, True)
        y2 = fused.pointwise_mlp_gn(x, lin, ab, fused.ACT_RELU, False)
    assert s1.shape == s0.shape and not torch.isnan(s1).any()
    scale = max(float(y0.abs().max()), 1.0)
    assert float((y1 - y0).abs().max()) <= 1e-5 * scale and float((y2 - torch.relu(y0)).abs().max()) <= 1e-5 * scale
    t = s0.shape[2]
    yd = torch.zeros(batch, cout, t * 32, dtype=torch.float64, device=device)
    yd[:, :, :l] = y1.double()
    yt = yd.reshape(batch, cout, t, 32)
    want = torch.stack([yt.sum(-1), (yt * yt).sum(-1)], -1)
    err = (s1.double() - want).abs()
    assert float(err[..., 0].max()) <= 1e-5 * max(float(yt.abs().sum(-1).max()), 1.0) and float(err[..., 1].max()) <= 1e-5 * max(float(want[..., 1].max()), 1.0)


@pytest.mark.parametrize("cin,cout,l,batch,with_ab", [(128, 512, 4096, 5, False), (512, 256, 4096, 9, True), (128, 512, 4032, 5, False), (64, 128, 1030, 64, True)])
def test_gn_chain_layer_statistics_epilogue_on_64x64_tiles(device, cin, cout, l, batch, with_ab):
    """captra_pointwise_mlp_gn at launch shapes that take the 64x64 wave tiles (>= 2048 of them; the rotation heads at >= 4 clouds): y is
    the plain layer's y bit for bit (the operand's relu(a x + b) formed by torch where coefficients are given), and the epilogue's
    per-(row, 64-column tile) partials (transposing DPP reduction on whole tiles, the butterfly on ragged ones) are the sums of that
    y to summation-order rounding."""
    from captra_amd import fused
    g = torch.Generator().manual_seed(cin + cout + l)
    x = torch.randn(batch, cin, l, generator=g).to(device)
    lin = fused.pack((torch.randn(cin, cout, generator=g) / cin ** 0.5).to(device), torch.randn(cout, generator=g).to(device))
    ab = torch.stack([torch.rand(batch, cin, generator=g) + 0.5, torch.randn(batch, cin, generator=g) * 0.3], -1).to(device).contiguous() if with_ab else None
    y, stats = fused.pointwise_mlp_gn(x, lin, ab, fused.ACT_NONE, True)
    xin = torch.relu(ab[:, :, :1] * x + ab[:, :, 1:]) if with_ab else x
    ref = fused.pointwise_mlp(xin.contiguous(), lin, fused.ACT_NONE)
    t = stats.shape[2]
    assert t == (l + 127) // 128 * 2
    if with_ab:       # (the kernel's fmaf(a, x, b) against torch's separately rounded a x + b: operands differ by an ulp)
        np.testing.assert_allclose(y.cpu().numpy(), ref.cpu().numpy(), atol=2e-5 * float(ref.abs().max()), rtol=0)
    else:
        assert torch.equal(y, ref)
    yd = torch.zeros(batch, cout, t * 64, dtype=torch.float64, device=device)
    yd[:, :, :l] = y.double()
    yt = yd.reshape(batch, cout, t, 64)
    want = torch.stack([yt.sum(-1), (yt * yt).sum(-1)], -1)
    err = (stats.double() - want).abs()
    assert float(err[..., 0].max()) <= 1e-5 * float(yt.abs().sum(-1).max()) and float(err[..., 1].max()) <= 1e-5 * float(want[..., 1].max())


@pytest.mark.parametrize("n,batch", [(4096, 3), (1000, 3), (4096, 1), (520, 2), (4096, 5)])
def test_group_norm_chain_fused_vs_separate_and_torch(device, n, batch):
    """Rotation-head MLP (Conv -> GroupNorm(C/2 groups) -> ReLU x3 -> Conv): statistics emitted by the conv epilogue and
    the normalisation applied in the next conv's operand load == the separate GroupNorm kernel == torch, to rounding."""
    from captra_amd import fused
    from captra_amd.blocks import MLPConv1d
    torch.manual_seed(3)
    head = MLPConv1d(128, [512, 512, 256, 3], bn=True, gn=True, last_activation="none").eval()
    with torch.no_grad():
        for m in head.modules():
            if isinstance(m, torch.nn.GroupNorm):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.3, 0.3)
    x = torch.randn(batch, 128, n)                      # small batches take the 32x32-tile variant (32-position statistics)
    with torch.no_grad():
        ref = head(x)                                   # CPU: plain torch modules
        head_gpu = head.to(device)
        got = head_gpu(x.to(device)).cpu()
        fused.USE_GN_FUSED = False
        try:
            head_gpu._cache = {}
            sep = head_gpu(x.to(device)).cpu()
        finally:
            fused.USE_GN_FUSED = True
    scale = float(ref.abs().max())
    np.testing.assert_allclose(got.numpy(), sep.numpy(), atol=2e-5 * scale, rtol=0)
    np.testing.assert_allclose(got.numpy(), ref.numpy(), atol=1e-4 * scale, rtol=0)


# ------------------------------------------------------------------------------- bf16 operand mode (configs[2])
def _bf16_round(a):
    """Round-to-nearest-even fp32 -> bf16 -> fp32 (numpy)."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def _bf16_layer(x, w, b, act):
    """act(b + sum_k bf16(w[k]) bf16(x[k])) with wide accumulation: the contract of the bf16 kernels up to fp32 summation order."""
    y = np.einsum("kc,bk...->bc...", _bf16_round(w).astype(np.float64), _bf16_round(x).astype(np.float64)) + b.reshape((1, -1) + (1,) * (x.ndim - 2))
    y = y.astype(np.float32)
    return np.maximum(y, 0) if act == 1 else y


@pytest.mark.parametrize("cin,cout,l", [(128, 512, 4096), (515, 256, 128), (134, 128, 1000), (256, 3, 4096), (320, 128, 512), (7, 40, 77)])
def test_bf16_dense_layer(device, cin, cout, l):
    from captra_amd import fused
    rng = np.random.default_rng(cin + cout + l)
    x = rng.standard_normal((2, cin, l)).astype(np.float32)
    w = (rng.standard_normal((cin, cout)) / np.sqrt(cin)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    fused.set_mlp_dtype("bf16")
    try:
        got = fused.pointwise_mlp(_dev(x, device), fused.pack(_dev(w, device), _dev(b, device)), 1).cpu().numpy()
    finally:
        fused.set_mlp_dtype("fp32")
    ref = _bf16_layer(x, w, b, 1)
    np.testing.assert_allclose(got, ref, atol=2e-5 * max(1.0, float(np.abs(ref).max())), rtol=0)


@pytest.mark.parametrize("cfeat,chans,n,m,k", [(3, (64, 96, 128), 4096, 512, 128), (0, (32, 32, 64), 700, 41, 32),
                                                (320, (128, 196, 256), 512, 128, 128), (320, (128, 128, 256), 200, 5, 64)])
def test_bf16_sa_scale(device, cfeat, chans, n, m, k):
    """bf16-operand SA scale against the same layer contract evaluated layer by layer in numpy; an occasional element whose
    fp32 pre-activation sits on a bf16 rounding boundary may round the other way (accumulation order), hence the two bounds."""
    from captra_amd import fused
    rng = np.random.default_rng(cfeat + sum(chans) + k)
    B = 2
    xyz_cn = (rng.random((B, 3, n), dtype=np.float32) - 0.5)
    feat = rng.standard_normal((B, cfeat, n)).astype(np.float32) if cfeat else None
    new_xyz = (rng.random((B, m, 3), dtype=np.float32) - 0.5)
    idx = rng.integers(0, n, (B, m, k)).astype(np.int32)
    dims = (cfeat + 3,) + chans
    layers = [((rng.standard_normal((dims[i], dims[i + 1])) / np.sqrt(dims[i])).astype(np.float32),
               rng.standard_normal(dims[i + 1]).astype(np.float32)) for i in range(3)]
    packed = [fused.pack(_dev(w, device), _dev(b, device)) for w, b in layers]
    out = torch.zeros(B, chans[2], m, device=device)
    fused.set_mlp_dtype("bf16")
    try:
        assert fused.sa_scale_bf16_supported(cfeat, packed, k)
        fused.sa_scale_bf16(None if feat is None else _dev(feat, device), _dev(xyz_cn, device), _dev(new_xyz, device),
                            _dev(idx, device), packed, out, 0)
    finally:
        fused.set_mlp_dtype("fp32")
    x = O.sa_group(feat, xyz_cn, new_xyz, idx)
    for w, b in layers:
        x = _bf16_layer(x, w, b, 1)
    ref = x.max(axis=-1)
    got = out.cpu().numpy()
    scale = float(np.abs(ref).max())
    err = np.abs(got - ref)
    assert err.max() <= 3e-2 * scale, err.max() / scale          # a flipped bf16 rounding upstream: <= 2^-8 relative per flip
    assert np.mean(err) <= 2e-4 * scale, np.mean(err) / scale    # typical elements agree to accumulation-order noise


@pytest.mark.parametrize("cfeat,chans,n,m,k,b", [(3, (64, 96, 128), 4096, 512, 128, 2), (0, (32, 32, 64), 700, 41, 32, 3), (3, (64, 64, 128), 900, 67, 64, 2),
                                                  (0, (64, 96, 128), 1000, 9, 128, 1), (320, (128, 196, 256), 512, 128, 128, 2),
                                                  (320, (128, 128, 256), 200, 5, 64, 3), (320, (128, 128, 256), 512, 128, 64, 2)])
def test_bf16_sa_scale_forms_bit_identical(device, cfeat, chans, n, m, k, b):
    """The launch forms of captra_sa_scale_bf16 (small-input scales: gather of the next pass prefetched or not, weight fragments
    through a ring or not; SA2 scales: sa_bf16_kernel or the two-accumulator-group kernel with the read-outs under the MFMAs) run
    the same MFMA sequence per position: identical bits."""
    import ctypes
    from captra_amd import _lib, fused
    rng = np.random.default_rng(7 * cfeat + sum(chans) + k + m)
    xyz_cn = _dev(rng.random((b, 3, n), dtype=np.float32) - 0.5, device)
    feat = _dev(rng.standard_normal((b, cfeat, n)).astype(np.float32), device) if cfeat else None
    new_xyz = _dev(rng.random((b, m, 3), dtype=np.float32) - 0.5, device)
    idx = _dev(rng.integers(0, n, (b, m, k)).astype(np.int32), device)
    dims = (cfeat + 3,) + chans
    packed = [fused.pack(_dev((rng.standard_normal((dims[i], dims[i + 1])) / np.sqrt(dims[i])).astype(np.float32), device),
                         _dev(rng.standard_normal(dims[i + 1]).astype(np.float32), device)) for i in range(3)]
    outs = {}
    fused.set_mlp_dtype("bf16")
    try:
        for variant in (9, 0):
            _lib.lib().captra_sa_bf16_set_variant(ctypes.c_int(variant))
            out = torch.full((b, chans[2], m), -7.0, device=device)
            fused.sa_scale_bf16(feat, xyz_cn, new_xyz, idx, packed, out, 0)
            outs[variant] = out
    finally:
        _lib.lib().captra_sa_bf16_set_variant(ctypes.c_int(0))
        fused.set_mlp_dtype("fp32")
    assert torch.equal(outs[9], outs[0])


_SLOT_PERM = np.array([0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15])


def _pm_to_dense(t, c):
    """(B,L,ceil32(c)) bf16 slot-order tensor (include/captra_hip.h "bf16-NATIVE dense layers") -> (B,c,L) float32."""
    a = t.float().cpu().numpy()
    B, L, cp = a.shape
    a = a.reshape(B, L, cp // 16, 16)
    nat = np.empty_like(a)
    nat[..., _SLOT_PERM] = a                      # memory slot s holds channel perm[s] of its block of 16
    nat = nat.reshape(B, L, cp)
    assert not nat[:, :, c:].any(), "padding channels of a point-major tensor are zero"
    return np.ascontiguousarray(nat[:, :, :c].transpose(0, 2, 1))


def _dense_to_pm(x):
    """(B,c,L) float32 (bf16-representable values) -> the (B,L,ceil32(c)) bf16 slot-order tensor."""
    B, c, L = x.shape
    cp = (c + 31) // 32 * 32
    nat = np.zeros((B, L, cp), np.float32)
    nat[:, :, :c] = x.transpose(0, 2, 1)
    nat = nat.reshape(B, L, cp // 16, 16)
    return torch.from_numpy(np.ascontiguousarray(nat[..., _SLOT_PERM]).reshape(B, L, cp)).to(torch.bfloat16)


@pytest.mark.parametrize("cin,cout,l", [(128, 512, 4096), (512, 512, 1000), (512, 256, 333), (256, 3, 4096), (40, 70, 77)])
def test_bf16pm_dense_layer_layouts_and_groupnorm_on_load(device, cin, cout, l):
    """The bf16-native dense kernel (csrc/dense_bf16.hip) in its four layout combinations, with and without the on-load
    GroupNorm, against act(b + sum_k bf16(w) bf16(x)) in float64; the statistics kernel against numpy sums of the stored tensor."""
    from captra_amd import fused
    rng = np.random.default_rng(cin * 7 + cout + l)
    B = 2
    x = _bf16_round(rng.standard_normal((B, cin, l)).astype(np.float32))
    w = (rng.standard_normal((cin, cout)) / np.sqrt(cin)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    lin = fused.pack(_dev(w, device), _dev(b, device))
    ref = _bf16_layer(x, w, b, 0)
    tol = 2e-5 * max(1.0, float(np.abs(ref).max()))
    xpm = _dense_to_pm(x).to(device)
    # fp32 channel-major in -> fp32 out / bf16 point-major out
    y = fused.pointwise_mlp_bf16pm(_dev(x, device), lin, l, in_pm=False, out_pm=False).cpu().numpy()
    np.testing.assert_allclose(y, ref, atol=tol, rtol=0)
    ypm = fused.pointwise_mlp_bf16pm(_dev(x, device), lin, l, in_pm=False, out_pm=True)
    got = _pm_to_dense(ypm, cout)
    assert np.abs(got - _bf16_round(ref)).max() <= 2.0 ** -7 * np.abs(ref).max()          # one bf16 ulp of slack on rounding ties
    assert np.mean(got == _bf16_round(ref)) > 0.995
    # point-major in -> both outputs, plain
    y2 = fused.pointwise_mlp_bf16pm(xpm, lin, l, in_pm=True, out_pm=False).cpu().numpy()
    np.testing.assert_allclose(y2, ref, atol=tol, rtol=0)
    y2r = fused.pointwise_mlp_bf16pm(xpm, lin, l, in_pm=True, out_pm=True, act=fused.ACT_RELU)
    assert np.mean(_pm_to_dense(y2r, cout) == _bf16_round(np.maximum(ref, 0))) > 0.995
    # statistics of the stored tensor
    stats = fused.gn_stats_bf16pm(xpm, cin).cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(stats[..., 0].sum(-1), x.astype(np.float64).sum(-1), atol=1e-3 * np.sqrt(l), rtol=1e-5)
    np.testing.assert_allclose(stats[..., 1].sum(-1), (x.astype(np.float64) ** 2).sum(-1), rtol=2e-5)
    # the same statistics left by the producing layer's own epilogue (chunks of 64 positions, fixed order): of what it STORED,
    # and the stored tensor bit-identical to the plain launch's
    for src, in_pm in ((_dev(x, device), False), (xpm, True)):
        ys, st = fused.pointwise_mlp_bf16pm(src, lin, l, in_pm=in_pm, out_pm=True, with_stats=True)
        plain = fused.pointwise_mlp_bf16pm(src, lin, l, in_pm=in_pm, out_pm=True)
        assert torch.equal(ys.view(torch.int16), plain.view(torch.int16))
        stored = _pm_to_dense(ys, cout).astype(np.float64)
        st = st.cpu().numpy().astype(np.float64)
        assert st.shape == (B, (l + 63) // 64, cout, 2)                                     # tile-major
        for t in range(st.shape[1]):
            seg = stored[:, :, 64 * t:64 * t + 64]
            np.testing.assert_allclose(st[:, t, :, 0], seg.sum(-1), atol=1e-4 * max(1.0, np.abs(seg).max()), rtol=1e-5)
            np.testing.assert_allclose(st[:, t, :, 1], (seg ** 2).sum(-1), atol=1e-6, rtol=1e-5)
        st2 = fused.pointwise_mlp_bf16pm(src, lin, l, in_pm=in_pm, out_pm=True, with_stats=True)[1]
        assert torch.equal(st2.cpu(), torch.from_numpy(st.astype(np.float32)))              # no atomics: run-to-run identical
    # on-load GroupNorm: x -> bf16(relu(a x + b))
    ab = rng.standard_normal((B, cin, 2)).astype(np.float32)
    xn = _bf16_round(np.maximum(np.float32(ab[:, :, 0:1]) * x + np.float32(ab[:, :, 1:2]), 0).astype(np.float32))
    refn = _bf16_layer(xn, w, b, 0)
    y3 = fused.pointwise_mlp_bf16pm(xpm, lin, l, in_pm=True, out_pm=False, ab=_dev(ab, device)).cpu().numpy()
    err = np.abs(y3 - refn)
    scale = max(1.0, float(np.abs(refn).max()))
    assert err.max() <= 2e-2 * scale and err.mean() <= 1e-4 * scale, (err.max() / scale, err.mean() / scale)   # fma vs mul+add on a rounding tie
    # ... and with the statistics epilogue (the shared-operand kernel for the wide layers): same stored tensor, its sums
    y4, st4 = fused.pointwise_mlp_bf16pm(xpm, lin, l, in_pm=True, out_pm=True, ab=_dev(ab, device), with_stats=True)
    assert torch.equal(y4.view(torch.int16), fused.pointwise_mlp_bf16pm(xpm, lin, l, in_pm=True, out_pm=True, ab=_dev(ab, device)).view(torch.int16))
    stored = _pm_to_dense(y4, cout).astype(np.float64)
    st4 = st4.cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(st4[..., 0].sum(1), stored.sum(-1), atol=1e-3 * max(1.0, np.abs(stored).max()), rtol=1e-5)
    np.testing.assert_allclose(st4[..., 1].sum(1), (stored ** 2).sum(-1), atol=1e-6, rtol=2e-5)


def test_bf16_feature_propagation_from_one_vector_per_cloud_and_row_max(device):
    """bf16 mode, FP3 (S == 1: pointnet_utils.py:265-268 repeats the pooled vector to every point and concatenates): the fused path
    never builds the concat -- W [x; v 1^T] + b = W1 x + (W2 v + b), the bracket as a per-cloud bias
    (captra_pointwise_mlp_bf16pm_cb) -- against the float64 evaluation of the module's own layers on bf16-rounded operands;
    and captra_row_max (the group_all pooling in this mode) against torch.max."""
    from captra_amd import fused
    from captra_amd.pointnet_utils import PointNetFeaturePropagation
    torch.manual_seed(5)
    B, C1, C2, N = 3, 512, 1024, 128
    fp = PointNetFeaturePropagation(in_channel=C1 + C2, mlp=[256, 256]).to(device).eval()
    with torch.no_grad():
        for bn in fp.mlp_bns:
            bn.running_mean.normal_(0, 0.1)
            bn.running_var.uniform_(0.5, 1.5)
    xyz1, xyz2 = torch.randn(B, 3, N, device=device), torch.zeros(B, 3, 1, device=device)
    p1, p2 = torch.randn(B, C1, N, device=device), torch.randn(B, C2, 1, device=device).abs()
    with torch.no_grad():
        ref = fp(xyz1, xyz2, p1, p2)                                   # exact fp32 mode (fused kernels)
        with fused.use_mlp_dtype("bf16"):
            got = fp(xyz1, xyz2, p1, p2)
    assert got.shape == ref.shape == (B, 256, N) and got.dtype == torch.float32
    d = (got - ref).abs()
    scale = float(ref.abs().max())
    assert float(d.max()) <= 3e-2 * scale and float(d.mean()) <= 4e-3 * scale, (float(d.max()) / scale, float(d.mean()) / scale)
    # the per-cloud-bias layer alone, against act(bias[b] + sum_k bf16(w) bf16(x)) in float64
    rng = np.random.default_rng(9)
    x = _bf16_round(rng.standard_normal((B, 96, 77)).astype(np.float32))
    w = (rng.standard_normal((96, 64)) / 10).astype(np.float32)
    bias = rng.standard_normal((B, 64)).astype(np.float32)
    lin = fused.pack(_dev(w, device), _dev(np.zeros(64, np.float32), device))
    y = fused.pointwise_mlp_bf16pm_cloud_bias(_dev(x, device), lin, 77, _dev(bias, device), out_pm=False, act=fused.ACT_RELU).cpu().numpy()
    want = np.maximum(np.einsum("kc,bkl->bcl", _bf16_round(w).astype(np.float64), x.astype(np.float64)) + bias[:, :, None], 0)
    np.testing.assert_allclose(y, want, atol=2e-5 * max(1.0, np.abs(want).max()), rtol=0)
    # row max
    for shape in [(2, 1024, 128), (3, 7, 130), (1, 5, 1)]:
        t = torch.randn(*shape, device=device)
        assert torch.equal(fused.row_max(t), t.max(dim=2, keepdim=True)[0])


def test_bf16_rotation_head_chain_vs_torch(device):
    """MLPConv1d(128 -> 512 -> 512 -> 256 -> 3, GroupNorm) in the bf16 mode (hidden activations bf16 point-major in HBM, GroupNorm on
    load) against the torch fp32 Sequential: bf16-level agreement on the head's raw output."""
    from captra_amd import fused
    from captra_amd.blocks import MLPConv1d
    torch.manual_seed(3)
    head = MLPConv1d(128, [512, 512, 256, 3], bn=True, gn=True, last_activation="none").to(device).eval()
    with torch.no_grad():
        for m in head.model:
            if isinstance(m, torch.nn.GroupNorm):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.3, 0.3)
    x = torch.randn(3, 128, 1000, device=device)
    with torch.no_grad():
        ref = head.model(x)
        with fused.use_mlp_dtype("bf16"):
            got = head(x)
    assert got.shape == ref.shape and got.dtype == torch.float32
    d = (got - ref).abs()
    scale = float(ref.abs().max())
    assert float(d.max()) <= 5e-2 * scale and float(d.mean()) <= 6e-3 * scale, (float(d.max()) / scale, float(d.mean()) / scale)


@pytest.mark.parametrize("c0,l", [(131, 4096), (134, 1000), (128, 77)])
def test_bf16_chain_one_launch_equals_layer_by_layer(device, c0, l):
    """captra_mlp_chain_bf16 (FP1 + conv1 register-resident, optionally CoordinateNet's heads behind them, one launch) against the
    same layers through captra_pointwise_mlp_bf16pm with bf16 point-major tensors in between: the same roundings at the same
    places and the same k-ascending accumulation, so the feature map agrees element for element (a rare 1-ulp bf16 flip from the
    MFMA's internal order aside) and the heads' outputs to 1e-5; and against the float64 layer contract."""
    from captra_amd import fused
    rng = np.random.default_rng(c0 + l)
    B = 2
    x = rng.standard_normal((B, c0, l)).astype(np.float32)
    dims = [c0, 128, 128, 128]
    ws = [((rng.standard_normal((dims[i], dims[i + 1])) / np.sqrt(dims[i])).astype(np.float32), rng.standard_normal(dims[i + 1]).astype(np.float32)) for i in range(3)]
    hw = [((rng.standard_normal((128, c)) / np.sqrt(128)).astype(np.float32), rng.standard_normal(c).astype(np.float32)) for c in (2, 128, 3)]
    layers = [fused.pack(_dev(w, device), _dev(b, device)) for w, b in ws]
    heads = [fused.pack(_dev(w, device), _dev(b, device)) for w, b in hw]
    xd = _dev(x, device)
    with fused.use_mlp_dtype("bf16"):
        assert fused.chain_bf16_supported(xd, layers) and fused.chain_bf16_supported(xd, layers, heads)
        feat = fused.mlp_chain_bf16_fused(xd, layers)
        seg, nocs = fused.mlp_chain_bf16_fused(xd, layers, heads)
        ref_pm = fused.mlp_chain_bf16(xd, layers, [fused.ACT_RELU] * 3, out_pm=True)
        ref_seg = fused.pointwise_mlp_bf16pm(ref_pm, heads[0], l, in_pm=True, out_pm=False)
        hid = fused.pointwise_mlp_bf16pm(ref_pm, heads[1], l, in_pm=True, out_pm=True, act=fused.ACT_RELU)
        ref_nocs = fused.pointwise_mlp_bf16pm(hid, heads[2], l, in_pm=True, out_pm=False, act=fused.ACT_SIGMOID_M05)
    got, ref = _pm_to_dense(feat.data, 128), _pm_to_dense(ref_pm, 128)
    assert feat.channels == 128 and np.mean(got == ref) > 0.999 and np.abs(got - ref).max() <= 2.0 ** -7 * np.abs(ref).max()
    np.testing.assert_allclose(seg.cpu().numpy(), ref_seg.cpu().numpy(), atol=2e-2 * float(ref_seg.abs().max()), rtol=0)
    assert float((seg - ref_seg).abs().mean()) <= 1e-4 * float(ref_seg.abs().max())
    assert float((nocs - ref_nocs).abs().mean()) <= 1e-4 and float((nocs - ref_nocs).abs().max()) <= 2e-2
    h = x
    for w, b in ws:
        h = _bf16_layer(h, w, b, 1)
    scale = float(np.abs(h).max())
    err = np.abs(got - _bf16_round(h))
    assert err.max() <= 3e-2 * scale and err.mean() <= 2e-4 * scale


def test_bf16_mode_track_step_close_to_fp32(device):
    """The whole tracking step with bf16 MFMA operands in the shared MLPs (fused.use_mlp_dtype / cfg['mlp_dtype'], BASELINE.json configs[2]) stays
    close to the exact-fp32 step on the same inputs: NOCS coordinates within bf16-level error, (almost) no label flips."""
    from captra_amd import fused
    from captra_amd.configs import make_config
    from captra_amd.trainer import Trainer
    cfg = make_config("1", experiment_dir="/tmp/captra_bf16_test")
    cfg["device"] = device
    trainer = Trainer(cfg)
    sd = make_state_dict({k: tuple(v.shape) for k, v in trainer.model.state_dict().items()}, seed=7)
    trainer.model.load_state_dict(sd)
    data = clouds.make_trajectory("nocs", 4, 3, seed=0)
    model = trainer.model.to(device).eval()
    model.set_data(data)
    pose = {k: v.clone() for k, v in model.feed_dict[0]["gt_part"].items()}
    outs = {}
    for dt in ("fp32", "bf16"):
        fused.set_mlp_dtype(dt)
        try:
            with torch.no_grad():
                npcs, _ = model.track_step(dict(model.feed_dict[1]), dict(model.npcs_feed_dict[1]), {k: v.clone() for k, v in pose.items()})
        finally:
            fused.set_mlp_dtype("fp32")
        outs[dt] = (npcs["nocs"].cpu().numpy(), npcs["seg"].cpu().numpy())
    d = np.abs(outs["fp32"][0] - outs["bf16"][0])
    assert np.isfinite(outs["bf16"][0]).all() and d.mean() < 5e-3 and d.max() < 5e-2, (d.mean(), d.max())
    flips = (outs["fp32"][1].argmax(1) != outs["bf16"][1].argmax(1)).mean()
    assert flips < 0.01, flips


def test_coord_tail_one_launch_equals_layer_by_layer(device):
    """CoordNet's FP1 + conv1 + seg / NOCS heads as one launch == the same layers through captra_pointwise_mlp (bit-exact
    for the logits; the NOCS sigmoid uses the same expf) and the reference-structured torch path to 1e-5."""
    from captra_amd import fused
    rng = np.random.default_rng(77)
    B, c0, l = 2, 134, 1000
    x = rng.standard_normal((B, c0, l)).astype(np.float32)
    dims = [(c0, 128), (128, 128), (128, 128), (128, 2), (128, 128), (128, 3)]
    layers = [((rng.standard_normal(d) / np.sqrt(d[0])).astype(np.float32), rng.standard_normal(d[1]).astype(np.float32)) for d in dims]
    packed = [fused.pack(_dev(w, device), _dev(b, device)) for w, b in layers]
    assert fused.coord_tail_supported(_dev(x, device), packed)
    seg, nocs = fused.coord_tail(_dev(x, device), packed)
    feat = x
    for w, b in layers[:3]:
        feat = O.pointwise_mlp(feat, w, b, 1)
    np.testing.assert_array_equal(seg.cpu().numpy(), O.pointwise_mlp(feat, layers[3][0], layers[3][1], 0))
    hid = O.pointwise_mlp(feat, layers[4][0], layers[4][1], 1)
    raw = O.pointwise_mlp(hid, layers[5][0], layers[5][1], 0)
    np.testing.assert_allclose(nocs.cpu().numpy(), 1.0 / (1.0 + np.exp(-raw.astype(np.float64))) - 0.5, atol=2e-7, rtol=0)


@pytest.mark.parametrize("cfeat,chans,k,mode", [(3, (64, 64, 128), 64, 0), (3, (64, 64, 128), 64, 2), (3, (64, 96, 128), 128, 0),
                                                 (320, (128, 128, 256), 64, 0), (0, (64, 64, 128), 64, 1)])
def test_sa_scale_with_padded_neighbour_lists(device, cfeat, chans, k, mode):
    """Ball-query style lists (short lists padded with the first neighbour), including an empty ball (all zeros), a
    single-neighbour ball and a later slice that merely starts with the first neighbour: every SA kernel variant equals the
    oracle.  (Skipping slices that only repeat the first neighbour was tried -- exact, but no measurable gain at 4-11 % of
    redundant slices -- and dropped; this test is what would guard it.)"""
    import ctypes
    from captra_amd import _lib, fused
    rng = np.random.default_rng(cfeat + k + mode)
    B, n, m = 2, 600, 70
    xyz_cn = (rng.random((B, 3, n), dtype=np.float32) - 0.5)
    feat = rng.standard_normal((B, cfeat, n)).astype(np.float32) if cfeat else None
    new_xyz = (rng.random((B, m, 3), dtype=np.float32) - 0.5)
    idx = np.zeros((B, m, k), np.int32)
    for b in range(B):
        for c in range(m):
            cnt = int(rng.integers(1, k + 1)) if c % 7 else (1 if c % 14 else k)
            lst = np.sort(rng.choice(n, cnt, replace=False)).astype(np.int32)
            idx[b, c, :cnt] = lst
            idx[b, c, cnt:] = lst[0]
    idx[0, 3, :] = 0                                                   # empty ball: the op leaves zeros
    idx[1, 5, 32] = idx[1, 5, 0]; idx[1, 5, 33:40] = rng.integers(0, n, 7)   # slice 1 starts with the first neighbour, then differs
    dims = (cfeat + 3,) + chans
    layers = [((rng.standard_normal((dims[i], dims[i + 1])) / np.sqrt(dims[i])).astype(np.float32),
               rng.standard_normal(dims[i + 1]).astype(np.float32)) for i in range(3)]
    packed = [fused.pack(_dev(w, device), _dev(b_, device)) for w, b_ in layers]
    out = torch.full((B, chans[2], m), -1.0, device=device)
    f_dev = None if feat is None else _dev(feat, device)
    _lib.lib().captra_sa_fused_set_mode(ctypes.c_int(mode))
    try:
        if f_dev is not None and fused.sa_scale_pre_supported(cfeat, packed, k):
            fused.sa_scale_pre(fused.sa_first_layer_pre(f_dev, packed[0]), _dev(xyz_cn, device), _dev(new_xyz, device), _dev(idx, device), packed, out, 0, cfeat)
        else:
            fused.sa_scale_fused(f_dev, _dev(xyz_cn, device), _dev(new_xyz, device), _dev(idx, device), packed, out, 0)
    finally:
        _lib.lib().captra_sa_fused_set_mode(ctypes.c_int(0))
    x = O.sa_group(feat, xyz_cn, new_xyz, idx)
    for w, b_ in layers:
        x = O.pointwise_mlp(x, w, b_, 1)
    np.testing.assert_array_equal(out.cpu().numpy(), O.max_over_k(x))


@pytest.mark.parametrize("tag,cat,objcfg,kind", [("bottle", "1", "obj_info_nocs.yml", "nocs"), ("camera", "3", "obj_info_nocs.yml", "nocs"),
                                                 ("drawers", "drawers", "obj_info_sapien.yml", "arti")])
def test_track_loss_dict_vs_reference(device, tag, cat, objcfg, kind):
    """`Trainer.test(data)` with evaluation on (the default of the reference's test.py): the whole loss dict of
    EvalTrackModel.compute_loss — pose errors of the prediction and of its initialisation, CoordinateNet's segmentation
    and NOCS losses, the three box IoUs — against golden G13 (tests/golden/make_golden_trackloss.py)."""
    from captra_amd.configs import make_config
    from captra_amd.trainer import Trainer
    g = np.load(Path(__file__).resolve().parent / "golden" / "g13_trackloss.npz")
    cfg = make_config(cat, objcfg, experiment_dir="/tmp/captra_trackloss")
    cfg["device"] = device
    cfg["track_cfg"]["gt_label"] = (tag == "drawers")
    trainer = Trainer(cfg)
    trainer.model.load_state_dict(make_state_dict({k: tuple(v.shape) for k, v in trainer.model.state_dict().items()}, seed=7))
    data = clouds.make_trajectory(kind, 2, 3, seed=0)
    torch.manual_seed(1234)
    np.random.seed(1234)
    _, loss = trainer.test(data)

    def flatten(d, prefix=""):
        out = {}
        for k, v in d.items():
            if isinstance(v, dict):
                out.update(flatten(v, f"{prefix}{k}/"))
            else:
                out[f"{prefix}{k}"] = float(v.detach()) if torch.is_tensor(v) else float(v)
        return out

    got = flatten({k: v for k, v in loss.items() if not k.startswith("frame_")})
    ref = {k.split("/", 1)[1]: float(g[k]) for k in g.files if k.startswith(tag + "/")}
    assert sorted(got) == sorted(ref)
    for k in sorted(ref):
        if tag == "drawers":
            # random weights drive the drawers' free-running poses out of the physical regime after frame 1 (negative
            # scales) where rounding noise is amplified (see test_track_loop_vs_golden): sanity bound only
            np.testing.assert_allclose(got[k], ref[k], rtol=5e-2, atol=5e-2, err_msg=k)
        elif "deg" in k and "cm" in k:
            assert abs(got[k] - ref[k]) < 1e-6, k
        else:
            # rdiff = acos(trace) in degrees: ill-conditioned near 0 and near 180 (random weights: 126-degree errors on the
            # drawers), pooled over a handful of points per part there -> 2e-3 relative; IoU: occupancy on a 50^3 grid
            atol = 5e-3 if "rdiff" in k else 2e-3 if "iou" in k else 1e-4
            np.testing.assert_allclose(got[k], ref[k], rtol=2e-3 if "rdiff" in k else 2e-4, atol=atol, err_msg=k)


def test_transform_pts_batch_free_rotation_vs_reference(device):
    """transform_pts_batch with no rotation given: the 3x3 Procrustes runs captra_procrustes_rot3 (on-device Jacobi SVD) where
    the reference calls torch.svd on the CPU — same rotation, scale and translation (golden G14)."""
    from captra_amd.pose_utils import procrustes as P
    from tests.golden.make_golden_api import inputs
    g = np.load(G / "g14_api.npz")
    d = inputs()
    r, s, t = P.transform_pts_batch(_dev(d["src"], device), _dev(d["tgt"], device))
    np.testing.assert_allclose(r.cpu().numpy(), g["tpb_free_rot"], atol=2e-5)
    np.testing.assert_allclose(s.cpu().numpy(), g["tpb_free_scale"], atol=2e-5)
    np.testing.assert_allclose(t.cpu().numpy(), g["tpb_free_trans"], atol=2e-5)


def test_seg_readout_and_track_fit_one_launch_forms(device):
    """The step's folded read-outs against the torch ops they replace: captra_seg_softmax_argmax == F.softmax + first-index arg
    max (ties included); captra_part_fit_st_track == captra_part_fit_st on points + mean with torch.where fallbacks, bit for
    bit (same additions, same reductions), with an empty and a 3-point part in the batch; captra_copy_multi copies."""
    from captra_amd import fused
    from captra_amd.pose_utils.pose_fit import part_fit_st_cn, part_fit_st_track
    g = torch.Generator().manual_seed(4)
    logits = torch.randn(3, 4, 1000, generator=g)
    logits[0, 1, :50] = logits[0, 3, :50] = 7.0                      # exact ties at the maximum: the FIRST index wins
    seg, lab = fused.seg_softmax_argmax(logits.to(device))
    np.testing.assert_allclose(seg.cpu().numpy(), torch.softmax(logits, 1).numpy(), atol=1e-6, rtol=0)
    np.testing.assert_array_equal(lab.cpu().numpy(), torch.argmax(logits, 1).numpy().astype(np.int32))
    assert (lab[0, :50] == 1).all()
    B, P, N = 4, 2, 2048
    labels = torch.randint(0, P + 1, (B, N), generator=g).int()
    labels[1] = torch.where(labels[1] == 1, torch.full_like(labels[1], 2), labels[1])      # trajectory 1: part 1 is empty
    labels[2, 3:] = torch.where(labels[2, 3:] == 0, torch.full_like(labels[2, 3:], 2), labels[2, 3:])
    labels[2, :3] = 0                                                                         # trajectory 2: part 0 has 3 points
    src = torch.randn(B, P, 3, N, generator=g)
    pts, mean = torch.randn(B, 3, N, generator=g) * 0.2, torch.randn(B, 3, 1, generator=g)
    rot = torch.linalg.qr(torch.randn(B, P, 3, 3, generator=g))[0]
    prev_s, prev_t = torch.rand(B, P, generator=g) + 0.5, torch.randn(B, P, 3, 1, generator=g)
    d = lambda t: t.to(device).contiguous()      # noqa: E731
    for sym in (True, False):
        s0, t0, v0 = part_fit_st_cn(d(labels), d(src), d(pts + mean), d(rot), sym)
        exp_s, exp_t = torch.where(v0, s0, d(prev_s)), torch.where(v0[..., None, None], t0, d(prev_t))
        s1, t1, v1 = part_fit_st_track(d(labels), d(src), d(pts), d(mean), d(rot), d(prev_s), d(prev_t), sym)
        assert torch.equal(v0, v1) and not bool(v1[1, 1]) and not bool(v1[2, 0]) and bool(v1[0].all())
        assert torch.equal(s1, exp_s) and torch.equal(t1, exp_t)
    a = [torch.randn(n, generator=g).to(device) for n in (9, 36, 4096, 5)]
    b = [torch.zeros_like(x) for x in a]
    fused.copy_multi(list(zip(a, b)))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
