"""tests/f32_judge.py proven on the CPU, on the shapes tests/test_f32_edges_gpu.py runs:

(a) its classes equal those of the reference's real operators in torch (nn.Conv1d / nn.Conv2d + F.relu + torch.max(..., -1)[0],
    F.max_pool2d, nn.GroupNorm + ReLU) for every poison value, and those of the CPU oracle's exact chain;
(b) it rejects the mutants: an fp32 layer whose ReLU is `v > 0 ? v : 0`, one whose pool is fmax, one with the sign-dependent integer
    ReLU, one that pads cout with zero-weight rows between two layers -- each on at least one case;
(c) no case is vacuous: dependent and independent outputs both exist, the independent ones are finite, a NaN poison gives a NaN, and
    the two Inf poisons of a case TOGETHER give a NaN, a +Inf and a finite dependent output.  (Together, because one Inf through a
    ReLU chain cannot give all three: -Inf under the strictly positive first-layer weights is 0 behind the ReLU and everything behind
    it finite, +Inf is +Inf / NaN everywhere.  GroupNorm and the plain row maximum are excepted as stated at their tests: GroupNorm
    makes every non-finite group NaN, the row maximum only hands the poison's own class on.)
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ops as O
from tests import f32_judge as J

POISON_NAMES = list(J.POISONS)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _conv(x, w, b, relu):
    """nn.Conv1d / nn.Conv2d with kernel size 1 holding the layer (w (cin, cout)), then F.relu: the reference's operators."""
    cin, cout = w.shape
    conv = (torch.nn.Conv1d if x.dim() == 3 else torch.nn.Conv2d)(cin, cout, 1)
    with torch.no_grad():
        conv.weight.copy_(_t(w.T).reshape(conv.weight.shape))
        conv.bias.copy_(_t(b))
        y = conv(x)
    return F.relu(y) if relu else y


def _same_classes(got, cls, what):
    got = got.numpy() if isinstance(got, torch.Tensor) else got
    bad = J.class_mismatches(got, cls)
    assert bad == 0, (what, bad)


def _check_vacuity(facts_by_poison, inf_all_three=True):
    for name, f in facts_by_poison.items():
        assert f["dep"] and f["indep"] and f["indep_finite"], (name, f)
        if name in J.NAN_POISONS:
            assert f["nan"], (name, f)
    if inf_all_three:
        infs = [facts_by_poison[n] for n in J.INF_POISONS]
        assert any(f["nan"] for f in infs) and any(f["pinf"] for f in infs) and any(f["finite_dep"] for f in infs), infs


# ---- the cases: inputs, poison index, the judge's verdict ----------------------------------------------------------------------------
def dense_case(cin, cout, L, B, pos, name):
    rng = J.case_rng("dense", cin, cout, L)
    row = cin // 2
    (w, b), = J.poisoned_layers(rng, (cin, cout), row)
    index = (J.middle(B), row, pos)
    x = J.put_bits(rng.standard_normal((B, cin, L)), index, name)
    return x, w, b, index


@pytest.mark.parametrize("cin,cout,L,B", J.DENSE_CASES)
def test_dense_layer_vs_conv1d_relu(cin, cout, L, B):
    facts = {}
    for name in POISON_NAMES:
        for pos in J.edge_positions(L):
            x, w, b, index = dense_case(cin, cout, L, B, pos, name)
            cls, val, dep = J.verdict(J.dense(J.T.poisoned(x, index), w, b, True))
            _same_classes(_conv(_t(x), w, b, True), cls, ("conv1d", name, pos))
            _same_classes(O.pointwise_mlp(x, w, b, 1), cls, ("oracle", name, pos))
            fin = cls == J.FIN
            np.testing.assert_allclose(O.pointwise_mlp(x, w, b, 1)[fin], val[fin], atol=1e-4, rtol=1e-5)
            assert dep.sum() == cout and dep[index[0], :, pos].all()
            facts[name] = J.non_vacuous(cls, dep)
    _check_vacuity(facts)


def chain_case(c0, L, B, pos, name, widths=(128, 128, 128)):
    rng = J.case_rng("chain", c0, L, widths)
    row = c0 // 2
    layers = J.poisoned_layers(rng, (c0,) + tuple(widths), row)
    index = (J.middle(B), row, pos)
    x = J.put_bits(rng.standard_normal((B, c0, L)), index, name)
    return x, layers, index


@pytest.mark.parametrize("c0,L,B", J.CHAIN_CASES)
@pytest.mark.parametrize("act3", [0, 1])
def test_three_layer_chain_vs_conv1d_relu(c0, L, B, act3):
    facts = {}
    for i, name in enumerate(POISON_NAMES):
        pos = J.edge_positions(L)[i % 3]
        x, layers, index = chain_case(c0, L, B, pos, name)
        cls, val, dep = J.verdict(J.chain(J.T.poisoned(x, index), layers, [1, 1, act3]))
        y, yo = _t(x), x
        for (w, b), a in zip(layers, [1, 1, act3]):
            y, yo = _conv(y, w, b, bool(a)), O.pointwise_mlp(yo, w, b, a)
        _same_classes(y, cls, ("conv1d", name))
        _same_classes(yo, cls, ("oracle", name))
        assert dep.sum() == 128
        facts[name] = J.non_vacuous(cls, dep)
    _check_vacuity(facts)


def sa_case(cfeat, chans, N, M, K, B, name, where, point="first_and_last_slot"):
    """where: "feat" (a feature channel; cfeat > 0) or "xyz" (a coordinate)."""
    rng = J.case_rng("sa", cfeat, chans, N, M, K)
    xyz_cn, feat, new_xyz, idx = J.sa_inputs(rng, cfeat, chans, N, M, K, B)
    cloud, p = J.middle(B), J.SA_POINTS[point]
    row = (cfeat // 2) if where == "feat" else cfeat + 1
    layers = J.poisoned_layers(rng, (cfeat + 3,) + tuple(chans), row)
    if where == "feat":
        index = (cloud, row, p)
        feat = J.put_bits(feat, index, name)
        tf, tx = J.T.poisoned(feat, index), J.T(xyz_cn)
    else:
        index = (cloud, 1, p)
        xyz_cn = J.put_bits(xyz_cn, index, name)
        tf, tx = (None if feat is None else J.T(feat)), J.T.poisoned(xyz_cn, index)
    return xyz_cn, feat, new_xyz, idx, layers, tf, tx, index


def _torch_sa(xyz_cn, feat, new_xyz, idx, layers, pool):
    g = _t(O.sa_group(feat, xyz_cn, new_xyz, idx))                      # the gather itself is data movement and one subtraction
    for w, b in layers:
        g = _conv(g, w, b, True)
    return torch.max(g, -1)[0] if pool == "max" else F.max_pool2d(g, [1, g.shape[-1]]).squeeze(-1)


@pytest.mark.parametrize("cfeat,chans,N,M,K,B,where", J.sa_cases_with_poison_site(J.SA_CASES + J.SA_PRE_CASES))
def test_sa_scale_vs_conv2d_relu_max(cfeat, chans, N, M, K, B, where):
    facts = {}
    for i, name in enumerate(POISON_NAMES):
        point = ("first_and_last_slot", "padded_slots_only")[i % 2]
        xyz_cn, feat, new_xyz, idx, layers, tf, tx, index = sa_case(cfeat, chans, N, M, K, B, name, where, point)
        cls, val, dep = J.verdict(J.sa_scale_dependent_only(tf, tx, new_xyz, idx, layers))
        _same_classes(_torch_sa(xyz_cn, feat, new_xyz, idx, layers, "max"), cls, ("torch.max", name))
        if i < 2:
            _same_classes(_torch_sa(xyz_cn, feat, new_xyz, idx, layers, "pool2d"), cls, ("max_pool2d", name))
        x = O.sa_group(feat, xyz_cn, new_xyz, idx)
        for w, b in layers:
            x = O.pointwise_mlp(x, w, b, 1)
        _same_classes(O.max_over_k(x), cls, ("oracle", name))
        # dependence is idx's: exactly the centres that name the point, in the poisoned cloud
        named = (idx[index[0]] == index[2]).any(-1)
        assert (dep[index[0]] == named[None, :]).all() and not np.delete(dep, index[0], 0).any()
        assert named.sum() == (2 if point == "first_and_last_slot" else 1)
        facts[name] = J.non_vacuous(cls, dep)
    _check_vacuity(facts)
    # a point no slot names: nothing depends on it
    xyz_cn, feat, new_xyz, idx, layers, tf, tx, index = sa_case(cfeat, chans, N, M, K, B, "qnan_neg", where, "unnamed")
    cls, _, dep = J.verdict(J.sa_scale_dependent_only(tf, tx, new_xyz, idx, layers))
    assert not dep.any() and (cls == J.FIN).all()
    _same_classes(_torch_sa(xyz_cn, feat, new_xyz, idx, layers, "max"), cls, "unnamed")


def max_case(cin, cout, M, K, B, name, slot):
    rng = J.case_rng("max", cin, cout, M, K)
    row = cin // 2
    (w, b), = J.poisoned_layers(rng, (cin, cout), row)
    index = (J.middle(B), row, M // 2, slot)
    x = J.put_bits(rng.standard_normal((B, cin, M, K)), index, name)
    return x, w, b, index


@pytest.mark.parametrize("cin,cout,M,K,B", J.MAX_CASES)
def test_layer_and_max_over_k_vs_conv2d_relu_max(cin, cout, M, K, B):
    facts = {}
    for name in POISON_NAMES:
        for slot in J.edge_positions(K):
            x, w, b, index = max_case(cin, cout, M, K, B, name, slot)
            cls, val, dep = J.verdict(J.max_last(J.dense(J.T.poisoned(x, index), w, b, True)))
            _same_classes(torch.max(_conv(_t(x), w, b, True), -1)[0], cls, ("torch.max", name))
            _same_classes(O.max_over_k(O.pointwise_mlp(x, w, b, 1)), cls, ("oracle", name))
            assert dep.sum() == cout
            facts[name] = J.non_vacuous(cls, dep)
    # (behind the max a -Inf poison's finite outputs and a +Inf poison's zeros are finite dependent outputs)
    _check_vacuity(facts)


def gn_case(B, C, N, groups, name, pos):
    rng = J.case_rng("gn", B, C, N, groups)
    gamma, beta = rng.standard_normal(C).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    index = (J.middle(B), C // 2, pos)
    x = J.put_bits(rng.standard_normal((B, C, N)), index, name)
    return x, gamma, beta, index


@pytest.mark.parametrize("B,C,N,groups", J.GN_CASES)
@pytest.mark.parametrize("relu", [False, True])
def test_group_norm_vs_torch(B, C, N, groups, relu):
    """Excepted from the +Inf / finite-dependent condition: every non-finite value makes its whole (cloud, group) NaN."""
    facts = {}
    for name in POISON_NAMES:
        for pos in J.edge_positions(N):
            x, gamma, beta, index = gn_case(B, C, N, groups, name, pos)
            cls, val, dep = J.verdict(J.group_norm(J.T.poisoned(x, index), groups, gamma, beta, 1e-5, relu))
            gn = torch.nn.GroupNorm(groups, C, eps=1e-5)
            with torch.no_grad():
                gn.weight.copy_(_t(gamma))
                gn.bias.copy_(_t(beta))
                y = gn(_t(x))
            _same_classes(F.relu(y) if relu else y, cls, (name, pos))
            assert dep.sum() == C // groups * N and (cls[dep] == J.NAN).all()
            facts[name] = J.non_vacuous(cls, dep)
    _check_vacuity(facts, inf_all_three=False)


@pytest.mark.parametrize("B,C,N", J.ROW_MAX_CASES)
def test_row_max_vs_torch(B, C, N):
    """Excepted from the all-three condition: the maximum of a row hands the poison's own class on (-Inf loses: finite)."""
    rng = J.case_rng("rowmax", B, C, N)
    facts = {}
    for name in POISON_NAMES:
        for pos in J.edge_positions(N):
            index = (J.middle(B), C // 2, pos)
            x = J.put_bits(rng.standard_normal((B, C, N)), index, name)
            cls, val, dep = J.verdict(J.max_last(J.T.poisoned(x, index), keepdims=True))
            _same_classes(torch.max(_t(x), 2, keepdim=True)[0], cls, (name, pos))
            assert dep.sum() == 1
            facts[name] = J.non_vacuous(cls, dep)
    _check_vacuity(facts, inf_all_three=False)
    assert facts["inf_pos"]["pinf"] and facts["inf_neg"]["finite_dep"]


@pytest.mark.parametrize("B,N,S,c1,c2", J.INTERP_CASES)
def test_interp_concat_vs_torch(B, N, S, c1, c2):
    rng = J.case_rng("interp", B, N, S)
    skip = rng.standard_normal((B, c1, N)).astype(np.float32)
    known = rng.standard_normal((B, c2, S)).astype(np.float32)
    idx = rng.integers(0, S, (B, N, 3)).astype(np.int32)
    wgt = rng.random((B, N, 3)).astype(np.float32)
    wgt /= wgt.sum(-1, keepdims=True)
    for name in POISON_NAMES:
        i_skip, i_known = (J.middle(B), c1 // 2, N - 1), (J.middle(B), c2 // 2, S // 2)
        for src, index in (("skip", i_skip), ("known", i_known)):
            sk = J.put_bits(skip, index, name) if src == "skip" else skip
            kn = J.put_bits(known, index, name) if src == "known" else known
            ts = J.T.poisoned(sk, index) if src == "skip" else J.T(sk)
            tk = J.T.poisoned(kn, index) if src == "known" else J.T(kn)
            cls, val, dep = J.verdict(J.interp_concat(ts, tk, idx, wgt))
            g = torch.stack([_t(kn)[b][:, torch.from_numpy(idx[b].astype(np.int64))] for b in range(B)])      # (B, c2, N, 3)
            ref = torch.cat([_t(sk), (g * _t(wgt)[:, None]).sum(-1)], 1)
            _same_classes(ref, cls, (name, src))
            f = J.non_vacuous(cls, dep)
            assert f["dep"] and f["indep"] and f["indep_finite"] and (cls[dep] != J.FIN).all()


# ---- (b) mutants -------------------------------------------------------------------------------------------------------------------------
def _f32_dense(x, w, b, relu_fn):
    y = np.broadcast_to(b[None, :, None], (x.shape[0], w.shape[1], x.shape[2])).astype(np.float32).copy()
    with np.errstate(all="ignore"):
        for k in range(w.shape[0]):
            y += w[k][None, :, None] * x[:, k:k + 1]
    return relu_fn(y) if relu_fn else y


def _relu_select(v):                      # v > 0 ? v : 0
    return np.where(v > 0, v, np.float32(0))


def _relu_int(v):                         # max on the bit pattern as a signed integer
    return np.maximum(np.ascontiguousarray(v).view(np.int32), 0).view(np.float32)


def _relu_ref(v):
    return J.relu(v).astype(np.float32)


def _rejected(got, cls):
    return J.class_mismatches(got, cls) > 0


def test_judge_rejects_the_mutants_and_accepts_the_faithful_layer():
    cin, cout, L, B = J.DENSE_CASES[1]
    verdicts = {}
    for name in POISON_NAMES:
        x, w, b, index = dense_case(cin, cout, L, B, L - 1, name)
        verdicts[name] = (x, w, b, J.verdict(J.dense(J.T.poisoned(x, index), w, b, True))[0])
        assert not _rejected(_f32_dense(x, w, b, _relu_ref), verdicts[name][3]), name          # the faithful fp32 layer passes
    # ReLU as a float select: every NaN becomes 0
    for name in J.NAN_POISONS:
        x, w, b, cls = verdicts[name]
        assert _rejected(_f32_dense(x, w, b, _relu_select), cls), name
    # ReLU on the integer bit pattern: a sign-clear NaN passes, a sign-set one becomes 0.  The poison's own sign is not what
    # reaches the ReLU (x86 arithmetic on NaNs keeps the first operand's payload and sign), so the mutant is shown on the layer's raw
    # output with the NaNs given the sign-set pattern
    x, w, b, cls = verdicts["qnan_neg"]
    raw = _f32_dense(x, w, b, None)
    raw.view(np.uint32)[np.isnan(raw)] = 0xFFC00000
    assert _rejected(_relu_int(raw), cls) and not _rejected(_relu_ref(raw), cls)
    raw.view(np.uint32)[np.isnan(raw)] = 0x7FC00000
    assert not _rejected(_relu_int(raw), cls)
    # fmax pool: the NaN loses
    cin, cout, M, K, B = J.MAX_CASES[0]
    for name in J.NAN_POISONS:
        x, w, b, index = max_case(cin, cout, M, K, B, name, K - 1)
        cls = J.verdict(J.max_last(J.dense(J.T.poisoned(x, index), w, b, True)))[0]
        h = _f32_dense(x.reshape(B, cin, M * K), w, b, _relu_ref).reshape(B, cout, M, K)
        assert not _rejected(h.max(-1), cls), name
        assert _rejected(np.fmax.reduce(h, axis=-1), cls), name


@pytest.mark.parametrize("c0,L,B", J.CHAIN_CASES)
def test_wave_model_is_the_signed_integer_relu_and_pool(c0, L, B):
    """The documented exception (J.relu_wave, `wave=True`) restates an fp32 chain whose inner ReLUs and whose pool are a max on the
    bit pattern as a signed integer.  x86 arithmetic signs its NaNs as the fp32 MFMA was measured to (an input NaN keeps its sign, a
    generated one is 0xFFC00000), so the fp32 numpy chain below stands in for the kernels: same classes for every poison.  And the
    exception is an exception: it differs from the reference's verdict for the sign-set NaN and for +Inf (whose Inf - Inf in the last
    layer is a generated, sign-set NaN), and agrees with it for the sign-clear NaNs."""
    for i, name in enumerate(POISON_NAMES):
        pos = J.edge_positions(L)[i % 3]
        x, layers, index = chain_case(c0, L, B, pos, name)
        ref_cls = J.verdict(J.chain(J.T.poisoned(x, index), layers, [1, 1, 1]))[0]
        wave_cls = J.verdict(J.chain(J.T.poisoned(x, index), layers, [1, 1, 1], wave=True))[0]
        h = _f32_dense(_f32_dense(x, *layers[0], _relu_int), *layers[1], _relu_int)
        _same_classes(_f32_dense(h, *layers[2], _relu_ref), wave_cls, ("chain", name))
        # ... and as an SA scale: the L positions as one centre's neighbours, ReLU + pool on the bits
        t = J.T.poisoned(x, index)
        for w, b in layers:
            t = J.dense(t, w, b, True, wave=True)
        pooled = np.maximum(np.ascontiguousarray(_f32_dense(h, *layers[2], None)).view(np.int32).max(-1), 0).view(np.float32)
        wave_pool = J.verdict(J.max_last(t))[0]
        _same_classes(pooled, wave_pool, ("pool", name))
        ref_pool = J.verdict(J.max_last(J.chain(J.T.poisoned(x, index), layers, [1, 1, 1])))[0]
        # the chain's last activation is the reference's own (the store epilogue), so only the sign-set input NaN differs there;
        # behind the pool the NaN that +Inf generates in the last layer is lost as well
        assert bool((ref_cls != wave_cls).any()) == (name == "qnan_neg"), name
        assert bool((ref_pool != wave_pool).any()) == (name in ("qnan_neg", "inf_pos")), name


def test_judge_rejects_zero_weight_padding_between_two_layers():
    """cout 96 padded to 128 with zero weight rows and zero bias, the next layer reading all 128: under +Inf the padded rows hold
    0 * Inf = NaN, which 0 * NaN hands to every output of the next layer; the reference gives +Inf there."""
    rng = J.case_rng("padding")
    cin, c1, c2, L, B = 16, 96, 64, 40, 3
    layers = J.poisoned_layers(rng, (cin, c1, c2), cin // 2)
    layers = [layers[0], (np.abs(layers[1][0]) + np.float32(0.01), layers[1][1])]            # second layer strictly positive: +Inf stays +Inf
    index = (1, cin // 2, L - 1)
    for name in J.INF_POISONS + J.NAN_POISONS:
        x = J.put_bits(rng.standard_normal((B, cin, L)), index, name)
        cls = J.verdict(J.chain(J.T.poisoned(x, index), layers, [1, 1]))[0]
        w1p = np.zeros((cin, 128), np.float32)
        w1p[:, :c1] = layers[0][0]
        b1p = np.zeros(128, np.float32)
        b1p[:c1] = layers[0][1]
        w2p = np.zeros((128, c2), np.float32)
        w2p[:c1] = layers[1][0]
        faithful = _f32_dense(_f32_dense(x, *layers[0], _relu_ref), *layers[1], _relu_ref)
        padded = _f32_dense(_f32_dense(x, w1p, b1p, _relu_ref), w2p, layers[1][1], _relu_ref)
        assert not _rejected(faithful, cls), name
        if name == "inf_pos":
            assert (cls[index[0], :, index[2]] == J.PINF).all()
            assert _rejected(padded, cls)
        elif name == "inf_neg":
            assert (cls == J.FIN).all()                                   # 0 behind the first ReLU
            assert _rejected(padded, cls)                                 # ... but 0 * -Inf = NaN in the padded rows
