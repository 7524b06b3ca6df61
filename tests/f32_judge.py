"""Judge for the exact-fp32 kernels' NaN / Inf semantics (tests/test_f32_edges_gpu.py; proven by tests/test_f32_judge_cpu.py).

A float64 numpy restatement of every operation of the shared-MLP path with the REFERENCE's semantics, not the kernels':
ReLU is F.relu (a NaN of either sign and any payload stays a NaN), the pools are torch.max / F.max_pool2d (a NaN among the pooled
values wins), GroupNorm normalises with the group's own mean and variance (one non-finite value makes the whole (cloud, group) NaN),
and no channel count is padded, so no 0 * Inf appears that the layer's own weights do not hold.

Every operation works on a `T`: the float64 values and, beside them, the DEPENDENCE mask -- which elements depend on the poisoned
input element at all.  The mask follows from the operation's structure alone (a dense layer mixes the channels of one position, a
pool the K slots of one centre, GroupNorm the (cloud, group), a gather follows `idx`), never from the values: an output whose value
happens not to change (a zero weight, a lost maximum) is still dependent.  `verdict` turns a T into (class, value, dependence).
"""
from __future__ import annotations

import numpy as np

FIN, PINF, NINF, NAN = 0, 1, 2, 3
CLASS_NAMES = ("finite", "+Inf", "-Inf", "NaN")

# the poison values, by bit pattern: quiet NaN with the sign clear / set (what x86 host code produces from inf - inf and 0 * inf is
# the sign-set one), a signalling NaN with a payload, and the infinities
POISONS = {"qnan_pos": 0x7FC00000, "qnan_neg": 0xFFC00000, "snan_payload": 0x7F800001, "inf_pos": 0x7F800000, "inf_neg": 0xFF800000}
NAN_POISONS = ("qnan_pos", "qnan_neg", "snan_payload")
INF_POISONS = ("inf_pos", "inf_neg")


def poison_f32(name: str) -> np.float32:
    return np.array([POISONS[name]], dtype=np.uint32).view(np.float32)[0]


def put_bits(a: np.ndarray, index, name: str) -> np.ndarray:
    """A copy of the fp32 array `a` with the poison's BITS at `index` (no arithmetic touches the value: a signalling NaN stays one)."""
    out = np.ascontiguousarray(a, dtype=np.float32).copy()
    out.view(np.uint32)[index] = np.uint32(POISONS[name])
    return out


def classify(a) -> np.ndarray:
    a = np.asarray(a)
    cls = np.full(a.shape, FIN, np.int8)
    cls[np.isposinf(a)] = PINF
    cls[np.isneginf(a)] = NINF
    cls[np.isnan(a)] = NAN
    return cls


class T:
    """values (float64) + dependence mask (bool) + the sign of every NaN (`neg`: True where a NaN is sign-SET), same shape.  The sign
    matters only to the documented exception (`wave=True` below); the reference's own semantics never look at it."""

    def __init__(self, v, d=None, neg=None):
        self.v = np.asarray(v, dtype=np.float64)
        self.d = np.zeros(self.v.shape, bool) if d is None else np.asarray(d, bool)
        self.neg = np.zeros(self.v.shape, bool) if neg is None else np.asarray(neg, bool)
        assert self.d.shape == self.v.shape and self.neg.shape == self.v.shape

    @staticmethod
    def poisoned(a, index) -> "T":
        """The fp32 array `a` (poison already in place at `index`) with that one element marked."""
        a = np.ascontiguousarray(a, dtype=np.float32)
        with np.errstate(invalid="ignore"):                          # (widening a signalling NaN raises the invalid flag)
            t = T(a.astype(np.float64))                              # float32 -> float64 keeps NaN-ness and the infinities
        t.d[index] = True
        t.neg = np.isnan(a) & ((a.view(np.uint32) >> 31) == 1)
        return t


def verdict(t: T):
    """-> (class per element, float64 value (meaningful where the class is FIN), dependence mask)."""
    return classify(t.v), t.v, t.d


def relu(v):
    with np.errstate(all="ignore"):
        return np.where(np.isnan(v), v, np.maximum(v, 0.0))


# The documented exception (include/captra_hip.h, "NaN / Inf contract"): the register-resident wave kernels (csrc/wave_mlp.h,
# csrc/sa_pipe.hip) keep their one-instruction ReLU and pools on the bit pattern as a SIGNED integer.  A sign-clear NaN is the
# largest such integer and behaves as in the reference; a sign-SET NaN is a negative integer: 0 behind the ReLU, the loser of the
# pool.  Which NaNs are sign-set is measured on gfx950 (tests/test_f32_edges_gpu.py::test_nan_generated_inside_the_mfma): the fp32
# MFMA hands an input NaN on with its sign and payload (quieted) under weights of either sign, and a NaN it generates itself (Inf - Inf,
# 0 * Inf) is 0xFFC00000, sign-set.  `wave=True` restates exactly that.
def relu_wave(t: T) -> T:
    dropped = np.isnan(t.v) & t.neg
    return T(np.where(dropped, 0.0, relu(t.v)), t.d, t.neg & ~dropped)


def dense(t: T, w, b, act_relu: bool, wave: bool = False) -> T:
    """act(W x + b) over axis 1 of t (B, cin, *): w (cin, cout), b (cout).  The sum runs over exactly the cin channels, one product
    at a time (no BLAS: a library may skip a zero operand, and 0 * Inf = NaN is the point).  `wave`: the ReLU is relu_wave."""
    w = np.asarray(w, dtype=np.float64)
    cin, cout = w.shape
    assert t.v.shape[1] == cin
    tail = t.v.shape[2:]
    one = (1, cout) + (1,) * len(tail)
    y = np.broadcast_to(np.asarray(b, dtype=np.float64).reshape(one), (t.v.shape[0], cout) + tail).copy()
    with np.errstate(all="ignore"):
        for k in range(cin):
            y += w[k].reshape(one) * t.v[:, k:k + 1]
    d = np.broadcast_to(t.d.any(axis=1, keepdims=True), y.shape).copy()
    # the sign of an output NaN: the input NaNs' where the position holds any (one poison: they all share it), else generated: sign-set
    nan_in = np.isnan(t.v)
    has, neg_in, pos_in = nan_in.any(axis=1, keepdims=True), (nan_in & t.neg).any(axis=1, keepdims=True), (nan_in & ~t.neg).any(axis=1, keepdims=True)
    assert not (neg_in & pos_in).any(), "NaNs of both signs meet in one dot product: the hardware's choice has not been measured"
    out = T(y, d, np.isnan(y) & np.where(has, neg_in, True))
    if not act_relu:
        return out
    return relu_wave(out) if wave else T(relu(y), d, out.neg)


def chain(t: T, layers, acts, wave: bool = False) -> T:
    """`wave`: the one-launch chain kernels -- the inner ReLUs are relu_wave, the last layer's activation is the reference's (it is
    applied by the store epilogue's apply_act)."""
    for i, ((w, b), a) in enumerate(zip(layers, acts)):
        t = dense(t, w, b, bool(a), wave=wave and i < len(layers) - 1)
    return t


def concat(t1: T, t2: T) -> T:
    """cat along the channels; a (B, c2, 1) second source is one vector per cloud, read at every position."""
    if t2.v.shape[2:] != t1.v.shape[2:]:
        shape = (t2.v.shape[0], t2.v.shape[1]) + t1.v.shape[2:]
        t2 = T(np.broadcast_to(t2.v, shape), np.broadcast_to(t2.d, shape), np.broadcast_to(t2.neg, shape))
    return T(np.concatenate([t1.v, t2.v], axis=1), np.concatenate([t1.d, t2.d], axis=1), np.concatenate([t1.neg, t2.neg], axis=1))


def max_last(t: T, keepdims: bool = False) -> T:
    """torch.max(x, -1)[0] / F.max_pool2d(x, [1, K]): np.max hands a NaN on, whatever its sign."""
    with np.errstate(all="ignore"):
        return T(np.max(t.v, axis=-1, keepdims=keepdims), t.d.any(axis=-1, keepdims=keepdims))


def affine_relu(t: T, ab) -> T:
    """relu(a x + b) with per-(cloud, channel) coefficients ab (B, C, 2) given as DATA (they carry no dependence of their own)."""
    ab = np.asarray(ab, dtype=np.float64)
    with np.errstate(all="ignore"):
        return T(relu(ab[:, :, 0:1] * t.v + ab[:, :, 1:2]), t.d)


def group_norm(t: T, groups: int, gamma, beta, eps: float, act_relu: bool) -> T:
    """nn.GroupNorm(groups, C) [+ ReLU] over (B, C, N): biased variance over the group's C / groups * N values."""
    B, C, N = t.v.shape
    g = t.v.reshape(B, groups, -1)
    with np.errstate(all="ignore"):
        mean = g.mean(-1, keepdims=True)
        var = ((g - mean) ** 2).mean(-1, keepdims=True)
        y = ((g - mean) / np.sqrt(var + eps)).reshape(B, C, N)
        y = y * np.asarray(gamma, np.float64)[None, :, None] + np.asarray(beta, np.float64)[None, :, None]
    d = np.broadcast_to(t.d.reshape(B, groups, -1).any(-1, keepdims=True), g.shape).reshape(B, C, N).copy()
    return T(relu(y) if act_relu else y, d)


def tile_stats(t: T, tile: int) -> T:
    """(sum, sum of squares) of every `tile` consecutive positions (the last tile ragged) of (B, C, L) -> (B, C, T, 2)."""
    B, C, L = t.v.shape
    nt = (L + tile - 1) // tile
    v = np.zeros((B, C, nt * tile))
    d = np.zeros((B, C, nt * tile), bool)
    v[..., :L], d[..., :L] = t.v, t.d
    v, d = v.reshape(B, C, nt, tile), d.reshape(B, C, nt, tile)
    with np.errstate(all="ignore"):
        s = np.stack([v.sum(-1), (v * v).sum(-1)], axis=-1)
    return T(s, np.broadcast_to(d.any(-1)[..., None], s.shape).copy())


def gn_coefficients(stats: T, groups: int, gamma, beta, eps: float, n: int) -> T:
    """The (a, b) of GroupNorm(x) = a x + b from the partial statistics (B, C, T, 2) over n positions."""
    B, C = stats.v.shape[:2]
    cpg = C // groups
    with np.errstate(all="ignore"):
        sm = stats.v[..., 0].sum(-1).reshape(B, groups, cpg).sum(-1, keepdims=True)
        sq = stats.v[..., 1].sum(-1).reshape(B, groups, cpg).sum(-1, keepdims=True)
        mean = sm / (cpg * n)
        var = sq / (cpg * n) - mean * mean
        rstd = 1.0 / np.sqrt(np.maximum(var, 0.0) + eps)
        a = np.asarray(gamma, np.float64).reshape(1, groups, cpg) * rstd
        b = np.asarray(beta, np.float64).reshape(1, groups, cpg) - mean * a
    d = np.broadcast_to(stats.d.reshape(B, groups, -1).any(-1)[:, :, None], (B, groups, cpg))
    return T(np.stack([a.reshape(B, C), b.reshape(B, C)], -1), np.stack([d.reshape(B, C)] * 2, -1))


def sa_group(feat: T | None, xyz_cn: T, new_xyz, idx) -> T:
    """gather by idx (B, M, K), subtract the centre from the coordinates, cat [feat, xyz] -> (B, cfeat + 3, M, K)."""
    B, M, K = idx.shape
    new_xyz = np.asarray(new_xyz, dtype=np.float64)
    bi = np.arange(B)[:, None, None]
    take = lambda a: np.moveaxis(a[bi, :, idx], 3, 1)           # noqa: E731
    with np.errstate(all="ignore"):
        gx = T(take(xyz_cn.v) - np.moveaxis(new_xyz, 2, 1)[:, :, :, None], take(xyz_cn.d), take(xyz_cn.neg))
    return gx if feat is None else concat(T(take(feat.v), take(feat.d), take(feat.neg)), gx)


def sa_scale(feat: T | None, xyz_cn: T, new_xyz, idx, layers, wave: bool = False) -> T:
    """One set-abstraction scale: group -> conv + ReLU per layer -> max over the K neighbours -> (B, c_last, M).  `wave`: the
    register-resident kernels -- every ReLU is relu_wave (the last one is the pool's: a sign-set NaN loses the signed-integer max)."""
    g = sa_group(feat, xyz_cn, new_xyz, idx)
    for w, b in layers:
        g = dense(g, w, b, True, wave=wave)
    return max_last(g)


def interp_concat(skip: T | None, feat_known: T, idx, weight) -> T:
    """cat([skip, sum_j weight_j feat_known[:, idx_j]]): idx, weight (B, N, 3) given as data."""
    B, N, _ = idx.shape
    bi = np.arange(B)[:, None, None]
    g = np.moveaxis(feat_known.v[bi, :, idx], 3, 1)                  # (B, c2, N, 3)
    gd = np.moveaxis(feat_known.d[bi, :, idx], 3, 1)
    with np.errstate(all="ignore"):
        v = (g * np.asarray(weight, np.float64)[:, None]).sum(-1)
    out = T(v, gd.any(-1))
    return out if skip is None else concat(skip, out)


# ---- weights under which the reference alone shows every class -----------------------------------------------------------------------
def poisoned_layers(rng, dims, row: int):
    """fp32 layers [(w (cin, cout), b)] of widths `dims` for a poison in input channel `row`.
    One layer: the poisoned row's weights are a third strictly positive, a third strictly negative, a third exactly zero, so that
    +-Inf gives +-Inf, -+Inf (0 behind a ReLU: a finite dependent output) and NaN.  Several layers: the poisoned row of the first
    and every inner layer strictly positive (+Inf stays +Inf, -Inf is 0 behind the first ReLU and everything behind it finite), the
    last layer's columns a third strictly positive (+Inf), a third strictly negative (-Inf, or 0 behind a ReLU) and a third mixed
    (Inf - Inf = NaN)."""
    n = len(dims) - 1
    layers = []
    for i in range(n):
        cin, cout = dims[i], dims[i + 1]
        w = rng.standard_normal((cin, cout)) / np.sqrt(cin)
        third = np.arange(cout) % 3
        if n == 1:
            w[row] = np.where(third == 0, np.abs(w[row]) + 0.05, np.where(third == 1, -np.abs(w[row]) - 0.05, 0.0))
        elif i == 0:
            w[row] = np.abs(w[row]) + 0.05
        elif i < n - 1:
            w = np.abs(w) + 0.01
        else:
            w = np.where(third[None, :] == 0, np.abs(w) + 0.01, np.where(third[None, :] == 1, -np.abs(w) - 0.01, w))
        layers.append((w.astype(np.float32), rng.standard_normal(cout).astype(np.float32)))
    return layers


# ---- comparing a result with a verdict ------------------------------------------------------------------------------------------------
def class_mismatches(got, cls) -> int:
    return int((classify(got) != cls).sum())


def describe(cls, dep) -> str:
    """'dep 96 of 7392: finite 32, +Inf 32, NaN 32' -- what a test prints before it asserts."""
    parts = [f"{CLASS_NAMES[c]} {int(((cls == c) & dep).sum())}" for c in (FIN, PINF, NINF, NAN) if ((cls == c) & dep).any()]
    return f"dep {int(dep.sum())} of {dep.size}: " + ", ".join(parts)


def non_vacuous(cls, dep) -> dict:
    """The facts the non-vacuity conditions are stated on."""
    return {"dep": bool(dep.any()), "indep": bool((~dep).any()), "nan": bool((cls == NAN).any()), "pinf": bool((cls == PINF).any()),
            "finite_dep": bool(((cls == FIN) & dep).any()), "indep_finite": bool((cls[~dep] == FIN).all())}


# ---- the cases both test files run: the smallest shapes that still take every variant of each entry point ------------------------------
DENSE_CASES = [(7, 40, 77, 3), (130, 96, 75, 3)]                       # (cin, cout, L, B): pointwise_mlp
TWO_SOURCE_CASES = [(3, 70, 96, 75, 3, False), (40, 96, 128, 77, 3, True)]   # (c, c2, cout, L, B, one vector per cloud): pointwise_mlp2
CHAIN_CASES = [(100, 256, 3), (134, 77, 3)]                            # (c0, L, B): mlp_chain3, widths 128
TAIL_CASES = [(134, 2, 3, 77, 3)]                                      # (c0, seg, nocs, L, B): coord_tail
MAX_CASES = [(16, 40, 37, 32, 3), (96, 128, 5, 128, 3)]                # (cin, cout, M, K, B): mlp_max
GROUP_MLP_CASES = [(5, 40, 300, 37, 32, 3)]                            # (cfeat, cout, N, M, K, B): sa_group_mlp
SA_CASES = [(0, (32, 32, 64), 700, 41, 32, 3), (3, (64, 96, 128), 700, 41, 128, 3), (320, (128, 196, 256), 200, 5, 64, 3)]
SA_PRE_CASES = [(320, (128, 128, 256), 512, 128, 64, 2)]               # (cfeat, chans, N, M, K, B)
GN_CASES = [(2, 8, 100, 4)]                                            # (B, C, N, groups): group_norm_relu
ROW_MAX_CASES = [(3, 5, 77), (3, 4, 128)]                              # (B, C, N): scalar and 16-byte loads
INTERP_CASES = [(3, 300, 7, 6, 5)]                                     # (B, N, S, c1, c2): fp_interpolate_concat


def case_rng(*parts):
    import zlib
    return np.random.default_rng(zlib.crc32(repr(parts).encode()))


def edge_positions(L: int, tile: int = 32):
    """Position 0, position L - 1 and the first position of the (ragged) last tile."""
    return [0, L - 1, (L - 1) // tile * tile]


def middle(B: int) -> int:
    """A cloud with both neighbours where the batch has three (else the last one)."""
    return B // 2


def sa_inputs(rng, cfeat, chans, N, M, K, B):
    """Points, centres and a neighbour list GIVEN by the test (dependence is defined by idx).  Point 0 of every cloud is named in no
    slot; point 1 only in PADDED slots (a centre with three found neighbours repeats its first one, as the ball query pads), point
    2 in the first slot of centre 0 and the last slot of centre M - 1; everything else random."""
    xyz_cn = (rng.random((B, 3, N)) - 0.5).astype(np.float32)
    feat = rng.standard_normal((B, cfeat, N)).astype(np.float32) if cfeat else None
    new_xyz = (rng.random((B, M, 3)) - 0.5).astype(np.float32)
    idx = rng.integers(3, N, (B, M, K)).astype(np.int32)
    mp = M // 2
    idx[:, mp, :3] = (1, 5, 6)
    idx[:, mp, 3:] = 1                                     # padded slots: the first neighbour again
    idx[:, 0, 0] = 2
    idx[:, M - 1, K - 1] = 2
    return xyz_cn, feat, new_xyz, idx


def sa_cases_with_poison_site(cases):
    """Every case with the poison in a coordinate, and in a feature channel where the scale has any."""
    return [c + (where,) for c in cases for where in ("feat", "xyz") if where == "xyz" or c[0] > 0]


SA_POINTS = {"first_and_last_slot": 2, "padded_slots_only": 1, "unnamed": 0}


def sa_scale_dependent_only(feat, xyz_cn, new_xyz, idx, layers, wave: bool = False) -> T:
    """sa_scale with the values computed for the DEPENDENT centres only (an independent output is finite and keeps the bits of the
    unpoisoned run, which the tests assert directly); the others hold 0."""
    g = sa_group(feat, xyz_cn, new_xyz, idx)
    depc = g.d.any(axis=(1, 3))                                        # (B, M)
    B, M = depc.shape
    c_last = layers[-1][0].shape[1]
    out = T(np.zeros((B, c_last, M)), np.broadcast_to(depc[:, None, :], (B, c_last, M)).copy())
    for b in range(B):
        ms = np.nonzero(depc[b])[0]
        if len(ms):
            t = T(g.v[b:b + 1][:, :, ms], g.d[b:b + 1][:, :, ms], g.neg[b:b + 1][:, :, ms])
            for w, bias in layers:
                t = dense(t, w, bias, True, wave=wave)
            out.v[b][:, ms] = max_last(t).v[0]
    return out
