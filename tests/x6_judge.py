"""Judge of the f32x6 arithmetic (include/captra_hip.h "f32x6"): numpy only, float64 / int64.

A layer in the mode is y = act(b + sum_k [w0 x0 + w0 x1 + w1 x0 + w1 x1 + w0 x2 + w2 x0]_k) on the RNE bf16 three-way splits of both
operands.  This file holds what the device tests (tests/test_x6_edges_gpu.py) stand on, each piece proven by
tests/test_x6_judge_cpu.py:
  * `split3`: the split itself;
  * `x6_layer_model`: the kept products summed in float64, with `keep` as the handle of the judge's own mutation tests;
  * probe values: fp32 numbers for which every kept product of every pair is >= 32 * 2^-24 |w x| (one product at a time);
  * integer lattices A / B / C: weights and inputs of whole fused kernels whose every piece, product and partial sum is an integer
    below 2^24 -- every fp32 summation order gives the same bits, int64 gives the answer;
  * power-of-two rescaling per input / output channel.
"""
from __future__ import annotations

import itertools

import numpy as np

U = 2.0 ** -24                                                    # unit of every bound here: half an fp32 ulp, relative
ALL_SIX = ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0))        # (piece of w, piece of x)
SWAP_X12 = ((0, 0), (0, 2), (1, 0), (1, 2), (0, 1), (2, 0))       # a kernel that reads x1 where x2 belongs and the other way round
SWAP_W12 = ((0, 0), (2, 0), (0, 1), (2, 1), (1, 0), (0, 2))       # the same on the weights' side
PROBE_TOL = 8                                                     # in U: three dropped products + five fp32 additions
PROBE_SENS = 32                                                   # in U: the smallest kept product of a probe pair


def bf16_rne(v):
    """fp32 -> the nearest bf16 (ties to even) as fp32; finite inputs."""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(v))


def split3(v):
    """v fp32 -> (v0, v1, v2) fp32 arrays holding bf16 values: v0 = bf16(v), v1 = bf16(v - v0), v2 = bf16(v - v0 - v1)."""
    v = np.asarray(v, dtype=np.float32)
    v0 = bf16_rne(v)
    r1 = (v - v0).astype(np.float32)
    v1 = bf16_rne(r1)
    v2 = bf16_rne((r1 - v1).astype(np.float32))
    return v0, v1, v2


def x6_layer_model(w, x, b=None, keep=ALL_SIX):
    """The kept products of one layer summed in float64: w (cin,cout), x (...,cin,L) fp32, b (cout) or None -> (...,cout,L) float64
    (no activation).  keep: the (w piece, x piece) pairs that enter."""
    ws = [p.astype(np.float64) for p in split3(w)]
    xs = [p.astype(np.float64) for p in split3(x)]
    y = 0.0
    for i in range(3):
        js = [j for (ii, j) in keep if ii == i]
        if js:
            y = y + np.matmul(ws[i].T, sum(xs[j] for j in js))
    if b is not None:
        y = y + np.asarray(b, np.float64)[:, None]
    return y


def act(y, relu):
    return np.maximum(y, 0) if relu else y


# ---- probe values ---------------------------------------------------------------------------------------------------------------
# |v1| >= 2^-9.5 |v| and |v2| >= 2^-19 |v|, each with a margin of (1 + 2^-7): |v0| >= (1 - 2^-8) |v| (half a bf16 ulp), so for ANY two
# accepted numbers w0 x2, w2 x0 >= (1 - 2^-8)(1 + 2^-7) 2^-19 |w x| >= 32 U |w x|, w1 x1 >= 2^-19 |w x|, the others are larger still.
_P1 = 2.0 ** -9.5 * (1 + 2.0 ** -7)
_P2 = 2.0 ** -19 * (1 + 2.0 ** -7)


def is_probe(v):
    v = np.asarray(v, np.float32)
    _, v1, v2 = split3(v)
    a = np.abs(v.astype(np.float64))
    return (a > 0) & (np.abs(v1) >= _P1 * a) & (np.abs(v2) >= _P2 * a)


def probe_values(rng, shape, emin=-2, emax=2, signed=True):
    """fp32 numbers of random mantissa, exponent in [emin, emax] and (signed) random sign that pass `is_probe`."""
    n = int(np.prod(shape))
    out = np.empty(0, np.float32)
    while out.size < n:
        m = (1.0 + rng.random(4 * n + 64)).astype(np.float32)
        out = np.concatenate([out, m[is_probe(m)]])
    out = out[:n] * np.exp2(rng.integers(emin, emax + 1, n)).astype(np.float32)
    if signed:
        out = out * rng.choice(np.float32([-1, 1]), n)
    return out.reshape(shape).astype(np.float32)


def six_products(w, x, keep=ALL_SIX):
    """The kept products of scalar pairs, float64, shape (len(keep),) + w.shape."""
    ws, xs = split3(w), split3(x)
    return np.stack([ws[i].astype(np.float64) * xs[j].astype(np.float64) for i, j in keep])


def worst_order_error(w, x):
    """max over pairs and over all 720 orders of |fp32 sum of the six products - w x| / |w x|, in U."""
    p = six_products(w, x).astype(np.float32)                     # a product of two bf16 numbers is exact in fp32
    exact = np.asarray(w, np.float64) * np.asarray(x, np.float64)
    worst = 0.0
    for order in itertools.permutations(range(6)):
        s = np.zeros_like(p[0])
        for i in order:
            s = (s + p[i]).astype(np.float32)
        worst = max(worst, float((np.abs(s.astype(np.float64) - exact) / np.abs(exact)).max()))
    return worst / U


# ---- power-of-two "permutation" layers (pass a value on within 2 U: x = x0 + x1 + x2 times one piece, two fp32 additions) ---------
def pow2_perm(rng, cin, cout, emin=-1, emax=1, negate=True):
    """(cin,cout) fp32 with one non-zero +-2^e per ROW where cout >= cin (every input channel goes to one output channel of its own),
    else one per column; returns (w, src) with src[c] = the input channel of output c, or -1."""
    w = np.zeros((cin, cout), np.float32)
    src = np.full(cout, -1)
    if cout >= cin:
        dst = rng.permutation(cout)[:cin]
        src[dst] = np.arange(cin)
    else:
        src[:] = rng.permutation(cin)[:cout]
    cs = np.nonzero(src >= 0)[0]
    w[src[cs], cs] = np.exp2(rng.integers(emin, emax + 1, cs.size)) * (rng.choice([-1.0, 1.0], cs.size) if negate else 1.0)
    return w, src


# ---- integer lattices -----------------------------------------------------------------------------------------------------------
LIMIT = 1 << 24


def _odd_ints(rng, shape, bits_lo, bits_hi, signed=True, need_piece=None):
    """Odd integers of bit length in [bits_lo, bits_hi] (so: that many significant bits); need_piece = 1 / 2: piece v1 / v2 non-zero."""
    n = int(np.prod(shape))
    out = np.empty(0, np.int64)
    while out.size < n:
        bl = rng.integers(bits_lo, bits_hi + 1, 2 * n + 16)
        v = (np.int64(1) << (bl - 1)) | rng.integers(0, np.int64(1) << (bl - 1), 2 * n + 16) | 1
        if need_piece:
            v = v[split3(v.astype(np.float32))[need_piece] != 0]
        out = np.concatenate([out, v])
    out = out[:n]
    if signed:
        out = out * rng.choice(np.int64([-1, 1]), n)
    return out.reshape(shape)


def _sparse_cols(rng, cin, cout, nnz):
    """rows (nnz,cout): for every column `nnz` distinct input channels, consecutive numbers under a random permutation of the
    channels; every input channel is used by some column when nnz * cout >= cin."""
    assert nnz <= cin
    perm = rng.permutation(cin)
    return perm[(np.arange(cout)[None, :] * nnz + np.arange(nnz)[:, None] + int(rng.integers(0, cin))) % cin]


class LatticeLayer:
    """One layer with integer weights: rows / vals (nnz,cout) int64, bias (cout) int64; `w` the dense (cin,cout) fp32."""

    def __init__(self, cin, cout, rows, vals, bias):
        self.cin, self.cout, self.rows, self.vals, self.bias = cin, cout, rows, vals.astype(np.int64), bias.astype(np.int64)
        self.w = np.zeros((cin, cout), np.float32)
        self.w[rows, np.arange(cout)[None, :]] = vals
        self.b = bias.astype(np.float32)

    def apply_int(self, h, absolute=False):
        """h (...,cin,L) int64 -> (...,cout,L) int64: W h + b, or |W| |h| + |b| (the bound on every partial sum)."""
        v, bias = (np.abs(self.vals), np.abs(self.bias)) if absolute else (self.vals, self.bias)
        if absolute:
            h = np.abs(h)
        y = np.zeros(h.shape[:-2] + (self.cout, h.shape[-1]), np.int64)
        for j in range(self.rows.shape[0]):
            y += np.take(h, self.rows[j], axis=-2) * v[j][:, None]
        return y + bias[:, None]


def _select_layer(rng, cin, cout, signed):
    """Selection: every output channel copies one input channel (integers stay the integers they are), times +-1 when `signed`."""
    rows = _sparse_cols(rng, cin, cout, 1)
    vals = rng.choice(np.int64([-1, 1]), (1, cout)) if signed else np.ones((1, cout), np.int64)
    return LatticeLayer(cin, cout, rows, vals, np.zeros(cout, np.int64))


def lattice(family, widths, target, rng, out_max=None):
    """Layers of a fused kernel of widths (c0, c1, ..., cn) whose layer `target` holds the family's weights and whose other layers are
    signed selections, plus the value generator of its input: returns (layers, make_x) with make_x(shape_prefix, L) -> int64 array
    (...,c0,L).  Family "A": 9-12 significant bits on both sides (bits_w + bits_x = 21 per input channel), four non-zeros per column --
    w0 x0, w0 x1, w1 x0, w1 x1 all matter, every third piece is zero.  "B": x of 17-20 bits (x2 != 0), w of <= 3 bits, two per
    column: w0 x2.  "C": the mirror image, w2 x0.  out_max: keep |outputs| of the target layer <= out_max instead (small weights and
    inputs; for statistics that must stay integers below 2^24) -- then the family only names the sparsity."""
    n = len(widths) - 1
    assert 0 <= target < n and family in "ABC"
    bx_max = int(rng.integers(9, 13))                                       # family A: x of 9..bx_max bits, w of 9..21 - bx_max
    layers = []
    for i in range(n):
        cin, cout = widths[i], widths[i + 1]
        if i != target:
            layers.append(_select_layer(rng, cin, cout, signed=(i == n - 1)))     # (+1 under a ReLU: nothing dies on the way)
            continue
        nnz = min(4 if family == "A" else 2, cin)
        rows = _sparse_cols(rng, cin, cout, nnz)
        if out_max is not None:
            vals = rng.integers(1, 4, (nnz, cout)) * rng.choice(np.int64([-1, 1]), (nnz, cout))
            bias = rng.integers(-3, 4, cout)
        elif family == "A":
            vals = _odd_ints(rng, (nnz, cout), 9, 21 - bx_max, need_piece=1)
            bias = rng.integers(-(1 << 12), 1 << 12, cout)
        elif family == "B":
            vals = rng.integers(1, 8, (nnz, cout)) * rng.choice(np.int64([-1, 1]), (nnz, cout))
            bias = rng.integers(-(1 << 20), 1 << 20, cout)
        else:
            vals = _odd_ints(rng, (nnz, cout), 17, 20, need_piece=2)
            bias = rng.integers(-(1 << 20), 1 << 20, cout)
        layers.append(LatticeLayer(cin, cout, rows, vals, bias))
    c0 = widths[0]
    nnz_t = min(4 if family == "A" else 2, widths[target])

    def make_x(prefix, L):
        shape = tuple(prefix) + (c0, L)
        sg = target == 0                                   # behind a ReLU a layer never sees a negative number
        if out_max is not None:
            lim = max(1, (out_max - 3) // (3 * nnz_t))
            return rng.integers(-lim if sg else 0, lim + 1, shape)
        if family == "A":
            return _odd_ints(rng, shape, 9, bx_max, signed=sg, need_piece=1)
        if family == "B":
            return _odd_ints(rng, shape, 17, 20, signed=sg, need_piece=2)
        return rng.integers(1, 8, shape) * (rng.choice(np.int64([-1, 1]), shape) if sg else 1)

    return layers, make_x


def lattice_forward(layers, x, relu, keep=None):
    """x int64 (...,c0,L) through the layers; relu: one flag per layer.  keep None: int64 arithmetic, with the assertion that
    sum |w| |h| + |b| < 2^24 after every layer (so every partial sum of every order is an fp32 integer).  keep given: the float64 model
    of the kept products instead (layer by layer, the hand-over rounded to fp32 as on the device).  Returns the outputs of ALL layers."""
    outs, h = [], np.asarray(x, np.int64)
    assert np.abs(h).max() < LIMIT
    for lay, r in zip(layers, relu):
        if keep is None:
            bound = int(lay.apply_int(h, absolute=True).max())
            assert bound < LIMIT, ("lattice leaves the exact range", bound)
            h = act(lay.apply_int(h), r)
            outs.append(h)
        else:
            y = act(x6_layer_model(lay.w, h.astype(np.float32), lay.b, keep), r)
            outs.append(y)
            h = y.astype(np.float32)
    return outs


# ---- power-of-two rescaling -----------------------------------------------------------------------------------------------------
def rescale_in(w, x, a):
    """x[..., k, :] <- 2^a_k x, w[k, :] <- 2^-a_k w (exact: powers of two, results asserted normal by the caller)."""
    s = np.exp2(np.asarray(a, np.float64))
    return (w.astype(np.float64) / s[:, None]).astype(np.float32), (x.astype(np.float64) * s[:, None]).astype(np.float32)


def rescale_out(w, b, g):
    """w[:, c], b[c] <- 2^g_c ."""
    s = np.exp2(np.asarray(g, np.float64))
    return (w.astype(np.float64) * s[None, :]).astype(np.float32), (b.astype(np.float64) * s).astype(np.float32)


def piece_range(*arrays):
    """(smallest |non-zero third piece|, largest |value|) over fp32 arrays: what the bit-exact rescaling claims are conditioned on."""
    lo, hi = np.inf, 0.0
    for v in arrays:
        v2 = np.abs(split3(v)[2].astype(np.float64))
        if (v2 > 0).any():
            lo = min(lo, float(v2[v2 > 0].min()))
        hi = max(hi, float(np.abs(v.astype(np.float64)).max()))
    return lo, hi
