"""Judge of the bf16 arithmetic (csrc/bf16_mlp.hip's header: y = act(b + sum_k bf16(w[k]) * bf16(x[k]))): numpy only, int64.

Weights are rounded once (RNE), every layer's input is rounded (RNE) when it becomes an operand, accumulation and bias are fp32, a
bf16 point-major output is the RNE rounding of the fp32 result, and the on-load GroupNorm operand is bf16(relu(fma(a, x, b))).
On integers all of this is deterministic, ties included: `forward` applies `rne` at exactly those places in int64 and asserts, per
output element, sum_k |bf16(w)| |bf16(h)| + |b| < 2^24 -- the condition under which every fp32 summation order gives the bits int64
gives (proven by tests/test_bf16_judge_cpu.py; that the bf16 MFMA accumulates such sums exactly is what tests/test_x6_edges_gpu.py
established on the MI355X).  The shared pieces (`bf16_rne`, `LatticeLayer`, `_sparse_cols`, `_select_layer`, `LIMIT`) are
tests/x6_judge.py's.

Lattice families (`lattice`): the layer `target` holds the family's weights, every other layer is a +-1 selection (+1 under a ReLU):
  S  nothing rounds: weights, inputs, hidden values and outputs are integers of at most 8 significant bits (|y| <= 255: also the
     small-output variant whose statistics stay integers below 2^24) -- pure data movement;
  T  the target's pre-activations take 9 to 11 bits, so the hand-over (or the bf16 store) rounds, ties of both parities included;
  W  weights of 9 to 12 bits and, for target 0, fp32 inputs of 9 to 12 bits (bits_w + bits_x <= 22, two non-zeros per column), ties
     among them: the pack-time rounding and the rounding of an fp32 input at load;
  G  (`affine_case`) a = +-2^e and an integer b per (cloud, channel): fma(a, x, b) is exact and takes 9 to 11 bits.
`Model` is the handle of the judge's own mutation tests: each field is one place where a kernel can round or move data wrongly.
"""
from __future__ import annotations

import dataclasses
from typing import Callable

import numpy as np

from tests.x6_judge import LIMIT, LatticeLayer, _odd_ints, _select_layer, _sparse_cols, act, bf16_rne  # noqa: F401

SMALL = 255                        # |every value| of family S: 8 significant bits, and 128 * 255^2 < 2^24


def _f32(v):
    v = np.asarray(v, np.int64)
    assert np.abs(v).max(initial=0) < LIMIT
    return v.astype(np.float32)


def rne(v):
    """int64 -> int64: the nearest bf16, ties to even (the contract's rounding)."""
    return bf16_rne(_f32(v)).astype(np.int64)


def rtz(v):
    """Mutation: truncation (the low 16 bits of the fp32 pattern dropped)."""
    u = _f32(v).view(np.uint32) & np.uint32(0xFFFF0000)
    return u.view(np.float32).astype(np.int64)


def rhu(v):
    """Mutation: round half up in magnitude (add half an ulp, truncate)."""
    u = (_f32(v).view(np.uint32).astype(np.uint64) + 0x8000) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).astype(np.int64)


def ident(v):
    """Mutation: no rounding."""
    return np.asarray(v, np.int64)


def shares(v):
    """Of the integers v, as fractions of ALL elements: exact ties, ties that round down / up to even, inexact non-ties."""
    u = _f32(v).view(np.uint32)
    frac, odd = u & 0xFFFF, ((u >> 16) & 1).astype(bool)
    tie = frac == 0x8000
    n = float(max(u.size, 1))
    return {"tie": tie.sum() / n, "down": (tie & ~odd).sum() / n, "up": (tie & odd).sum() / n, "inexact": ((frac != 0) & ~tie).sum() / n}


def assert_shares(v, what=""):
    """The issue's conditions on a family whose values must round: >= 5 % ties, >= 1 % of each parity, >= 25 % inexact non-ties."""
    s = shares(v)
    assert s["tie"] >= 0.05 and s["down"] >= 0.01 and s["up"] >= 0.01 and s["inexact"] >= 0.25, (what, s)
    return s


def _contract_affine(a, h, b):
    return rne(np.maximum(a * h + b, 0))


@dataclasses.dataclass(frozen=True)
class Model:
    """Where the arithmetic rounds.  The defaults are the contract; the CPU tests replace one field at a time."""
    pack: Callable = rne                   # weights, once
    load: Callable = rne                   # the fp32 input of the first layer
    handover: Callable = rne               # a hidden activation (behind its ReLU: RNE commutes with the ReLU, proven on the CPU)
    affine: Callable = _contract_affine    # (a, h, b) -> the operand of a layer that normalises on load


CONTRACT = Model()


def _apply(lay, vals, h, absolute=False):
    """W h + b on int64 with the given (rounded) weights, or |W| |h| + |b|."""
    bias = lay.bias
    if absolute:
        vals, h, bias = np.abs(vals), np.abs(h), np.abs(bias)
    y = np.zeros(h.shape[:-2] + (lay.cout, h.shape[-1]), np.int64)
    for j in range(lay.rows.shape[0]):
        y += np.take(h, lay.rows[j], axis=-2) * vals[j][:, None]
    return y + bias[:, None]


def forward(layers, x, relu, ab=None, model=CONTRACT):
    """x int64 (...,c0,L) through the layers; relu: one flag per layer; ab: None, or per layer None / (a, b) int64 arrays (...,cin)
    -- that layer's operand is bf16(relu(a h + b)) of the fp32 h in front of it.  Returns the fp32 results of ALL layers as int64;
    a bf16 store of one of them is `rne` of it."""
    outs, h = [], np.asarray(x, np.int64)
    assert np.abs(h).max(initial=0) < LIMIT
    for i, (lay, r) in enumerate(zip(layers, relu)):
        if ab is not None and ab[i] is not None:
            a, b = (np.asarray(t, np.int64)[..., None] for t in ab[i])
            assert np.abs(a * h).max(initial=0) + np.abs(b).max(initial=0) < LIMIT       # fma(a, x, b) is exact
            v = model.affine(a, h, b)
        else:
            v = (model.load if i == 0 else model.handover)(h)
        wq = model.pack(lay.vals)
        bound = int(_apply(lay, wq, v, absolute=True).max(initial=0))
        assert bound < LIMIT, ("lattice leaves the exact range", i, bound)
        h = act(_apply(lay, wq, v), r)
        outs.append(h)
    return outs


def forward_f32(layers, x, relu, ab=None, order="asc", rng=None):
    """The same chain in float32 numpy, one fmaf-free product and addition at a time in the given order of k ("asc", "desc", "perm"),
    starting from the bias -- what the GPU's fp32 accumulation does in SOME order.  Only for the judge's own proof (slow)."""
    outs, h = [], np.asarray(x, np.int64).astype(np.float32)
    for i, (lay, r) in enumerate(zip(layers, relu)):
        if ab is not None and ab[i] is not None:
            a, b = (np.asarray(t, np.float32)[..., None] for t in ab[i])
            v = bf16_rne(np.maximum((a * h + b).astype(np.float32), 0))
        else:
            v = bf16_rne(h)
        w = bf16_rne(lay.w)
        ks = np.arange(lay.cin)
        if order == "desc":
            ks = ks[::-1]
        elif order == "perm":
            ks = rng.permutation(lay.cin)
        y = np.broadcast_to(lay.b[:, None], h.shape[:-2] + (lay.cout, h.shape[-1])).astype(np.float32)
        for k in ks:
            if w[k].any():
                y = (y + (w[k][:, None] * v[..., k, :][..., None, :]).astype(np.float32)).astype(np.float32)
        h = np.maximum(y, 0) if r else y
        outs.append(h)
    return outs


# ---- lattices -------------------------------------------------------------------------------------------------------------------------
def _signs(rng, shape, p_neg=0.5):
    return np.where(rng.random(shape) < p_neg, -1, 1).astype(np.int64)


def _rounding_ints(rng, shape, bits_hi, signed=True):
    """Odd integers of 9 .. bits_hi bits that all round, in fixed proportions however few there are (a layer of 134 -> 3 has six
    weights): a quarter 9-bit ties that go down to even (256 + 4 m + 1), a quarter 9-bit ties that go up (256 + 4 m + 3), half
    odd numbers of 10 .. bits_hi bits (inexact, no ties)."""
    n = int(np.prod(shape))
    cls = rng.permutation(np.arange(n) % 4)
    m = rng.integers(0, 64, n)
    big = _odd_ints(rng, (n,), 10, bits_hi, signed=False)
    out = np.where(cls == 0, 257 + 4 * m, np.where(cls == 1, 259 + 4 * m, big))
    if signed:
        out = out * _signs(rng, n)
    return out.reshape(shape)


def lattice(family, widths, target, rng, last_signed=True):
    """Layers of a fused kernel of widths (c0, ..., cn) with the family's weights in layer `target` (0-based) and selections elsewhere
    (signed only in a last layer without ReLU: `last_signed`), and the generator of its input: (layers, make_x), make_x(prefix, L) ->
    int64 (...,c0,L).  Behind a ReLU (target > 0) the target sees non-negative inputs only."""
    n = len(widths) - 1
    assert 0 <= target < n and family in "STW"
    cin_t, cout_t = widths[target], widths[target + 1]
    sg = target == 0
    wide_w = bool(rng.integers(0, 2))                    # family W: which side takes up to 12 bits
    if family == "S":
        nnz = min(cin_t, max(4, -(-cin_t // cout_t)))   # every input channel is read by some column
        wmax = 3 if 3 * nnz + 16 <= SMALL else 1
        lim = (SMALL - 16) // (wmax * nnz)
        assert lim >= 1, (cin_t, cout_t)
    elif family == "T":
        nnz = min(cin_t, 3)
    else:
        nnz = min(cin_t, 2)
    layers = []
    for i in range(n):
        cin, cout = widths[i], widths[i + 1]
        if i != target:
            layers.append(_select_layer(rng, cin, cout, signed=(last_signed and i == n - 1)))
            continue
        rows = _sparse_cols(rng, cin, cout, nnz)
        if family == "S":
            vals = rng.integers(1, wmax + 1, (nnz, cout)) * _signs(rng, (nnz, cout))
            bias = rng.integers(-16, 17, cout)
        elif family == "T":
            # |sum| <= 3 * 3 * 127 = 1143, bias 300 .. 900: most pre-activations are positive integers of 9 to 11 bits
            vals = rng.integers(1, 4, (nnz, cout)) * _signs(rng, (nnz, cout), 0.3)
            bias = rng.integers(300, 901, cout)
        else:
            vals = _rounding_ints(rng, (nnz, cout), 12 if wide_w or not sg else 10)
            bias = rng.integers(-(1 << 12), 1 << 12, cout)
        layers.append(LatticeLayer(cin, cout, rows, vals, bias))

    def make_x(prefix, L):
        shape = tuple(prefix) + (widths[0], L)
        if family == "S":
            return rng.integers(-lim if sg else 0, lim + 1, shape)
        if family == "T":
            return rng.integers(-127 if sg else 0, 128, shape)
        if sg:
            return _rounding_ints(rng, shape, 10 if wide_w else 12)
        return rng.integers(0, 256, shape)                # (behind a selection: 8 bits, nothing rounds on the way to the target)

    return layers, make_x


def affine_case(rng, prefix, cin, L, small=False):
    """Family G: x int64 (...,cin,L) of at most 8 bits (what a bf16 tensor holds), a = +-2^e (e = 0, 1, 2) and an integer b per
    (cloud, channel) -> (x, a, b) with fma(a, x, b) of 9 to 11 bits, about half the coefficients negative.  small: |a x + b| <= 31
    instead (for the statistics epilogues: nothing rounds)."""
    shape = tuple(prefix) + (cin,)
    if small:
        x = rng.integers(-7, 8, shape + (L,))
        a = (1 << rng.integers(0, 2, shape)) * _signs(rng, shape)
        b = rng.integers(-8, 17, shape)
        return x, a, b
    x = rng.integers(-255, 256, shape + (L,))
    a = (1 << rng.integers(0, 3, shape)) * _signs(rng, shape)
    b = rng.integers(400, 1000, shape)
    return x, a, b


def affine_operand(x, a, b):
    """What family G hands to `assert_shares`: relu(a x + b), the values that the contract rounds."""
    return np.maximum(np.asarray(a, np.int64)[..., None] * x + np.asarray(b, np.int64)[..., None], 0)


def dense_small_layer(rng, cin, cout, nnz=2, wmax=2):
    """A layer of small integer weights (nnz per column, |w| <= wmax, |bias| <= 16) behind family G's operand or for the heads."""
    nnz = min(cin, nnz)
    rows = _sparse_cols(rng, cin, cout, nnz)
    vals = rng.integers(1, wmax + 1, (nnz, cout)) * _signs(rng, (nnz, cout))
    return LatticeLayer(cin, cout, rows, vals, rng.integers(-16, 17, cout))


# ---- data-movement mutations (family S) ----------------------------------------------------------------------------------------------
def swap_channels(x, k0, k1):
    """Two input channels exchanged (two slots of a 16-slot block)."""
    x = np.array(x)
    x[..., [k0, k1], :] = x[..., [k1, k0], :]
    return x


def drop_last_kstep(x):
    """The input channels of the last 16-wide k-step read as zero."""
    x = np.array(x)
    x[..., (x.shape[-2] - 1) // 16 * 16:, :] = 0
    return x


def repeat_neighbour(y):
    """The last (ragged) position replaced by the one in front of it."""
    y = np.array(y)
    y[..., -1] = y[..., -2]
    return y


def pool(y, K, skip_last=False):
    """(...,c,M*K) -> (...,c,M): the max over each centre's K neighbours (mutation: without the last one)."""
    g = y.reshape(y.shape[:-1] + (y.shape[-1] // K, K))
    return (g[..., :-1] if skip_last else g).max(-1)
