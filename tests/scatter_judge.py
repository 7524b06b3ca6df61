"""Judge of the gather-gradient kernels (csrc/scatter_reduce.hip, the atomic fall-backs of group.hip / interpolate.hip): numpy only.

The three backward operators are one scatter:  d points[b][ch][i] (+)= sum over the positions p of cloud b with idx[b][p] == i of
term[b][ch][p],  term = grad_out[b][ch][p] (group, gather) or weight[b][p] * grad_out[b][ch][p // 3] (interp, p = 3 n + j).

Layout used by everything here: grad_out (B, c, row) fp32 with row = npos (group, gather) or npos / 3 (interp); idx (B, npos) int32
(the operators' (B, m, k) / (B, n, 3) / (B, npoints) lists flattened); weight (B, npos) fp32 or None; init / results (B, c, n_src).

This file holds what a device test of these kernels stands on, each piece proven by tests/test_scatter_judge_cpu.py:
  * `scatter64`: the scatter in float64, with the list length L and S = sum |term| of every output element;
  * `bound`: the derived fp32 error bound gamma_(L+2) * S;
  * `mirror32`: an fp32 mirror of the CSR kernels' order, with `mutate=` as the handle of the judge's own mutation tests;
  * `lattice`: integer-valued inputs on which every fp32 summation order is exact;
  * the index-list makers and the table of shapes (one row per route or edge of captra_scatter_reduce).
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

U = 2.0 ** -24                    # unit roundoff of fp32 (round to nearest)
TINY = 2.0 ** -149                # the smallest fp32 subnormal: the absolute slack of every bounded comparison
KINDS = ("group", "gather", "interp")
MUTATIONS = ("drop_last", "start_plus_one", "weight_j_swapped", "no_accumulate", "channel_stride_off_by_one")

# mirrors of the launcher's limits (scatter_reduce.hip), used to label routes and to predict the scratch size
CSR_MAX_SRC = 16384
LDS_ROW_CAP = 16384
MIN_CHANNELS = 8


# ------------------------------------------------------------------------------------------------------------ references
def _terms(kind, g_b, w_b, npos, dtype):
    """(c, npos) terms of one cloud in `dtype` (fp32: one rounding per product, as a build with -ffp-contract=off gives)."""
    if kind == "interp":
        col = np.arange(npos) // 3
        return g_b[:, col].astype(dtype) * w_b.astype(dtype)[None, :]
    return g_b.astype(dtype)


def _csr(idx_b, n_src):
    """Stable inversion of one cloud's list: (order, start, counts); every list ascending in position."""
    order = np.argsort(idx_b, kind="stable")
    counts = np.bincount(idx_b, minlength=n_src).astype(np.int64)
    return order, np.cumsum(counts) - counts, counts


def scatter64(kind, grad_out, idx, weight, n_src, init=None):
    """-> (ref (B,c,n_src) float64, L (B,n_src) int64, S (B,c,n_src) float64).  S = sum |term| of the element's list, plus |init| of
    the element when `init` is given: the final `+=` rounds relative to |init + sum| <= |init| + sum |term|, so the value the caller
    accumulates into counts as one more summand of the bound (it does not count in L: `bound` already allows for that addition)."""
    assert kind in KINDS
    g = np.asarray(grad_out, np.float32)
    idx = np.asarray(idx)
    B, c, _ = g.shape
    npos = idx.shape[1]
    ref = np.zeros((B, c, n_src), np.float64)
    S = np.zeros((B, c, n_src), np.float64)
    L = np.zeros((B, n_src), np.int64)
    for b in range(B):
        t = _terms(kind, g[b], None if weight is None else np.asarray(weight, np.float32)[b], npos, np.float64)
        order, start, counts = _csr(idx[b], n_src)
        L[b] = counts
        hit = counts > 0
        if hit.any():
            ts = t[:, order]
            ref[b][:, hit] = np.add.reduceat(ts, start[hit], axis=1)
            S[b][:, hit] = np.add.reduceat(np.abs(ts), start[hit], axis=1)
    if init is not None:
        init = np.asarray(init, np.float64)
        ref += init
        S += np.abs(init)
    return ref, L, S


def bound(L, S):
    """gamma_(L+2) * S, gamma_k = k u / (1 - k u), u = 2^-24.  Roundings on the way to one output element: one per product (no
    contraction into an fma), one per addition of a recursive fp32 sum of L terms in ANY order (L - 1 for the ordered CSR sum started
    from the first term, L for atomics onto the caller's value), one for the final `+=`: at most L + 2, each relative to a partial
    sum of magnitude <= S.  Derived, not measured; holds for the ordered sums and for float atomics alike."""
    k = (np.asarray(L, np.float64) + 2.0) * U
    return k / (1.0 - k) * np.asarray(S, np.float64)


def tolerance(L, S):
    """Absolute tolerance per element: L (B,n_src) broadcast over the channels of S (B,c,n_src)."""
    return bound(np.asarray(L)[:, None, :], S) + TINY


def mirror32(kind, grad_out, idx, weight, n_src, init=None, mutate=None):
    """fp32 mirror of the CSR kernels: every list summed in ascending position order starting from 0.f, the finished sum added to
    `init` (zeros when None).  mutate: one of MUTATIONS -- the defects the device tests must be able to see."""
    assert kind in KINDS and (mutate is None or mutate in MUTATIONS)
    g = np.ascontiguousarray(grad_out, np.float32)
    idx = np.asarray(idx)
    B, c, row = g.shape
    npos = idx.shape[1]
    if mutate == "channel_stride_off_by_one":           # channel ch >= 1 reads the row after its own (the last one of the tensor wraps)
        src = np.arange(B * c).reshape(B, c).copy()
        src[:, 1:] += 1
        g = g.reshape(B * c, row)[src % (B * c)]
    out = np.zeros((B, c, n_src), np.float32)
    for b in range(B):
        w = None
        if kind == "interp":
            w = np.asarray(weight, np.float32)[b]
            if mutate == "weight_j_swapped":
                w = w.reshape(-1, 3)[:, [1, 2, 0]].reshape(-1)
        t = _terms(kind, g[b], w, npos, np.float32)
        order, start, counts = _csr(idx[b], n_src)
        lo = 1 if mutate == "start_plus_one" else 0
        hi = counts - 1 if mutate == "drop_last" else counts
        acc = np.zeros((c, n_src), np.float32)
        for r in range(lo, int(hi.max(initial=0))):
            act = np.nonzero(hi > r)[0]
            acc[:, act] += t[:, order[start[act] + r]]
        out[b] = acc
    if init is None or mutate == "no_accumulate":
        return out
    return (np.asarray(init, np.float32) + out).astype(np.float32)


def lattice(kind, shape, rng):
    """Integer-valued inputs for shape = (B, c, row, n_src): (grad_out in {-4..4}, weight in {0.25, 0.5, 1} (B, 3 row) or None,
    init in {-3..3}).  Every partial sum is a multiple of 0.25 below 2^22: fp32 is exact in any order, so ordered sums and float
    atomics alike must reproduce float64 bit for bit."""
    B, c, row, n_src = shape
    g = rng.integers(-4, 5, (B, c, row)).astype(np.float32)
    w = rng.choice(np.array([0.25, 0.5, 1.0], np.float32), size=(B, 3 * row)) if kind == "interp" else None
    init = rng.integers(-3, 4, (B, c, n_src)).astype(np.float32)
    return g, w, init


# ------------------------------------------------------------------------------------------------------------ index lists
def ball_like(rng, n, m, k):
    """Index lists shaped like a ball query's: a few distinct neighbours per centre, padded with the first."""
    idx = np.empty((m, k), np.int32)
    for j in range(m):
        cnt = int(rng.integers(1, k + 1))
        hits = np.sort(rng.choice(n, size=min(cnt, n), replace=False)).astype(np.int32)
        idx[j, :len(hits)] = hits
        idx[j, len(hits):] = hits[0]
    return idx


def uniform(rng, n_src, npos):
    return rng.integers(0, n_src, npos).astype(np.int32)


def permutation(rng, n_src, npos):
    """npos == n_src: every list has length 1."""
    assert npos == n_src
    return rng.permutation(n_src).astype(np.int32)


def all_first(rng, n_src, npos):
    """One list holds every position: what a ball query's all-empty balls produce."""
    return np.zeros(npos, np.int32)


def all_last(rng, n_src, npos):
    return np.full(npos, n_src - 1, np.int32)


def sparse(rng, n_src, npos):
    """Only every 7th source point is referenced: most lists are empty (start[i] == start[i + 1])."""
    return (7 * rng.integers(0, (n_src + 6) // 7, npos)).astype(np.int32)


def long_first(rng, n_src, npos):
    """The first 2048 positions on source point 0, the rest spread: a long list inside a row too long for one list of its own."""
    idx = uniform(rng, n_src, npos)
    idx[:2048] = 0
    return idx


_FLAT_MAKERS = {"uniform": uniform, "permutation": permutation, "all_first": all_first, "all_last": all_last, "sparse": sparse,
                "long_first": long_first}


# ------------------------------------------------------------------------------------------------------------ shapes
class Run(NamedTuple):
    """One parametrised case: `dims` = (m, k) group, (n,) interp, (npoints,) gather; `lists` names the list maker ("nn": real
    3-nearest-neighbour lists); csr: the shape is inside the CSR path (else the hand-over to the atomic kernels)."""
    id: str
    kind: str
    B: int
    c: int
    n_src: int
    dims: tuple
    lists: str
    csr: bool

    @property
    def npos(self):
        return {"group": lambda d: d[0] * d[1], "interp": lambda d: 3 * d[0], "gather": lambda d: d[0]}[self.kind](self.dims)

    @property
    def row(self):
        return self.npos // 3 if self.kind == "interp" else self.npos

    @property
    def cpb(self):
        """Channels per workgroup of the LDS kernel, as the launcher picks them."""
        cpb = 1
        while -(-self.c // cpb) * self.B > 1024 and cpb < 16:
            cpb *= 2
        return cpb

    @property
    def route(self):
        """Label for reports: lds-cpb1 | lds-cpb>1 | nonlds-group | nonlds-interp | atomics-group | atomics-interp."""
        fam = "interp" if self.kind == "interp" else "group"
        if not self.csr:
            return f"atomics-{fam}"
        if self.row > LDS_ROW_CAP:
            return f"nonlds-{fam}"
        return "lds-cpb1" if self.cpb == 1 else "lds-cpb>1"

    @property
    def ws_bytes(self):
        return self.B * (self.n_src + 1 + self.npos) * 4 if self.csr else 0


# (B, c, n_src, m, k): npos = row = m k
GROUP_CASES = [
    ("lds-cpb1-float4", (2, 8, 64, 16, 8), True),
    ("lds-scalar-staging", (2, 9, 70, 7, 9), True),
    ("lds-cpb2-odd-c", (8, 129, 50, 8, 8), True),
    ("lds-cpb4-train-batch", (12, 320, 128, 16, 16), True),
    ("lds-cpb16-tail6", (8, 1030, 20, 4, 4), True),
    ("lds-row-cap", (1, 8, 300, 128, 128), True),
    ("nonlds-chan-tail", (2, 13, 257, 241, 68), True),
    ("nsrc1", (2, 8, 1, 33, 4), True),
    ("nsrc1023", (2, 8, 1023, 33, 4), True),
    ("nsrc1024", (2, 8, 1024, 33, 4), True),
    ("nsrc1025", (2, 8, 1025, 33, 4), True),
    ("nsrc16384", (2, 8, 16384, 33, 4), True),
    ("atomics-nsrc16385", (2, 8, 16385, 33, 4), False),
    ("atomics-c7", (2, 7, 64, 16, 8), False),
    ("one-position", (1, 8, 5, 1, 1), True),
]
# (B, c, n_src = m, n): npos = 3 n, row = n
INTERP_CASES = [
    ("lds-cpb1", (2, 8, 5, 12), True),
    ("lds-row-mod4", (2, 8, 5, 13), True),
    ("lds-cpb2", (8, 129, 30, 40), True),
    ("lds-cpb4", (12, 256, 128, 512), True),
    ("lds-row-cap", (1, 9, 50, 16384), True),
    ("nonlds-16385", (1, 9, 50, 16385), True),
    ("nonlds-16388", (1, 9, 50, 16388), True),
    ("m1", (2, 8, 1, 40), True),
    ("m2", (2, 8, 2, 40), True),
    ("m16384", (1, 8, 16384, 64), True),
    ("atomics-m16385", (1, 8, 16385, 64), False),
]
# (B, c, n_src, npoints)
GATHER_CASES = [
    ("lds", (2, 8, 100, 37), True),
    ("nonlds", (1, 8, 100, 16388), True),
    ("atomics-c7", (2, 7, 100, 37), False),
]
LONG_LIST = 2048      # positions of a single-list run: build_csr_kernel sorts a list in one thread, quadratic in the worst case


def _runs():
    runs = []

    def add(kind, name, B, c, n_src, dims, lists, csr):
        runs.append(Run(f"{kind}-{name}-{lists}", kind, B, c, n_src, tuple(dims), lists, csr))

    for name, (B, c, n_src, m, k), csr in GROUP_CASES:
        for lists in ("ball_like", "sparse"):
            add("group", name, B, c, n_src, (m, k), lists, csr)
        if name == "lds-cpb1-float4":
            add("group", name, B, c, m * k, (m, k), "permutation", csr)
            for lists in ("all_first", "all_last"):
                add("group", name, B, c, n_src, (m, k), lists, csr)
        if name == "nonlds-chan-tail":
            # one list of every position is capped at LONG_LIST positions, a row the LDS kernel takes: the non-LDS case's batch,
            # channel tail and n_src with m k = 2048 ...
            for lists in ("all_first", "all_last"):
                add("group", name + "-2048", B, c, n_src, (32, 64), lists, csr)
            # ... and the non-LDS kernel itself walks a 2048-position list next to spread ones
            add("group", name, B, c, n_src, (m, k), "long_first", csr)
    for name, (B, c, m, n), csr in INTERP_CASES:
        for lists in ("nn", "sparse"):
            add("interp", name, B, c, m, (n,), lists, csr)
        if name == "lds-cpb1":
            add("interp", name, B, c, 3 * n, (n,), "permutation", csr)
            for lists in ("all_first", "all_last"):
                add("interp", name, B, c, m, (n,), lists, csr)
        if name == "nonlds-16385":                       # (n = 682: 2046 positions, see the group cases)
            for lists in ("all_first", "all_last"):
                add("interp", "nonlds-682", B, c, m, (682,), lists, csr)
        if name.startswith("nonlds"):
            add("interp", name, B, c, m, (n,), "long_first", csr)
    for name, (B, c, n_src, npoints), csr in GATHER_CASES:
        for lists in ("uniform", "sparse"):
            add("gather", name, B, c, n_src, (npoints,), lists, csr)
        if name == "nonlds":
            for lists in ("all_first", "all_last"):
                add("gather", name + "-2048", B, c, n_src, (LONG_LIST,), lists, csr)
    return runs


RUNS = _runs()


def inverse_distance_weights(d2):
    """three_nn's squared distances -> the interpolation weights of the FP modules, fp32."""
    recip = 1.0 / (np.sqrt(d2) + 1e-8)
    return (recip / recip.sum(-1, keepdims=True)).astype(np.float32)


def make_lists(run, rng, three_nn=None):
    """-> (idx (B, npos) int32, weight (B, npos) fp32 inverse-distance weights or None).  Every cloud of the batch gets a list of
    its own (the constant makers excepted).  three_nn(unknown (B,n,3), known (B,m,3)) -> (squared distances, idx) serves "nn"."""
    B, n_src, npos = run.B, run.n_src, run.npos
    w = None
    if run.lists == "nn":
        n = run.dims[0]
        unknown = (rng.random((B, n, 3), dtype=np.float32) - 0.5).astype(np.float32)
        known = (rng.random((B, n_src, 3), dtype=np.float32) - 0.5).astype(np.float32)
        d2, idx = three_nn(unknown, known)
        return np.ascontiguousarray(idx.reshape(B, npos), np.int32), inverse_distance_weights(d2).reshape(B, npos)
    if run.lists == "ball_like":
        idx = np.stack([ball_like(rng, n_src, *run.dims).reshape(-1) for _ in range(B)])
    else:
        idx = np.stack([_FLAT_MAKERS[run.lists](rng, n_src, npos) for _ in range(B)])
    if run.kind == "interp":
        d2 = (rng.random((B, npos // 3, 3), dtype=np.float32) + 0.01).astype(np.float32) ** 2
        w = inverse_distance_weights(d2).reshape(B, npos)
    return idx.astype(np.int32), w
