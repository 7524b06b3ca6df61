"""The judge of the gather-gradient tests judged (tests/scatter_judge.py): no GPU.

For the index structure of every case of the judge's table (one row per route or edge of captra_scatter_reduce), at 8 channels:
  * the fp32 mirror of the CSR order stays within the derived bound of the float64 scatter on N(0,1) data, and equals it exactly on
    the integer lattices;
  * every mutation the mirror can carry -- a dropped last or first list entry, the weights of a neighbour triple rotated, an
    overwrite in place of the accumulation, a channel reading its neighbour's row -- turns the lattice comparison unequal AND puts at
    least one element outside the bound, on every case where it can matter.  A check that passes these is a check that bites.
The float data give interpolation strictly positive weights: with fewer than three known points the real inverse-distance weights
of the missing neighbours are exact zeros, and a dropped term of weight 0 is no defect any arithmetic check could see (the lattice,
whose weights are never 0, sees it on those lists too).
"""
import zlib

import numpy as np
import pytest

from oracle import ops as O
from tests import scatter_judge as J

C = 8     # enough elements that a list of ~6000 terms (gamma S ~ 0.6) has one whose dropped term is larger than its bound


def _case(run):
    rng = np.random.default_rng(zlib.crc32(run.id.encode()))
    idx, _ = J.make_lists(run, rng, O.three_nn)
    B, row, n_src = run.B, run.row, run.n_src
    w = None
    if run.kind == "interp":
        w = rng.uniform(0.1, 1.0, (B, row, 3))
        w = (w / w.sum(-1, keepdims=True)).astype(np.float32).reshape(B, 3 * row)
    g = rng.standard_normal((B, C, row)).astype(np.float32)
    init = rng.standard_normal((B, C, n_src)).astype(np.float32)
    return rng, idx, w, g, init


def _matters(run, idx, mutate):
    if mutate == "weight_j_swapped":                    # a triple on ONE source point sums the same three products in any rotation
        if run.kind != "interp":
            return False
        t = idx.reshape(run.B, -1, 3)
        return bool(((t[..., 0] != t[..., 1]) | (t[..., 1] != t[..., 2])).any())
    return True                                          # every case has a non-empty list, a non-zero init and C >= 2


@pytest.mark.parametrize("run", J.RUNS, ids=[r.id for r in J.RUNS])
def test_mirror_within_bound_exact_on_lattice_and_every_mutation_caught(run):
    rng, idx, w, g, init = _case(run)
    kind, n_src = run.kind, run.n_src
    assert idx.shape == (run.B, run.npos) and idx.min() >= 0 and idx.max() < n_src
    # floats: zero init and accumulation
    ref0, L, S0 = J.scatter64(kind, g, idx, w, n_src)
    assert int(L.sum()) == run.B * run.npos
    assert (np.abs(J.mirror32(kind, g, idx, w, n_src) - ref0) <= J.tolerance(L, S0)).all()
    ref, _, S = J.scatter64(kind, g, idx, w, n_src, init)
    tol = J.tolerance(L, S)
    assert (np.abs(J.mirror32(kind, g, idx, w, n_src, init) - ref) <= tol).all()
    # lattice: exact
    gl, wl, il = J.lattice(kind, (run.B, C, run.row, n_src), rng)
    refl, _, _ = J.scatter64(kind, gl, idx, wl, n_src, il)
    assert np.abs(refl).max() < 2.0 ** 22
    np.testing.assert_array_equal(J.mirror32(kind, gl, idx, wl, n_src, il).astype(np.float64), refl)
    # mutations
    for mutate in J.MUTATIONS:
        bad_l = J.mirror32(kind, gl, idx, wl, n_src, il, mutate=mutate).astype(np.float64)
        bad_f = J.mirror32(kind, g, idx, w, n_src, init, mutate=mutate)
        if _matters(run, idx, mutate):
            assert not np.array_equal(bad_l, refl), mutate
            assert (np.abs(bad_f - ref) > tol).any(), mutate
        else:
            np.testing.assert_array_equal(bad_l, refl)
            assert (np.abs(bad_f - ref) <= tol).all(), mutate


def test_scatter64_against_a_plain_loop():
    rng = np.random.default_rng(1)
    B, c, m, n = 2, 3, 4, 7
    idx = rng.integers(0, m, (B, 3 * n)).astype(np.int32)
    w = rng.random((B, 3 * n), dtype=np.float32)
    g = rng.standard_normal((B, c, n)).astype(np.float32)
    init = rng.standard_normal((B, c, m)).astype(np.float32)
    ref, L, S = J.scatter64("interp", g, idx, w, m, init)
    want, wantS, wantL = init.astype(np.float64), np.abs(init.astype(np.float64)), np.zeros((B, m), np.int64)
    for b in range(B):
        for p in range(3 * n):
            wantL[b, idx[b, p]] += 1
            for ch in range(c):
                t = float(w[b, p]) * float(g[b, ch, p // 3])
                want[b, ch, idx[b, p]] += t
                wantS[b, ch, idx[b, p]] += abs(t)
    np.testing.assert_allclose(ref, want, rtol=1e-14, atol=0)
    np.testing.assert_allclose(S, wantS, rtol=1e-14, atol=0)
    np.testing.assert_array_equal(L, wantL)
    refg, _, Sg = J.scatter64("gather", g, idx[:, :n], None, m)
    wantg = np.zeros((B, c, m))
    for b in range(B):
        for p in range(n):
            wantg[b, :, idx[b, p]] += g[b, :, p]
    np.testing.assert_allclose(refg, wantg, rtol=1e-14, atol=1e-300)


def test_bound_is_the_written_formula():
    for L, S in ((0, 3.0), (1, 1.0), (100, 7.5), (16384, 1e3)):
        k = (L + 2) * 2.0 ** -24
        assert J.bound(L, S) == k / (1 - k) * S
    assert J.bound(5, 0.0) == 0.0
    assert (J.tolerance(np.zeros((1, 2), np.int64), np.zeros((1, 3, 2))) == 2.0 ** -149).all()


def test_list_makers_and_table():
    rng = np.random.default_rng(3)
    assert sorted(J.permutation(rng, 50, 50)) == list(range(50))
    assert (J.all_first(rng, 9, 20) == 0).all() and (J.all_last(rng, 9, 20) == 8).all()
    s = J.sparse(rng, 100, 500)
    assert (s % 7 == 0).all() and s.max() < 100 and len(np.unique(s)) > 5
    for r in J.RUNS:
        if r.lists in ("all_first", "all_last", "permutation"):
            continue
        idx, _ = J.make_lists(r, np.random.default_rng(4), O.three_nn)
        if r.B > 1 and r.n_src > 7:                                   # (up to 7 source points `sparse` has only point 0 to name)
            assert not np.array_equal(idx[0], idx[1]), r.id           # every cloud a list of its own
    assert len({r.id for r in J.RUNS}) == len(J.RUNS)
    routes = {r.route for r in J.RUNS}
    assert routes == {"lds-cpb1", "lds-cpb>1", "nonlds-group", "nonlds-interp", "atomics-group", "atomics-interp"}
    by = {r.id: r for r in J.RUNS}
    assert by["group-lds-cpb2-odd-c-ball_like"].cpb == 2 and by["group-lds-cpb4-train-batch-ball_like"].cpb == 4
    assert by["group-lds-cpb16-tail6-ball_like"].cpb == 16 and by["interp-lds-cpb4-nn"].cpb == 4 and by["interp-lds-cpb2-nn"].cpb == 2
    assert by["group-lds-row-cap-ball_like"].route == "lds-cpb1" and by["group-nonlds-chan-tail-ball_like"].row == 16388
