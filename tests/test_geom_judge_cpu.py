"""The geometry judge judged (tests/geom_judge.py), no GPU.

* the judge's references, run as themselves, equal the C oracle on EVERY row of RUNS -- indices, squared distances, the sampler's
  running minima -- the non-finite clouds included, where the C semantics decide (d < temp ? d : temp, d2 > best, d < best);
* every deviation applicable to a knife-edge cloud changes an output index of that cloud, and does so at every route-specific
  position (each lane / chunk edge, the 8192-point tile edge, the K-th hit, every rank boundary): a knife-edge cloud that does not
  bite is a broken test, and this is what keeps tests/test_z_geom_edges_gpu.py honest;
* the exact evaluators are what they claim (rounding against numpy's, the contract against numpy float32);
* the fp32 weight mirror lies within gamma_8 of the float64 evaluation on every finite triple;
* the scaled clouds reproduce the unscaled indices in the judge itself.
Every output element of every row is compared: no masks, no tolerances on indices or squared distances.
"""
from fractions import Fraction

import numpy as np
import pytest

from oracle import ops as O
from tests import geom_judge as J


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_floats(a, b):
    """Equal as values, NaN == NaN (the sign and payload of a NaN are not part of the geometry contract)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


# ---- the exact arithmetic ---------------------------------------------------------------------------------------------------------------
def test_rounding_to_the_fp32_grid_is_numpys():
    rng = np.random.default_rng(0)
    xs = np.concatenate([rng.standard_normal(2000) * 10.0 ** rng.integers(-44, 30, 2000),
                         # exact ties between two floats, normal and subnormal, and the smallest numbers
                         [1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, 2.0 ** -149 * 0.5, 2.0 ** -149 * 1.5, 2.0 ** -149 * 2.5, 2.0 ** -127, 0.0]])
    for x in xs:
        assert J._rn(Fraction(float(x))) == Fraction(float(np.float32(x))), x


def test_exact_contract_is_the_numpy_float32_expression_and_the_deviations_deviate():
    rng = np.random.default_rng(1)
    a, b = (rng.random((300, 3)) - 0.5).astype(np.float32), (rng.random((300, 3)) - 0.5).astype(np.float32)
    differ = {d: 0 for d in J.DISTANCE_DEVIATIONS}
    for p, q in zip(a, b):
        c = J.exact("contract", p, q)
        assert c == J.contract(p, q)
        assert J.exact("assoc_r", p, q) == (lambda d: d[0] * d[0] + (d[1] * d[1] + d[2] * d[2]))(p - q)
        for d in J.DISTANCE_DEVIATIONS:
            v = J.exact(d, p, q)
            assert abs(float(v) - float(c)) <= (4e-7 if d == "expanded" else 2.5e-7 * float(c)), (d, v, c)
            differ[d] += int(v != c)
    print("deviations differing from the contract on 300 random pairs:", differ)
    assert all(n > 10 for n in differ.values()), differ


def test_the_two_squares_of_the_knife_radius_differ():
    assert J.r2_float(J.KNIFE_R) != J.r2_double(J.KNIFE_R)
    assert J.r2_float(J.LATTICE_R) == np.float32(0.0625)


# ---- judge == oracle on every row -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", J.RUNS, ids=J.row_id)
def test_references_equal_the_oracle(row):
    e = J.expected(row)
    if row["op"] == "fps":
        temp = np.full(e["xyz"].shape[:2], J.FPS_START, np.float32) if e["temp_in"] is None else e["temp_in"].copy()
        idx = O.furthest_point_sample(e["xyz"], row["m"], temp=temp)
        np.testing.assert_array_equal(e["idx"], idx)
        assert _same_floats(e["temp"], temp)
        if e["temp_in"] is not None:
            # the CUDA kernel's min(d, temp) replaces a NaN temp, the oracle's ternary keeps it: the case tells the two apart
            assert not np.array_equal(e["idx"], e["idx_fminf"]) or not _same_floats(e["temp"], e["temp_fminf"])
            assert np.isnan(e["temp"]).sum() == 3 and not np.isnan(e["temp_fminf"]).any()
    elif row["op"] == "ball":
        for (r, k), got in zip(e["queries"], e["lists"]):
            np.testing.assert_array_equal(got, O.ball_query(r, k, e["xyz"], e["centres"]), err_msg=f"r={r} k={k}")
    else:
        k = row.get("k", 3)
        d2, idx = O.knn(k, e["unknown"], e["known"])
        np.testing.assert_array_equal(e["idx"], idx)
        assert _same_floats(e["d2"], d2)
        if k == 3:
            d2, idx = O.three_nn(e["unknown"], e["known"])
            np.testing.assert_array_equal(e["idx"], idx)
            assert _same_floats(e["d2"], d2)


# ---- every knife bites ------------------------------------------------------------------------------------------------------------------
def _ball_mutant(dev, c):
    kw = dict(r2=J.r2_float(J.KNIFE_R))
    if dev == "le":
        kw["cmp"] = J.le
    elif dev == "r2_double":
        kw["r2"] = J.r2_double(J.KNIFE_R)
    else:
        kw["d2"] = J.overridden(dev, c["pairs"])
    return kw


@pytest.mark.parametrize("n", [1500, 4096, 9000])
@pytest.mark.parametrize("dev", J.DEVIATIONS)
def test_ball_knife_cloud_bites_at_every_position(dev, n):
    c = J.ball_knife_cloud(dev, n)
    kw = _ball_mutant(dev, c)
    r2 = kw.pop("r2")
    centre = c["centres"][:1]
    ref = J.ball_query(J.r2_float(J.KNIFE_R), 64, c["xyz"], centre)[0]
    mut = J.ball_query(r2, 64, c["xyz"], centre, **kw)[0]
    flips = [(p in ref) != (p in mut) for p in c["positions"]]
    print(f"ball knife {dev} n={n}: positions {c['positions']} flipped {flips}; list {ref[:len(set(ref))].tolist()} -> {mut[:len(set(mut))].tolist()}")
    assert all(flips)
    if n > 8192:
        assert {8191, 8192} <= set(c["positions"])                  # across the scan's 8192-point LDS tile edge
    # once as the K-th hit: truncation and membership interact
    k = c["kth"]
    ref_k = J.ball_query(J.r2_float(J.KNIFE_R), k, c["xyz"], centre)[0]
    mut_k = J.ball_query(r2, k, c["xyz"], centre, **kw)[0]
    assert ref_k[k - 1] != mut_k[k - 1] and c["kth_pos"] in (ref_k[k - 1], mut_k[k - 1]), (ref_k, mut_k)
    # the neighbouring radii straddle every knife: all of them out below, all of them in above
    in_lo = J.ball_query(J.r2_float(J.KNIFE_R_LO), 64, c["xyz"], centre)[0]
    in_hi = J.ball_query(J.r2_float(J.KNIFE_R_HI), 64, c["xyz"], centre)[0]
    assert not set(c["positions"]) & set(in_lo) and set(c["positions"]) <= set(in_hi)


def test_exact_on_r2_lattice_points_bite_under_le():
    c = J.ball_knife_cloud("le", 4096)
    centre = c["centres"][1:2]
    on = (62, 65, 254, 257, 300, 301)
    assert (J.contract(c["xyz"][list(on)], centre[0]) == J.r2_float(J.LATTICE_R)).all()
    ref = J.ball_query(J.r2_float(J.LATTICE_R), 4096, c["xyz"], centre)[0]
    mut = J.ball_query(J.r2_float(J.LATTICE_R), 4096, c["xyz"], centre, cmp=J.le)[0]
    assert not set(on) & set(ref) and set(on) <= set(mut)


@pytest.mark.parametrize("n", J.FPS_SIZES)
def test_fps_knife_clouds_bite(n):
    kb = J.fps_knife_batch(n)
    m = 8
    lines = []
    for meta in kb["meta"]:
        ref, _ = J.fps(meta["xyz"], m)
        mut, _ = J.fps(meta["xyz"], m, d2=J.overridden(meta["dev"], meta["pairs"]))
        p = meta["pick"]
        want = meta["ib"] if meta["kind"] == "swap" else meta["ia"]     # swap: b is farther under the contract; eq: the lower index wins
        other = meta["ia"] if meta["kind"] == "swap" else meta["ib"]
        lines.append(f"{meta['dev']}/{meta['kind']}/pick{p}: {ref[p]} -> {mut[p]}")
        assert ref[p] == want and mut[p] == other, (meta["dev"], meta["kind"], p, ref, mut)
    print(f"fps knife n={n}: " + "; ".join(lines))


@pytest.mark.parametrize("n", J.FPS_SIZES)
def test_tie_clouds_bite_under_the_later_index_mutant(n):
    for b, xyz in enumerate(J.tie_clouds(n)):
        ref, _ = J.fps(xyz, 64)
        mut, _ = J.fps(xyz, 64, later_wins=True)
        assert not np.array_equal(ref, mut), (n, b)


@pytest.mark.parametrize("k", J.KNN_KS)
@pytest.mark.parametrize("dev", J.DISTANCE_DEVIATIONS)
def test_nn_knife_clouds_bite_at_every_rank_boundary(dev, k):
    c = J.expected(dict(op="knn", cloud=("knife", dev), k=k))["meta"][0]
    _, ref = J.knn(k, c["unknown"], c["known"])
    _, mut = J.knn(k, c["unknown"], c["known"], d2=J.overridden(dev, c["pairs"]))
    lines = []
    for t, j, kind, ia, ib in c["rows"]:
        first, second = (ia, ib)                                      # contract: a before b (nearer, or equal and earlier)
        assert ref[t, j - 1] == first and (j == k or ref[t, j] == second), (t, j, kind, ref[t])
        assert mut[t, j - 1] == second and (j == k or mut[t, j] == first), (t, j, kind, mut[t])
        lines.append(f"rank {j}/{kind}")
    print(f"knn knife {dev} k={k}: order changed at " + ", ".join(lines))
    assert {r[1] for r in c["rows"]} == {1, max(k - 1, 1), k}


@pytest.mark.parametrize("s", [v for v in J.WEIGHT_SIZES if v >= 37])
def test_weight_route_knife_clouds_bite(s):
    e = J.expected(dict(op="weights", cloud=("knife", s)))
    for dev, c in zip(J.DISTANCE_DEVIATIONS, e["meta"]):
        _, ref = J.three_nn(c["unknown"], c["known"])
        _, mut = J.three_nn(c["unknown"], c["known"], d2=J.overridden(dev, c["pairs"]))
        for t, j, kind, ia, ib in c["rows"]:
            assert ref[t, j - 1] == ia and mut[t, j - 1] == ib, (dev, t, j, kind)
        if s > 4096:
            assert c["rows"][0][3:] == (4095, 4096)                  # a pair across the 4096-point tile edge of the known cloud


def test_tie_clouds_bite_under_the_le_insertion_mutant():
    e = J.expected(dict(op="nn3", cloud=("ties",)))
    for u, kn in zip(e["unknown"], e["known"]):
        assert not np.array_equal(J.three_nn(u, kn)[1], J.three_nn(u, kn, cmp=J.le)[1])
        assert not np.array_equal(J.knn(16, u, kn)[1], J.knn(16, u, kn, cmp=J.le)[1])
    e = J.expected(dict(op="ball", cloud=("ties", 4096)))
    r, k = e["queries"][0]
    on = sum(int((J.contract(x, c) == J.r2_float(r)).sum()) for x, cs in zip(e["xyz"][:1], e["centres"][:1]) for c in cs)
    print(f"lattice cloud: {on} points exactly on r2 over 64 centres")
    assert on > 20 and r == J.LATTICE_TIE_R
    assert not np.array_equal(e["lists"][0], J.ball_query_batch(J.r2_float(r), k, e["xyz"], e["centres"], cmp=J.le))


# ---- weights ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", [r for r in J.RUNS if r["op"] == "weights"], ids=J.row_id)
def test_weight_mirror_is_within_gamma8_of_float64(row):
    """r_j = 1 / (sqrt(d2_j) + 1e-8), norm = (r0 + r1) + r2, w_j = r_j / norm: correctly rounded operations on positive values."""
    e = J.expected(row)
    fin = np.isfinite(e["w64"]).all(-1)
    assert (np.isfinite(e["w32"]).all(-1) == fin).all()
    err = np.abs(e["w32"][fin].astype(np.float64) - e["w64"][fin]) / e["w64"][fin].clip(1e-300)
    nz = e["w64"][fin] > 0
    worst = float(err[nz].max()) if nz.any() else 0.0
    print(f"{J.row_id(row)}: finite triples {int(fin.sum())} of {fin.size}, worst relative error {worst / J.U:.2f} u (bound 8 u)")
    assert worst <= J.GAMMA8
    assert (e["w32"][fin][~nz] == 0).all()                             # a missing neighbour (d2 = +inf) weighs exactly 0 in both


# ---- scale ------------------------------------------------------------------------------------------------------------------------------
def test_power_of_two_scales_reproduce_the_unscaled_indices():
    for n in (512, 4096, 8192):
        base = J.expected(dict(op="fps", cloud=("scaled", n, 0), m=16))
        for e in (-20, 10):
            np.testing.assert_array_equal(J.expected(dict(op="fps", cloud=("scaled", n, e), m=16))["idx"], base["idx"])
        # 2^40: every squared distance exceeds the 1e10 start value, so the minimum never moves and index order decides
        np.testing.assert_array_equal(J.expected(dict(op="fps", cloud=("scaled", n, 40), m=16))["idx"], np.tile(np.arange(16), (2, 1)))
        # 2^-60: the squares of the smaller differences are subnormal, the sums about 2^-122; 2^-64: every squared distance is subnormal
        sub = J.contract(J.scaled(base["xyz"], -64)[0], J.scaled(base["xyz"], -64)[0, 0])
        assert ((sub > 0) & (sub < 2.0 ** -126)).sum() == n - 1
    base = J.expected(dict(op="ball", cloud=("scaled", 4096, 0)))
    for e in (-20, 10, 40):
        for a, b in zip(J.expected(dict(op="ball", cloud=("scaled", 4096, e)))["lists"], base["lists"]):
            np.testing.assert_array_equal(a, b)
    base = J.expected(dict(op="nn3", cloud=("scaled", 0)))
    for e in (-20, 10, 40):
        np.testing.assert_array_equal(J.expected(dict(op="nn3", cloud=("scaled", e)))["idx"], base["idx"])
