"""tests/size_judge.py proved on the CPU: the state machine against a hand-computed transition table whose every comparison is exact
(max_ratio = 2, means that are powers of two), E with the scale given against closed forms on exact lattices, the mutations of the
judge each caught by some row, and the fixtures of tests/test_size_gpu.py (their preconditions are asserted where they are built)."""
import numpy as np
import pytest

from tests import size_judge as ZJ
from tests import st_ransac_judge as SJ

F = np.float32
UP8, DOWN2 = np.nextafter(F(8), F(np.inf)), np.nextafter(F(2), F(0))
OPTS = dict(min_frames=2, max_ratio=2.0, max_frames=4, reset_after=3)
# (name, (mean_in, n_in, miss_in, scale_free, valid_free), (mean_out, n_out, miss_out, accepted, held)) under OPTS
TABLE = [
    ("first frame", (0.0, 0, 0, 4.0, 1), (4.0, 1, 0, 1, 0)),
    ("first frame, stale mean ignored", (64.0, 0, 5, 4.0, 1), (4.0, 1, 0, 1, 0)),
    ("min_frames-th accepted frame", (4.0, 1, 0, 8.0, 1), (6.0, 2, 0, 1, 1)),
    ("not established: no gate", (4.0, 1, 0, 64.0, 1), (34.0, 2, 0, 1, 1)),
    ("at the ratio, above", (4.0, 2, 0, 8.0, 1), (4.0 + 4.0 / 3.0, 3, 0, 1, 1)),
    ("at the ratio, below", (4.0, 2, 1, 2.0, 1), (4.0 - 2.0 / 3.0, 3, 0, 1, 1)),
    ("one ulp outside, above", (4.0, 2, 0, UP8, 1), (4.0, 2, 1, 0, 1)),
    ("one ulp outside, below", (4.0, 2, 1, DOWN2, 1), (4.0, 2, 2, 0, 1)),
    ("invalid frame", (4.0, 2, 1, 4.0, 0), (4.0, 2, 1, 0, 1)),
    ("NaN frame", (4.0, 1, 1, np.nan, 1), (4.0, 1, 1, 0, 0)),
    ("negative frame", (4.0, 1, 1, -4.0, 1), (4.0, 1, 1, 0, 0)),
    ("restart at reset_after", (4.0, 2, 2, 32.0, 1), (32.0, 1, 0, 1, 0)),
    ("one before reset_after", (4.0, 2, 1, 32.0, 1), (4.0, 2, 2, 0, 1)),
    ("saturation at max_frames", (4.0, 4, 0, 8.0, 1), (5.0, 4, 0, 1, 1)),
    ("beyond max_frames", (4.0, 7, 0, 8.0, 1), (5.0, 4, 0, 1, 1)),
    ("NaN mean restarts", (np.nan, 3, 1, 4.0, 1), (4.0, 1, 0, 1, 0)),
    ("mean <= 0 restarts", (-2.0, 3, 0, 4.0, 1), (4.0, 1, 0, 1, 0)),
    ("NaN mean, invalid frame: +0 leaves", (np.nan, 3, 1, 4.0, 0), (0.0, 0, 1, 0, 0)),
]


def _row(row, **kw):
    return ZJ.decide(*row[1], **{**OPTS, **kw})


@pytest.mark.parametrize("row", TABLE, ids=[r[0] for r in TABLE])
def test_transition_table(row):
    d = _row(row)
    mean, n, miss, accepted, held = row[2]
    assert (d["n"], d["miss"], d["accepted"], d["held"]) == (n, miss, accepted, held), d
    assert d["mean"] == mean and np.isfinite(d["mean32"])
    assert d["mean32"] == F(mean)
    # pass-through, first frames and restarts are bits, an average is one rounding of the float64 value
    assert d["exact"] == (accepted == 0 or n == 1), d


def test_options_absent_and_rotation():
    assert ZJ.decide(4.0, 100, 0, 8.0, 1, min_frames=1, max_ratio=2.0)["n"] == 101                   # no cap
    d = ZJ.decide(4.0, 2, 50, 32.0, 1, min_frames=1, max_ratio=2.0)                                  # never restarts
    assert (d["n"], d["miss"], d["accepted"], d["mean"]) == (2, 51, 0, 4.0)
    assert ZJ.decide(4.0, 2, 0, 4.0, 1, min_frames=1, max_ratio=2.0, rot_finite=False)["held"] == 0
    assert ZJ.decide(0.0, 0, 0, 4.0, 1, min_frames=1, max_ratio=2.0)["held"] == 1                    # decided on n_out
    # max_ratio is read as fp32
    r = 1.1
    edge = F(4.0) * F(r)
    assert float(edge) == 4.0 * float(F(r))
    assert ZJ.decide(4.0, 1, 0, edge, 1, min_frames=1, max_ratio=r)["accepted"] == 1


@pytest.mark.parametrize("mutation", ZJ.MUTATIONS)
def test_every_mutation_is_caught(mutation):
    caught = []
    for row in TABLE:
        d = _row(row, mutate=mutation)
        mean, n, miss, accepted, held = row[2]
        if (d["mean"], d["n"], d["miss"], d["accepted"], d["held"]) != (mean, n, miss, accepted, held):
            caught.append(row[0])
    print(mutation, "caught by", caught)
    assert caught
    with pytest.raises(AssertionError):
        for row in TABLE:
            d = _row(row, mutate=mutation)
            assert (d["mean"], d["n"], d["miss"], d["accepted"], d["held"]) == row[2]


# ------------------------------------------------------------------------------------------------------------- E-given
LATTICE = np.array([[x, y, z] for x in (1, 3) for y in (2, 4) for z in (5, 7)], np.float64)           # centroid (2, 3, 6), eight points
ROT = np.array([[0.0, 0, 1], [1, 0, 0], [0, 1, 0]])                                                # a cyclic permutation: exact products
RY90 = np.array([[0.0, 0, 1], [0, 1, 0], [-1, 0, 0]])                                              # R_y(90 degrees)
T_TRUE, S_TRUE = np.array([-3.0, 5.0, 16.0]), 0.25


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("sym", [False, True])
def test_estimator_given_closed_form(sym, dt):
    """Every quantity is a small dyadic rational: the closed forms hold EXACTLY, in float64 and in the fp32 mirror."""
    T = S_TRUE * LATTICE @ ROT.T + T_TRUE
    # sym: the given rotation is the true one turned about its own y-axis; E finds the in-plane angle back from the moments
    R0 = ROT @ RY90 if sym else ROT
    Rp, t = ZJ.estimator_given(LATTICE, T, R0, S_TRUE, sym, dt)
    np.testing.assert_array_equal(Rp, ROT.astype(dt))
    np.testing.assert_array_equal(t, T_TRUE.astype(dt))
    # the free estimator agrees on the scale to rounding (its denominator carries + 1e-6)
    _, s_free, _ = SJ.estimator(LATTICE, T, R0, sym, dt)
    assert abs(s_free - S_TRUE) < 1e-5
    for s2 in (0.5, 0.125, 1.0):
        Rp, t = ZJ.estimator_given(LATTICE, T, R0, s2, sym, dt)
        np.testing.assert_array_equal(t, (T_TRUE + (S_TRUE - s2) * ROT @ LATTICE.mean(0)).astype(dt))
    if not sym:
        # without sym the given rotation is taken as it is, right or wrong
        Rp, t = ZJ.estimator_given(LATTICE, T, ROT @ RY90, S_TRUE, False, dt)
        np.testing.assert_array_equal(Rp, (ROT @ RY90).astype(dt))
        np.testing.assert_array_equal(t, (T.mean(0) - S_TRUE * (ROT @ RY90) @ LATTICE.mean(0)).astype(dt))


@pytest.mark.parametrize("sym", [False, True])
def test_fit_given_on_a_recipe_cloud(sym):
    """Robust mode with the true scale given: the inliers are the true ones and t is the recipe's to the noise; plain mode on the same
    members is dragged by the outliers."""
    case = SJ.batch_case(257, 2257 + 10 * sym, False, True, sym, B=1)
    pts, S, T = SJ.members_of(case, 0, 0)
    ext = float(case["th"]) / 0.02
    j = ZJ.fit_given(S, T, case["rot"][0, 0], case["ranks"][0, 0] % len(pts), float(case["th"]), sym, ext)
    assert (j["inliers"] == case["true_in"][0, 0]).all() and j["t"] is not None
    _, s_free, t_free = SJ.estimator(S[j["inliers"]], T[j["inliers"]], case["rot"][0, 0], sym)
    assert abs(s_free - ext) < 1e-3 * ext and np.abs(j["t"] - t_free).max() < float(case["th"])
    t_plain = ZJ.plain_given(S, T, case["rot"][0, 0], ext, sym)
    assert np.abs(t_plain - t_free).max() > float(case["th"])


# ---------------------------------------------------------------------------------------------------- the GPU test's fixtures
def test_gpu_fixtures_hold_their_preconditions():
    """Every case of tests/test_size_gpu.py is built here, on the CPU: st_ransac_judge's preconditions for the free fit and
    size_judge's for the held fit are asserted by the builders (a broken seed raises and is replaced in SEEDS)."""
    from tests import test_size_gpu as G
    for N in G.SIZES:
        for sym in (False, True):
            case, state = G.fixture(N, sym)
            assert set(state[3]) == {(b, p) for b in range(3) for p in range(3)}
            if N == 257:
                G.drawn_fixture(sym)
    for kw in G.EXTRA_SHAPES:
        G.fixture(257, False, **kw)
