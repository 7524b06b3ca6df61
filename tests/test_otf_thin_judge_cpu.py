"""The judge of the re-crop's on-device thinning (tests/otf_thin_judge.py) held to the rule's own properties (include/captra_hip.h:
captra_otf_thin): T distinct ascending members, a pure function of (seed, trajectory, frame, count) that every one of them changes,
the tie rule on given keys, uniform inclusion -- and each of four mutations of the rule is caught by at least one of these checks, so
a judge that had drifted into one of them would not pass."""
import numpy as np
import pytest

from tests import otf_thin_judge as TJ


def _row(count=250, num_points=40, seed=3, traj=5, frame=7, cap=3000, keys=None, judge=TJ):
    return judge.thin_row(count, cap, num_points, seed, traj, frame, keys)


def check_ascending_distinct(judge):
    for count, n in ((41, 8), (250, 40), (3000, 8), (1025, 8)):
        row = _row(count, n, judge=judge)
        assert row.dtype == np.int32 and len(row) == 5 * n
        assert (np.diff(row.astype(np.int64)) > 0).all() and row[0] >= 0 and row[-1] < count


def check_pure_function_of_every_argument(judge):
    base = _row(judge=judge)
    assert np.array_equal(base, _row(judge=judge))
    for change in ({"seed": 4}, {"traj": 6}, {"frame": 8}, {"count": 251}):
        assert not np.array_equal(base, _row(judge=judge, **change)), change
    # the launch form: row i of a launch at b0 is trajectory b0 + i
    counts = [250, 250, 250, 250, 250]
    whole, flags = judge.thin(counts, 3000, 40, 0, 7, 3)
    lane, _ = judge.thin(counts[2:], 3000, 40, 2, 7, 3)
    assert flags.tolist() == [1] * 5 and np.array_equal(whole[2:], lane) and not np.array_equal(whole[0], whole[1])
    assert np.array_equal(whole[4], judge.thin_row(250, 3000, 40, 3, 4, 7))


def check_given_keys(judge):
    T, c = 40, 100
    same = np.full(c, 77, np.uint32)
    assert _row(c, 8, keys=same, judge=judge).tolist() == list(range(T))
    desc = np.arange(c, 0, -1).astype(np.uint32)
    assert _row(c, 8, keys=desc, judge=judge).tolist() == list(range(c - T, c))
    for extreme in (0, 0xFFFFFFFF):
        assert _row(c, 8, keys=np.full(c, extreme, np.uint32), judge=judge).tolist() == list(range(T))
    # two equal keys straddling rank T - 1 / T: 39 members below them, members 20 and 70 carry the threshold key, the rest lie above
    keys = np.full(c, 5000, np.uint32) + np.arange(c, dtype=np.uint32)
    low = [j for j in range(c) if j not in (20, 70)][:T - 1]
    keys[low] = np.arange(T - 1, dtype=np.uint32)
    keys[[20, 70]] = 1000
    got = _row(c, 8, keys=keys, judge=judge).tolist()
    assert got == sorted(low + [20]), got


def check_uniform(judge):
    """c = 250, T = 200, 4000 (trajectory, frame) rows: every member's inclusion count within 5 sigma of Binomial(4000, 0.8)."""
    c, n, rows = 250, 40, 4000
    hits = np.zeros(c, np.int64)
    for r in range(rows):
        hits[_row(c, n, seed=11, traj=r % 50, frame=r // 50, judge=judge)] += 1
    p = 200 / 250
    dev = np.abs(hits - rows * p) / np.sqrt(rows * p * (1 - p))
    assert dev.max() < 5.0, dev.max()


CHECKS = [check_ascending_distinct, check_pure_function_of_every_argument, check_given_keys, check_uniform]


@pytest.mark.parametrize("check", CHECKS, ids=[c.__name__ for c in CHECKS])
def test_judge(check):
    check(TJ)


def test_not_thinned_rows_and_launch_form():
    assert TJ.thin_row(40, 3000, 8, 0, 0, 0) is None and TJ.thin_row(3001, 3000, 8, 0, 0, 0) is None and TJ.thin_row(0, 3000, 8, 0, 0, 0) is None
    assert TJ.thin_row(41, 3000, 8, 0, 0, 0) is not None and TJ.thin_row(3000, 3000, 8, 0, 0, 0) is not None
    prefill = np.full((4, 40), -9, np.int32)
    table, flags = TJ.thin([40, 41, 3001, 3000], 3000, 8, 0, 1, 2, table=prefill)
    assert flags.tolist() == [0, 1, 0, 1] and (table[[0, 2]] == -9).all() and (table[[1, 3]] >= 0).all()


def test_mix_is_splitmix64s_finaliser():
    """Against Python integers: the published constants, modulo 2^64 (first outputs of splitmix64 seeded with 0 are the published
    0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4)."""
    def py_mix(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % (1 << 64)
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % (1 << 64)
        return z ^ (z >> 31)
    g = 0x9E3779B97F4A7C15
    assert int(TJ.mix(np.uint64(g))) == py_mix(g) == 0xE220A8397B1DCDAF
    assert int(TJ.mix(np.uint64((2 * g) % (1 << 64)))) == 0x6E789E6AA1B965F4
    seed, traj, frame = 12345, 9, 77
    row = py_mix(py_mix((seed + g) % (1 << 64)) ^ ((traj << 32) | frame))
    want = [py_mix(row ^ j) >> 32 for j in range(20)]
    assert TJ.member_keys(seed, traj, frame, 20).tolist() == want


# ---- mutations of the rule: each is caught ------------------------------------------------------------------------------------
class _Mutant:
    """otf_thin_judge with one function replaced."""
    def __init__(self, **repl):
        self.__dict__.update({k: getattr(TJ, k) for k in ("mix", "row_key", "member_keys", "select", "is_thinned")})
        self.__dict__.update(repl)

    def thin_row(self, count, cap, num_points, seed, traj, frame, keys=None):
        if not self.is_thinned(count, cap, num_points):
            return None
        u = self.member_keys(seed, traj, frame, count) if keys is None else np.asarray(keys, np.uint32)[:int(count)]
        return self.select(u, 5 * int(num_points))

    def thin(self, counts, cap, num_points, b0, frame, seed):
        rows = [self.thin_row(int(c), cap, num_points, seed, self.traj_of(b0, i), frame) for i, c in enumerate(counts)]
        return np.stack(rows), np.ones(len(rows), np.int32)

    def traj_of(self, b0, i):
        return b0 + i


def _descending(u, keep):
    return TJ.select(u, keep)[::-1].copy()


def _tie_to_higher(u, keep):
    u = np.asarray(u, np.uint32)
    j = np.arange(len(u))
    return np.sort(np.lexsort((-j, u))[:int(keep)]).astype(np.int32)


def _no_frame(seed, traj, frame, count):
    return TJ.member_keys(seed, traj, 0, count)


class _NoB0(_Mutant):
    def traj_of(self, b0, i):
        return i


MUTANTS = {"descending": _Mutant(select=_descending), "tie_to_higher_index": _Mutant(select=_tie_to_higher),
           "frame_left_out": _Mutant(member_keys=_no_frame), "b_instead_of_b0_plus_b": _NoB0()}


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_mutation_is_caught(name):
    caught = []
    for check in (check_ascending_distinct, check_pure_function_of_every_argument, check_given_keys):
        try:
            check(MUTANTS[name])
        except AssertionError:
            caught.append(check.__name__)
    assert caught, name


def test_the_unmutated_rule_passes_through_the_mutant_harness():
    for check in (check_ascending_distinct, check_pure_function_of_every_argument, check_given_keys):
        check(_Mutant())
