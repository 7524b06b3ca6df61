"""A float64 judge for holding a track's size (captra_part_fit_st_size, include/captra_hip.h; tests/test_size_judge_cpu.py,
tests/test_size_gpu.py, tests/test_size_loop_gpu.py), on top of tests/st_ransac_judge.py (members, the estimator E, the two inlier
tests, the free robust fit).

  * `decide(...)`: the state machine of one (trajectory, part) and one frame, in float64 on the fp32 values as stored.  `mutate` names
    one deliberate mistake ('open_gate', 'k_off_by_one', 'hold_on_n_in'): tests/test_size_judge_cpu.py shows that its table catches each.
  * `estimator_given(S, T, R, s, sym, dt)`: E with the scale GIVEN -- st_ransac_judge.estimator with s in place of <R', C> / (...).
  * `fit_given(S, T, R, triples, th, sym, s, dt)`: one part in robust mode: E-given on every three-member hypothesis, the inlier count
    of each, the first best, E-given on its inliers; `plain_given`: E-given on all members.  dt = float32: the MIRROR.
  * `judge_batch`: decision and held fit over a (B,P) batch in the kernel's layouts, from the free fit AS THE KERNEL READ OR WROTE IT
    (the decision is a function of those fp32 bits).
  * `check_precondition` / `check_batch`: (a)-(c) of st_ransac_judge for the HELD fit of every held recipe part -- its inlier set is
    immune to a rounding of any residual by 10 % of th.  A case that fails them is a broken fixture.
  * `table_state(base)`: nine rows of the transition table laid over the nine (b, p) cells of st_ransac_judge.batch_case.
"""
import numpy as np

from tests import st_ransac_judge as SJ
from tests.st_ransac_judge import members_of

INT_MAX = 2 ** 31 - 1
MUTATIONS = ("open_gate", "k_off_by_one", "hold_on_n_in")


# ----------------------------------------------------------------------------------------------------------- state machine
def decide(mean_in, n_in, miss_in, scale_free, valid_free, min_frames, max_ratio, max_frames=None, reset_after=None, rot_finite=True,
           mutate=None):
    """One step of the size state.  mean_in, scale_free: fp32 values (read as stored); max_ratio: read as fp32.
    -> dict(mean: the float64 value of mean_out BEFORE its one rounding, mean32: np.float32 of it, exact: mean_out must be these bits
            (pass-through, first frame, restart), n, miss, accepted, held)."""
    mean32_in, sf32 = np.float32(mean_in), np.float32(scale_free)
    n_in, miss_in = int(n_in), int(miss_in)
    if not (n_in > 0 and np.isfinite(mean32_in) and mean32_in > 0):
        n_in, mean32_in = 0, np.float32(0.0)
    m, s, r = float(mean32_in), float(sf32), float(np.float32(max_ratio))
    finite = bool(valid_free) and bool(np.isfinite(sf32)) and sf32 > 0
    established = n_in >= min_frames
    if mutate == "open_gate":
        inside = s < r * m and s * r > m
    else:
        inside = s <= r * m and s * r >= m
    accept = finite and (not established or inside)
    mean, exact, n, miss = m, True, n_in, miss_in
    if accept:
        cap = INT_MAX - 1 if max_frames is None else max_frames - 1
        k = min(n_in, cap)
        div = k + 2 if mutate == "k_off_by_one" and k > 0 else k + 1
        mean, exact = (s, True) if k == 0 else (m + (s - m) / div, False)
        n, miss = k + 1, 0
    elif finite:
        miss = min(miss_in + 1, INT_MAX)
        if reset_after is not None and miss >= reset_after:
            mean, exact, n, miss, accept = s, True, 1, 0, True
    held = ((n_in if mutate == "hold_on_n_in" else n) >= min_frames) and bool(rot_finite)
    return dict(mean=mean, mean32=np.float32(mean), exact=exact, n=n, miss=miss, accepted=int(accept), held=int(held))


# --------------------------------------------------------------------------------------------------------------- E-given
def estimator_given(S, T, R, s, sym, dt=np.float64):
    """E with the scale given: S, T (..., K, 3), R (3,3), s scalar -> R' (...,3,3), t (...,3)."""
    S, T, R = np.asarray(S).astype(dt), np.asarray(T).astype(dt), np.asarray(R).astype(dt)
    s = dt(s)
    with np.errstate(all="ignore"):
        Rp, _, _ = SJ.estimator(S, T, R, sym, dt)           # (the in-plane angle does not depend on s)
        sb, tb = S.mean(-2), T.mean(-2)
        t = tb - s * np.einsum("...ij,...j->...i", Rp, sb)
    return Rp.astype(dt), t.astype(dt)


def fit_given(S, T, R, triples, th, sym, s, dt=np.float64):
    """Robust mode, one part: dict(score (H,), best, inliers (K,) bool, err (H,K), t of E-given on the inliers or None)."""
    with np.errstate(all="ignore"):
        Rp, t = estimator_given(S[triples], T[triples], R, s, sym, dt)
        sv = np.full(len(triples), dt(s), dt)
        err = SJ.errors(S, T, R, Rp, sv, t, sym, dt)
        inl_all = err < dt(th)
        score = inl_all.sum(-1)
        best = int(np.argmax(score))
        inl = inl_all[best]
        t2 = estimator_given(S[inl], T[inl], R, s, sym, dt)[1] if inl.sum() >= 3 else None
    return dict(score=score, best=best, inliers=inl, err=err, t=t2)


def plain_given(S, T, R, s, sym, dt=np.float64):
    """Plain mode: E-given on ALL members -> t."""
    return estimator_given(S, T, R, s, sym, dt)[1]


def check_precondition(S, T, R, triples, th, true_in, sym, s):
    """(a)-(c) of st_ransac_judge's docstring for the held fit, in float64; raises on a broken fixture."""
    j = fit_given(S, T, R, triples, th, sym, s)
    e = j["err"]
    best, ntrue = int(j["score"].max()), int(true_in.sum())
    assert best == ntrue and (j["inliers"] == true_in).all(), ("(a)", best, ntrue)
    lo = (e < 0.9 * th).sum(-1)
    assert (lo == best).any(), ("(b)", int(lo.max()), best)
    hiset = e < 1.1 * th
    for h in np.nonzero(hiset.sum(-1) >= best)[0]:
        assert (hiset[h] == true_in).all(), ("(c)", int(h))
    return j


# ----------------------------------------------------------------------------------------------------------------- batch
def judge_batch(case, free, state, opts, robust, ranks=None, dt=np.float64, given=None):
    """free = (scale (B,P) f32, trans (B,P,3) f32, valid (B,P)) as the kernel read (plain) or wrote (robust) it; state = (mean, n, miss);
    opts = dict(min_frames, max_ratio, max_frames, reset_after); given (B,P) f32: the scale the held fit is given (default the
    judge's own fp32 mean_out).
    -> dict: decision {(b,p): decide()}, scale, trans (float64 where held and valid, else the pass-through value), valid (B,P) bool,
       held_inliers (B,P), inliers {(b,p): (N,) bool over the POINTS} of held cells."""
    ranks = case["ranks"] if ranks is None else ranks
    B, P, _, N = case["src"].shape
    th = float(case["th"])
    fs, ft, fv = free
    out = dict(decision={}, scale=np.asarray(fs, np.float64).copy(), trans=np.asarray(ft, np.float64).copy(), valid=np.asarray(fv).astype(bool).copy(),
               held_inliers=np.zeros((B, P), np.int64), inliers={})
    for b in range(B):
        for p in range(P):
            rot = case["rot"][b, p]
            d = decide(state[0][b, p], state[1][b, p], state[2][b, p], fs[b, p], fv[b, p], rot_finite=np.isfinite(rot.astype(np.float64).sum()), **opts)
            out["decision"][b, p] = d
            if not d["held"]:
                continue
            s = np.float32(d["mean32"] if given is None else given[b, p])
            pts, S, T = members_of(case, b, p)
            mask = np.zeros(N, bool)
            out["inliers"][b, p] = mask
            out["scale"][b, p], out["valid"][b, p] = s, False              # (an invalid held fit keeps trans_free)
            t = None
            if robust:
                if len(pts) >= 3:
                    j = fit_given(S, T, rot, np.asarray(ranks[b, p]) % len(pts), th, case["sym"], s, dt)
                    mask[pts[j["inliers"]]] = True
                    out["held_inliers"][b, p] = int(j["inliers"].sum())
                    t = j["t"]
            else:
                out["held_inliers"][b, p] = len(pts)
                mask[pts] = True
                if len(pts) > 3:
                    t = plain_given(S, T, rot, s, case["sym"], dt)
            if t is not None and len(pts) > 3 and np.isfinite(t.astype(np.float32)).all():
                out["trans"][b, p], out["valid"][b, p] = t, True
    return out


def check_batch(case, free, state, opts, ranks=None):
    """The held fit's preconditions for every held recipe part of >= 3 members (robust mode); the part of gross outliers: no
    hypothesis has three points below 1.1 th."""
    ranks = case["ranks"] if ranks is None else ranks
    th = float(case["th"])
    B, P = case["ranks"].shape[:2]
    for b in range(B):
        for p in range(P):
            d = decide(state[0][b, p], state[1][b, p], state[2][b, p], free[0][b, p], free[2][b, p], **opts)
            pts, S, T = members_of(case, b, p)
            if not d["held"] or len(pts) < 3:
                continue
            tri = np.asarray(ranks[b, p]) % len(pts)
            if (b, p) == case["outlier_part"]:
                j = fit_given(S, T, case["rot"][b, p], tri, th, case["sym"], d["mean32"])
                lo, hi = (j["err"] < 0.9 * th).sum(-1), (j["err"] < 1.1 * th).sum(-1)
                assert (hi < 3).all() and (lo == hi).all(), ("outlier part", b, p)
            else:
                check_precondition(S, T, case["rot"][b, p], tri, th, case["true_in"][b, p], case["sym"], d["mean32"])


# ------------------------------------------------------------------------------------------------------------------ cases
TABLE_OPTS = dict(min_frames=2, max_ratio=2.0, max_frames=4, reset_after=3)


def table_state(base, B=3, P=3, robust=False):
    """Nine rows of the transition table over the (b, p) cells of st_ransac_judge.batch_case, for a free scale of `base` (fp32) under
    TABLE_OPTS -> (mean (B,P) f32, n, miss (B,P) i32, what: {(b,p): the row's name}).  The rows are named for PLAIN mode, where the
    free fit is an input: scale `base` everywhere, valid everywhere but in cell (2, 2).  In robust mode the free fit is the cell's own
    -- valid in the recipe parts (0,0), (0,1), (2,0) and the part of four members (1,2), scale near base there -- so the cells of
    parts that cannot be fitted replay 'invalid frame' on their row's state; cell (1,1) (three members: found, never valid) then
    gets a mean near base, so that every held part of >= 3 members is held at a scale under which its true inliers stay inside
    0.9 th (the held fit's precondition)."""
    base = np.float32(base)
    two = np.float32(2) * base
    rows = {(0, 0): (0.0, 0, 0, "first frame: accepted, not yet held"),
            (0, 1): (np.float32(base * np.float32(1.004)), 1, 0, "the min_frames-th accepted frame: held"),
            (0, 2): (two, 2, 1, "exactly at the ratio from below: accepted"),
            (1, 0): (np.nextafter(two, np.float32(np.inf)), 2, 0, "one ulp outside: rejected, miss + 1, still held"),
            (1, 1): ((np.float32(base * np.float32(0.998)), 2, 1, "(robust) three members: invalid frame, held at the state's mean") if robust else
                     (np.float32(base / np.float32(2)), 2, 1, "exactly at the ratio from above: accepted")),
            (1, 2): (np.float32(8) * base, 3, 2, "restart at reset_after"),
            (2, 0): (np.float32(base * np.float32(0.996)), 4, 0, "saturation at max_frames"),
            (2, 1): (np.float32(np.nan), 3, 1, "a NaN mean with n > 0: empty"),
            (2, 2): (base, 2, 1, "invalid frame: the state's bits, held")}
    if P > 3:       # the part of gross outliers is the LAST one: its row follows it, and part 2 (a recipe part then) is held near base
        rows[0, P - 1] = rows[0, 2]
        rows[0, 2] = (np.float32(base * np.float32(1.002)), 2, 0, "established: accepted, held")
    mean, n, miss = np.zeros((B, P), np.float32), np.zeros((B, P), np.int32), np.zeros((B, P), np.int32)
    for (b, p), (m, k, s, _) in rows.items():
        if b < B and p < P:
            mean[b, p], n[b, p], miss[b, p] = m, k, s
    return mean, n, miss, {k: v[3] for k, v in rows.items()}
