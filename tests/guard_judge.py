"""A float64 judge for the track guard (captra_part_fit_guard; tests/test_guard_cpu.py, tests/test_guard_gpu.py), on top of the
RANSAC judge (tests/ransac_judge.py: draw_ranks, fit, residuals, members_of, recipe_cloud).

  * `check(S, T, rot, scale, trans, th, dt)`: the check of include/captra_hip.h for ONE part (members only).  The twelve parameters
    are fp32(scale * rot) and trans for both dt (they are the kernel's input by definition); dt = float64 evaluates the residuals
    in float64 from them, dt = float32 is the MIRROR: the kernel's expression, operation by operation, in numpy float32, the mean
    and the root in float32 too.
  * `verdict(count, inliers, L, D, min_members)`: integers only.
  * `judge(case, ...)`: check + verdict + (refit) the RANSAC judge's `fit` on the ranks `draw_ranks(seed, b0 + b, p, ...)` for
    every lost part, with the acceptance rule: valid and best score > tracked inliers.
  * `check_case` / `refit_case`: the fixtures, and `preconditions(case, ...)`, what makes them decidable (asserted in float64):
      (1) no member's residual under the tracked pose lies within [0.9 th, 1.1 th];
      (2) inliers * D - L * count != 0 for every part that has min_members;
      (3) for a lost part, the re-fit's decision cannot turn on a rounding either: with lo / hi = the largest number of members
          below 0.9 th / 1.1 th over the hypotheses, either lo == hi != the tracked inlier count and the top hypotheses select one
          inlier set, or hi < 3 (fewer than three inliers whatever the rounding: invalid, rejected).  The second form is what the
          part of gross outliers meets: the true pose has 0 inliers there and no hypothesis has any, so "differs" cannot hold,
          and the re-fit is rejected for being invalid, not for its score.
"""
import numpy as np

from tests import ransac_judge as J

OK, TOO_FEW, LOST, RECOVERED = 0, 1, 2, 3


def params(rot, scale, trans):
    """fp32(scale * rot) row-major and trans: the twelve parameters as the kernel forms them."""
    with np.errstate(all="ignore"):
        return (np.float32(scale) * np.asarray(rot, np.float32)).astype(np.float32), np.asarray(trans, np.float32).reshape(3)


def check(S, T, rot, scale, trans, th, dt=np.float64):
    """S, T (K,3) fp32 members -> dict(e2 (K,) squared residuals, inl (K,) bool, inliers, rms)."""
    sR, t = params(rot, scale, trans)
    with np.errstate(all="ignore"):
        if dt == np.float32:
            S32, T32 = S.astype(np.float32), T.astype(np.float32)
            e = []
            for a in range(3):
                pr = ((sR[a, 0] * S32[:, 0] + sR[a, 1] * S32[:, 1]) + sR[a, 2] * S32[:, 2]) + t[a]
                e.append(T32[:, a] - pr)
            e2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
            assert e2.dtype == np.float32
            inl = e2 < np.float32(th) * np.float32(th)
        else:
            d = T.astype(dt) - (S.astype(dt) @ sR.astype(dt).T + t.astype(dt))
            e2 = (d * d).sum(-1)
            inl = e2 < dt(th) * dt(th)
        k = int(inl.sum())
        rms = np.sqrt(e2[inl].sum(dtype=dt) / dt(k)) if k else dt(0)
    return dict(e2=e2, inl=inl, inliers=k, rms=rms)


def verdict(count, inliers, L, D, min_members):
    if count < min_members:
        return TOO_FEW
    return LOST if inliers * D < L * count else OK


def _pose_of(case, b, p):
    return case["rot"][b, p], case["scale"][b, p], case["trans"][b, p]


def judge(case, L, D, min_members=4, refit=False, num_hyps=64, seed=0, b0=0, dt=np.float64):
    """-> dict(count, inliers, verdict (B,P) int, rms (B,P), rot / scale / trans: the pose the kernel must return -- for a
    recovered part the re-fit (of `dt`), everywhere else the input bits --, refit {(b,p): ransac_judge.fit result})."""
    B, P = case["scale"].shape
    th = float(case["th"])
    out = dict(count=np.zeros((B, P), np.int64), inliers=np.zeros((B, P), np.int64), verdict=np.zeros((B, P), np.int64),
               rms=np.zeros((B, P), dt), rot=case["rot"].astype(np.float64), scale=case["scale"].astype(np.float64),
               trans=case["trans"].astype(np.float64), refit={})
    for b in range(B):
        for p in range(P):
            pts, S, T = J.members_of(case, b, p)
            c = check(S, T, *_pose_of(case, b, p), th, dt)
            v = verdict(len(pts), c["inliers"], L, D, min_members)
            if refit and v == LOST and len(pts) >= 3:
                j = J.fit(S, T, J.draw_ranks(seed, b0 + b, p, num_hyps, len(pts)), th, dt)
                out["refit"][b, p] = j
                if j["pose"] is not None and int(j["score"].max()) > c["inliers"]:
                    R, s, t = j["pose"]
                    if np.isfinite(R.astype(np.float32)).all() and np.isfinite(np.float32(s)) and np.isfinite(t.astype(np.float32)).all():
                        v = RECOVERED
                        out["rot"][b, p], out["scale"][b, p], out["trans"][b, p] = R, s, t
            out["count"][b, p], out["inliers"][b, p], out["verdict"][b, p], out["rms"][b, p] = len(pts), c["inliers"], v, c["rms"]
    return out


def preconditions(case, L, D, min_members=4, refit=False, num_hyps=64, seed=0, b0=0):
    """(1)-(3) of the module docstring for every part, in float64; raises on a broken fixture.  -> the judge's result."""
    B, P = case["scale"].shape
    th = float(case["th"])
    ref = judge(case, L, D, min_members, refit, num_hyps, seed, b0)
    for b in range(B):
        for p in range(P):
            pts, S, T = J.members_of(case, b, p)
            with np.errstate(all="ignore"):
                e = np.sqrt(check(S, T, *_pose_of(case, b, p), th)["e2"])
            assert not ((e >= 0.9 * th) & (e <= 1.1 * th)).any(), ("(1)", b, p)
            if len(pts) >= min_members:
                assert ref["inliers"][b, p] * D - L * len(pts) != 0, ("(2)", b, p)
            if (b, p) in ref["refit"]:
                err = ref["refit"][b, p]["err"]
                lo, hi = (err < 0.9 * th).sum(-1), (err < 1.1 * th).sum(-1)
                if hi.max() < 3:
                    assert ref["verdict"][b, p] == LOST, ("(3)", b, p)
                    continue
                k = int(ref["inliers"][b, p])
                assert lo.max() == hi.max() and lo.max() != k, ("(3)", b, p, int(lo.max()), int(hi.max()), k)
                top = np.nonzero(hi == hi.max())[0]
                assert (lo[top] == hi[top]).all(), ("(3) a residual within 10 % of th", b, p)
                sets = (err[top] < th)
                assert (sets == sets[0]).all(), ("(3) two top hypotheses with different inlier sets", b, p)
    return ref


# ---------------------------------------------------------------------------------------------------------------- fixtures
def _rot_about(axis, deg):
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    a = np.deg2rad(deg)
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def _assemble(rng, labels, P, ext, with_mean, mode_of, nan_member):
    """Recipe clouds (ransac_judge.recipe_cloud: 30 % outliers from 8 members on) for every part of `labels` (B,N), one scale
    (hence one th) for the batch, one target cloud per trajectory; the tracked pose per part by mode_of(b, p):
      'true' the generating pose; 'off' rotated by 30 degrees about a random axis and shifted by 3 th along it; 'shift' shifted by 3 th;
      'zero' the true pose with scale 0; 'gross' the true pose on targets uniform in a cube of side 1000 th (gross outliers only).
    NaN / Inf in half of the points that are not members (src: of the part; pts: of any part); nan_member: the first member of
    part (0, 0) has a NaN target."""
    B, N = labels.shape
    th = 0.02 * ext
    src = (rng.random((B, P, 3, N)) - 0.5).astype(np.float32)
    pts = np.array([0.0, 0.0, 2.0])[None, :, None] + (rng.random((B, 3, N)) - 0.5)
    rot, scale, trans = np.tile(np.eye(3, dtype=np.float32), (B, P, 1, 1)), np.ones((B, P), np.float32), np.zeros((B, P, 3), np.float32)
    modes = {}
    for b in range(B):
        for p in range(P):
            idx = np.nonzero(labels[b] == p)[0]
            mode = modes[b, p] = mode_of(b, p)
            R, s, t = J.random_rotation(rng), ext, np.array([rng.uniform(-.5, .5), rng.uniform(-.5, .5), rng.uniform(1, 3)])
            if len(idx):
                S, T, _, _, (R, s, t) = J.recipe_cloud(rng, len(idx), ext=ext)
                if mode == "gross":
                    T = t + (rng.random((len(idx), 3)) - 0.5) * 1000 * th
                src[b, p][:, idx], pts[b][:, idx] = S.T, T.T
            if mode == "off":
                # the shift ALONG the rotation's axis: (R_delta - I) x is orthogonal to it, so every inlier of the true pose is at
                # least 3 th off under this one -- no residual can come near th
                axis = rng.normal(size=3)
                axis /= np.linalg.norm(axis)
                R, t = _rot_about(axis, 30.0) @ R, t + 3 * th * axis
            elif mode == "shift":
                d = rng.normal(size=3)
                t = t + 3 * th * d / np.linalg.norm(d)
            elif mode == "zero":
                s = 0.0
            rot[b, p], scale[b, p], trans[b, p] = R, s, t
    mean = None
    if with_mean:
        mean = pts.mean(-1).astype(np.float32)
        pts = pts - mean[:, :, None]
    pts = pts.astype(np.float32)
    bad = np.array([np.nan, np.inf, -np.inf], np.float32)
    member = labels[:, None, :] == np.arange(P)[None, :, None]
    hit = ~member & (rng.random((B, P, N)) < 0.5)
    src = np.where(hit[:, :, None, :], bad[rng.integers(0, 3, src.shape)], src)
    hit_t = ~member.any(1) & (rng.random((B, N)) < 0.5)
    pts = np.where(hit_t[:, None, :], bad[rng.integers(0, 3, pts.shape)], pts)
    if nan_member and (labels[0] == 0).any():
        pts[0, :, np.nonzero(labels[0] == 0)[0][0]] = np.nan
    return dict(labels=labels, src=np.ascontiguousarray(src, np.float32), tgt=np.ascontiguousarray(pts, np.float32), tgt_mean=mean,
                th=np.float32(th), rot=rot, scale=scale, trans=trans, modes=modes)


SMALL_COUNTS = (2, 3, 4, 0)


def check_case(B, P, N, with_mean, seed=0):
    """The fixture of the check: trajectory 0 random labels in [-2, P+1] (negative, P and P+1 belong to no part), tracked poses
    true except the last part's, whose scale is 0, and one member of part 0 with a NaN target; trajectory 1 parts of 2, 3, 4 and 0
    members (as far as P and N allow), the rest no part, true poses; trajectory 2 every point in part 0, its pose shifted by 3 th
    (lost), the other parts empty.  With B = 1 only trajectory 0 exists."""
    rng = np.random.default_rng(seed + 7919 * (N + 17 * P + 5 * B + with_mean))
    labels = np.empty((B, N), np.int32)
    labels[0] = rng.integers(-2, P + 2, N)
    if B > 1:
        row = np.full(N, P, np.int32)
        row[1::2] = -1
        at = 0
        for p in range(P):
            c = min(SMALL_COUNTS[p % 4], N - at)
            row[at:at + c] = p
            at += c
        labels[1] = row[rng.permutation(N)]
    if B > 2:
        labels[2:] = 0

    def mode_of(b, p):
        if b == 0:
            return "zero" if p == P - 1 else "true"
        return "shift" if b >= 2 else "true"
    return _assemble(rng, labels, P, rng.uniform(0.05, 0.3), with_mean, mode_of, nan_member=True)


REFIT_MODES = ("true", "off", "gross")


def refit_case(B, P, N, seed=0):
    """The fixture of the re-fit: labels uniform over [-1, P), recipe clouds with 30 % outliers; part (b, p) takes the mode
    REFIT_MODES[(b * P + p) % 3]: the true pose (ok), a pose 30 degrees / 3 th off (lost -> recovered), the true pose on a part of
    gross outliers only (lost, re-fit rejected)."""
    rng = np.random.default_rng(seed + 104729 * (N + 17 * P + 5 * B))
    labels = rng.integers(-1, P, (B, N)).astype(np.int32)
    return _assemble(rng, labels, P, rng.uniform(0.05, 0.3), True, lambda b, p: REFIT_MODES[(b * P + p) % 3], nan_member=False)
