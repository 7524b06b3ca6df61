"""A float64 judge for the AXIS-ONLY inlier test of the symmetric categories (captra_part_fit_guard_sym, captra_part_fit_ransac_sym;
tests/test_guard_sym_cpu.py, tests/test_guard_sym_gpu.py), on top of tests/guard_judge.py (verdict, the verdict codes) and
tests/ransac_judge.py (draw_ranks, umeyama, members_of, recipe_cloud).

  * `residual2(S, T, a, sc, tr, dt)`: the test of include/captra_hip.h.  The seven parameters are fp32 for both dt (the kernel's input
    by definition); dt = float64 evaluates from them in float64, dt = float32 is the MIRROR: the header's expression operation by
    operation in numpy float32.
  * `check(S, T, rot, scale, trans, th, dt)`: the guard's check of one part, a = the second column of rot.
  * `fit(S, T, triples, th, dt)`: ransac_judge.fit with the axis-only residual in the scores and in the winner's inlier set.
  * `judge` / `preconditions`: guard_judge's, with the new residual in the check AND in the re-fit; the draws from J.draw_ranks.
    The preconditions, asserted in float64, are guard_judge's (1)-(3) restated for the axis-only residual e = sqrt(e2):
      (1) no member's e under the tracked pose lies within [0.9 th, 1.1 th];
      (2) inliers * D - L * count != 0 for every part that has min_members;
      (3) for a lost part, with lo / hi = the largest number of members with e below 0.9 th / 1.1 th over the hypotheses, either
          lo == hi != the tracked inlier count and the top hypotheses select one inlier set with no e within 10 % of th, or hi < 3.
  * `judge_fit` / `fit_preconditions`: the same for the fit alone (captra_part_fit_ransac_sym), (3) for EVERY part of >= 3 members.
  * `check_case` / `refit_case`: guard_judge's fixtures made decidable under the wider acceptance band of this test (a ring of
    revolution has far more volume than a sphere):
      - every tracked pose, 'true' included, is composed with R_y(phi), phi uniform in [0.5, 2.5] rad, in float64 before rounding:
        for a symmetric object the same pose, for the full-rotation test another one;
      - 'lost' = the pose shifted by 3 th along the part's own y-axis: every true inlier is 3 th off in height, its radius unchanged
        (guard_judge's 30 degree tilt crosses the band by construction and is not used);
      - outliers are redrawn until their e under the true pose exceeds 3 th;
      - any member still within [0.9 th, 1.1 th] under the tracked pose is relabelled -1.
"""
import numpy as np

from tests import guard_judge as G
from tests import ransac_judge as J

OK, TOO_FEW, LOST, RECOVERED = G.OK, G.TOO_FEW, G.LOST, G.RECOVERED


def rot_y(phi):
    c, s = np.cos(phi), np.sin(phi)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def params(rot, scale, trans):
    """(a (3,), sc, tr (3,)) fp32: the seven parameters as the kernel forms them from a pose."""
    return np.asarray(rot, np.float32)[:, 1].copy(), np.float32(scale), np.asarray(trans, np.float32).reshape(3)


def residual2(S, T, a, sc, tr, dt=np.float64):
    """S, T (K,3) fp32 members; a (...,3), sc (...), tr (...,3) -> e2 (..., K)."""
    f = dt
    a, sc, tr = np.asarray(a).astype(f)[..., None, :], np.asarray(sc).astype(f)[..., None], np.asarray(tr).astype(f)[..., None, :]
    S_, T_ = S.astype(f), T.astype(f)
    with np.errstate(all="ignore"):
        d = [T_[:, k] - tr[..., k] for k in range(3)]
        h = (a[..., 0] * d[0] + a[..., 1] * d[1]) + a[..., 2] * d[2]
        w = [d[k] - h * a[..., k] for k in range(3)]
        rt = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
        hs = sc * S_[:, 1]
        rs = sc * np.sqrt(S_[:, 0] * S_[:, 0] + S_[:, 2] * S_[:, 2])
        eh, er = h - hs, rt - rs
        e2 = eh * eh + er * er
    assert e2.dtype == f
    return e2


def check(S, T, rot, scale, trans, th, dt=np.float64):
    """-> dict(e2 (K,), inl (K,) bool, inliers, rms) under the tracked pose."""
    a, sc, tr = params(rot, scale, trans)
    with np.errstate(all="ignore"):
        e2 = residual2(S, T, a, sc, tr, dt)
        th_ = dt(np.float32(th))                # (the kernel's th is fp32; th * th in dt)
        inl = e2 < th_ * th_
        k = int(inl.sum())
        rms = np.sqrt(e2[inl].sum(dtype=dt) / dt(k)) if k else dt(0)
    return dict(e2=e2, inl=inl, inliers=k, rms=rms)


def fit(S, T, triples, th, dt=np.float64):
    """ransac_judge.fit with the axis-only residual: dict(score (H,), best, inliers (K,) bool, err (H,K), pose or None)."""
    with np.errstate(all="ignore"):
        R, s, t = J.umeyama(S[triples], T[triples], dt)
        err = np.sqrt(residual2(S, T, R[..., :, 1], s, t, dt))
        inl_all = err < dt(th)
        score = inl_all.sum(-1)
        best = int(np.argmax(score))
        inl = inl_all[best]
        pose = J.umeyama(S[inl], T[inl], dt) if inl.sum() >= 3 else None
    return dict(score=score, best=best, inliers=inl, err=err, pose=pose)


def _finite32(pose):
    R, s, t = pose
    return bool(np.isfinite(R.astype(np.float32)).all() and np.isfinite(np.float32(s)) and np.isfinite(t.astype(np.float32)).all())


def judge(case, L, D, min_members=4, refit=False, num_hyps=64, seed=0, b0=0, dt=np.float64):
    """guard_judge.judge with the axis-only residual in the check and in the re-fit's scoring."""
    B, P = case["scale"].shape
    th = float(case["th"])
    out = dict(count=np.zeros((B, P), np.int64), inliers=np.zeros((B, P), np.int64), verdict=np.zeros((B, P), np.int64),
               rms=np.zeros((B, P), dt), rot=case["rot"].astype(np.float64), scale=case["scale"].astype(np.float64),
               trans=case["trans"].astype(np.float64), refit={})
    for b in range(B):
        for p in range(P):
            pts, S, T = J.members_of(case, b, p)
            c = check(S, T, case["rot"][b, p], case["scale"][b, p], case["trans"][b, p], th, dt)
            v = G.verdict(len(pts), c["inliers"], L, D, min_members)
            if refit and v == LOST and len(pts) >= 3:
                j = fit(S, T, J.draw_ranks(seed, b0 + b, p, num_hyps, len(pts)), th, dt)
                out["refit"][b, p] = j
                if j["pose"] is not None and int(j["score"].max()) > c["inliers"] and _finite32(j["pose"]):
                    v = RECOVERED
                    out["rot"][b, p], out["scale"][b, p], out["trans"][b, p] = j["pose"]
            out["count"][b, p], out["inliers"][b, p], out["verdict"][b, p], out["rms"][b, p] = len(pts), c["inliers"], v, c["rms"]
    return out


def _decidable_fit(j, th, tag, tracked=None):
    """(3) for one fit; -> False when no hypothesis can have three inliers whatever the rounding."""
    err = j["err"]
    lo, hi = (err < 0.9 * th).sum(-1), (err < 1.1 * th).sum(-1)
    if hi.max() < 3:
        return False
    assert lo.max() == hi.max() and lo.max() != tracked, ("(3)",) + tag + (int(lo.max()), int(hi.max()), tracked)
    top = np.nonzero(hi == hi.max())[0]
    assert (lo[top] == hi[top]).all(), ("(3) a residual within 10 % of th",) + tag
    sets = err[top] < th
    assert (sets == sets[0]).all(), ("(3) two top hypotheses with different inlier sets",) + tag
    return True


def preconditions(case, L, D, min_members=4, refit=False, num_hyps=64, seed=0, b0=0):
    """(1)-(3) of the module docstring for every part, in float64; raises on a broken fixture.  -> the judge's result."""
    B, P = case["scale"].shape
    th = float(case["th"])
    ref = judge(case, L, D, min_members, refit, num_hyps, seed, b0)
    for b in range(B):
        for p in range(P):
            pts, S, T = J.members_of(case, b, p)
            with np.errstate(all="ignore"):
                e = np.sqrt(check(S, T, case["rot"][b, p], case["scale"][b, p], case["trans"][b, p], th)["e2"])
            assert not ((e >= 0.9 * th) & (e <= 1.1 * th)).any(), ("(1)", b, p)
            if len(pts) >= min_members:
                assert ref["inliers"][b, p] * D - L * len(pts) != 0, ("(2)", b, p)
            if (b, p) in ref["refit"]:
                if not _decidable_fit(ref["refit"][b, p], th, (b, p), int(ref["inliers"][b, p])):
                    assert ref["verdict"][b, p] == LOST, ("(3)", b, p)
    return ref


def judge_fit(case, num_hyps=64, seed=0, b0=0, dt=np.float64):
    """captra_part_fit_ransac_sym drawing in the kernel (key b0 + b): ransac_judge.judge_batch's outputs plus fits {(b,p): fit}."""
    B, P = case["src"].shape[:2]            # (not the pose's: a batch padded in front has more trajectories than poses)
    th = float(case["th"])
    out = dict(rot=np.tile(np.eye(3), (B, P, 1, 1)), scale=np.ones((B, P)), trans=np.zeros((B, P, 3)), valid=np.zeros((B, P), bool),
               num_inliers=np.zeros((B, P), np.int64), best=np.zeros((B, P), np.int64), fits={})
    for b in range(B):
        for p in range(P):
            pts, S, T = J.members_of(case, b, p)
            if len(pts) < 3:
                continue
            j = out["fits"][b, p] = fit(S, T, J.draw_ranks(seed, b0 + b, p, num_hyps, len(pts)), th, dt)
            out["best"][b, p], out["num_inliers"][b, p] = j["best"], int(j["inliers"].sum())
            if j["pose"] is not None and _finite32(j["pose"]):
                out["rot"][b, p], out["scale"][b, p], out["trans"][b, p] = j["pose"]
                out["valid"][b, p] = True
    return out


def fit_preconditions(case, num_hyps=64, seed=0, b0=0):
    """(3) for every part of >= 3 members (no tracked count to differ from); a part whose hypotheses cannot reach three inliers is
    invalid whatever the rounding, but its best index is not pinned: -> (judge_fit result, {(b,p)} of the parts with a pinned best)."""
    ref = judge_fit(case, num_hyps, seed, b0)
    pinned = {bp for bp, j in ref["fits"].items() if _decidable_fit(j, float(case["th"]), bp)}
    return ref, pinned


# ---------------------------------------------------------------------------------------------------------------- fixtures
def _assemble(rng, labels, P, ext, with_mean, mode_of, nan_member):
    """guard_judge._assemble for the axis-only test (module docstring); modes 'true', 'lost', 'zero', 'gross'.  Adds true_in
    {(b,p): (K0,) bool over the part's members BEFORE the relabelling} and n_true (B,P): the true inliers that are still members."""
    labels = labels.copy()
    B, N = labels.shape
    th = 0.02 * ext
    src = (rng.random((B, P, 3, N)) - 0.5).astype(np.float32)
    pts = np.array([0.0, 0.0, 2.0])[None, :, None] + (rng.random((B, 3, N)) - 0.5)
    rot, scale, trans = np.tile(np.eye(3, dtype=np.float32), (B, P, 1, 1)), np.ones((B, P), np.float32), np.zeros((B, P, 3), np.float32)
    modes, true_pts = {}, {}
    for b in range(B):
        for p in range(P):
            idx = np.nonzero(labels[b] == p)[0]
            mode = modes[b, p] = mode_of(b, p)
            R, s, t = J.random_rotation(rng), ext, np.array([rng.uniform(-.5, .5), rng.uniform(-.5, .5), rng.uniform(1, 3)])
            true_pts[b, p] = idx[:0]
            if len(idx):
                S, T, _, tin, (R, s, t) = J.recipe_cloud(rng, len(idx), ext=ext)
                T = T.astype(np.float64)
                if mode == "gross":
                    T = t + (rng.random((len(idx), 3)) - 0.5) * 1000 * th
                    tin = np.zeros(len(idx), bool)
                else:
                    out = np.nonzero(~tin)[0]
                    while len(out):      # outliers clear of the surface of revolution by 3 th
                        e = np.sqrt(residual2(S[out], T[out].astype(np.float32), R[:, 1], np.float64(s), t))
                        out = out[e <= 3 * th]
                        T[out] = t + (rng.random((len(out), 3)) - 0.5) * 100 * th
                src[b, p][:, idx], pts[b][:, idx] = S.T, T.T
                true_pts[b, p] = idx[tin]
            if mode == "lost":
                t = t + 3 * th * R[:, 1]
            elif mode == "zero":
                s = 0.0
            R = R @ rot_y(rng.uniform(0.5, 2.5))            # the same pose of a symmetric object, another one for the full test
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
    case = dict(labels=labels, src=np.ascontiguousarray(src, np.float32), tgt=np.ascontiguousarray(pts, np.float32), tgt_mean=mean,
                th=np.float32(th), rot=rot, scale=scale, trans=trans, modes=modes)
    # members still within the band under the tracked pose (as the kernel reads them) leave their part
    n_true = np.zeros((B, P), np.int64)
    for b in range(B):
        for p in range(P):
            ptsi, S, T = J.members_of(case, b, p)
            with np.errstate(all="ignore"):
                e = np.sqrt(check(S, T, rot[b, p], scale[b, p], trans[b, p], float(case["th"]))["e2"])
            labels[b, ptsi[(e >= 0.9 * th) & (e <= 1.1 * th)]] = -1
            keep = true_pts[b, p][labels[b, true_pts[b, p]] == p]
            n_true[b, p] = np.isfinite(case["tgt"][b][:, keep]).all(0).sum()
    case["n_true"] = n_true
    return case


SMALL_COUNTS = G.SMALL_COUNTS


def check_case(B, P, N, with_mean, seed=0):
    """guard_judge.check_case: trajectory 0 random labels in [-2, P+1], phi-rotated true poses except the last part's (scale 0), one
    member of part 0 with a NaN target; trajectory 1 parts of 2, 3, 4 and 0 members; trajectory 2 every point in part 0, its pose
    lost (3 th along its y-axis)."""
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
        return "lost" if b >= 2 else "true"
    return _assemble(rng, labels, P, rng.uniform(0.05, 0.3), with_mean, mode_of, nan_member=True)


REFIT_MODES = ("true", "lost", "gross")


def refit_case(B, P, N, seed=0, first=0):
    """guard_judge.refit_case: part (b, p) takes REFIT_MODES[(first + b * P + p) % 3]: the phi-rotated true pose (ok), that pose 3 th
    along its y-axis (lost -> recovered), the true pose on a part of gross outliers only (lost, re-fit rejected).  `first` lets a
    shape of a single part meet all three."""
    rng = np.random.default_rng(seed + 104729 * (N + 17 * P + 5 * B) + 15485863 * first)
    labels = rng.integers(-1, P, (B, N)).astype(np.int32)
    return _assemble(rng, labels, P, rng.uniform(0.05, 0.3), True, lambda b, p: REFIT_MODES[(first + b * P + p) % 3], nan_member=False)
