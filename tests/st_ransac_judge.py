"""A float64 judge for the robust scale / translation fit with the rotation given (captra_part_fit_st_ransac;
tests/test_st_ransac_cpu.py, tests/test_st_ransac_gpu.py), on top of tests/ransac_judge.py (draws, recipe clouds, members, the
full-rotation residual) and tests/sym_judge.py (the axis-only residual, R_y).

  * `estimator(S, T, R, sym, dt)`: E of include/captra_hip.h in numpy -- the algebra of captra_part_fit_st on a set of pairs.
  * `fit(S, T, R, triples, th, sym, dt)`: one part (members only): E on every three-member hypothesis, the inlier count of each by
    the full-rotation (sym = 0) or the axis-only (sym = 1) test, the first best one, E on its inliers.  dt = float64 is the judge
    (from the fp32 inputs as stored), dt = float32 the same code in float32: the MIRROR.
  * `judge_batch`: the judge / mirror over a (B,P) batch in the kernel's layouts, with its validity and previous-value rules.
  * `batch_case`: ransac_judge.batch_case with the recipe's true rotation kept as `rot` (fp32; for sym composed with R_y(phi), phi in
    [0.5, 2.5], before rounding: the same pose of a symmetric object) and random finite prev_scale / prev_trans.  For sym the
    outliers are redrawn until their axis-only residual under the true pose exceeds 3 th (sym_judge's rule: a ring of revolution has
    far more volume than a sphere).
  * `check_batch`: ransac_judge's preconditions (a)-(c) for THIS estimator, in float64, for every recipe part -- a RANSAC result is a
    function of an inlier SET, and (a)-(c) make that set immune to a rounding of any residual by 10 % of th:
      (a) the best score equals the number of true inliers, and the best hypothesis's inliers are the true ones;
      (b) some hypothesis has all of them below 0.9 th;
      (c) every hypothesis with at least that many points below 1.1 th has exactly the true inliers below 1.1 th;
    for the part of gross outliers: no hypothesis has three points below 1.1 th.  `pinned_best` adds what makes the INDEX of the
    best hypothesis immune too: the first hypothesis that can reach the top score within 1.1 th reaches it within 0.9 th.
    A case that fails them is a broken fixture: the builder raises.
"""
import numpy as np

from tests.ransac_judge import draw_ranks, draw_triples, members_of, recipe_cloud, residuals  # noqa: F401  (draw_ranks: for the tests)
from tests.sym_judge import residual2, rot_y


# ------------------------------------------------------------------------------------------------------------- algorithm
def estimator(S, T, R, sym, dt=np.float64):
    """E: S, T (..., K, 3) pairs, R (3,3) the given rotation -> R' (...,3,3), s (...), t (...,3)."""
    S, T, R = np.asarray(S).astype(dt), np.asarray(T).astype(dt), np.asarray(R).astype(dt)
    with np.errstate(all="ignore"):
        sb, tb = S.mean(-2), T.mean(-2)
        sc, tc = S - sb[..., None, :], T - tb[..., None, :]
        C = np.swapaxes(tc, -1, -2) @ sc                    # C[a][c] = sum tc_a sc_c
        Css = np.swapaxes(sc, -1, -2) @ sc
        Rp = np.broadcast_to(R, C.shape).copy()
        if sym:
            M = (R.T @ C)[..., [0, 2], :][..., :, [0, 2]]   # the (x,z) block of R^T C
            a, c = M[..., 0, 0] + M[..., 1, 1], M[..., 1, 0] - M[..., 0, 1]
            h = np.sqrt(a * a + c * c)
            safe = np.where(h > 0, h, dt(1))
            cs = np.where(h > 0, a / safe, np.where(np.isnan(h), dt(np.nan), dt(1)))
            sn = np.where(h > 0, c / safe, np.where(np.isnan(h), dt(np.nan), dt(0)))
            R3 = np.zeros(C.shape, dt)
            R3[..., 0, 0], R3[..., 0, 2], R3[..., 1, 1], R3[..., 2, 0], R3[..., 2, 2] = cs, -sn, 1, sn, cs
            Rp = R @ R3
        num = (Rp * C).sum((-1, -2))
        den = ((np.swapaxes(Rp, -1, -2) @ Rp) * Css).sum((-1, -2)) + dt(1e-6)
        s = num / den
        t = tb - s[..., None] * np.einsum("...ij,...j->...i", Rp, sb)
    return Rp.astype(dt), s.astype(dt), t.astype(dt)


def errors(S, T, rot, Rp, s, t, sym, dt=np.float64):
    """The residual of every member under every hypothesis -> (H, K): the full-rotation one, or for sym the axis-only one about
    a = the second column of the GIVEN rotation as stored (R' has R's second column)."""
    if not sym:
        return residuals(S, T, Rp, s, t, dt)
    a = np.broadcast_to(np.asarray(rot, np.float32)[:, 1], (len(s), 3))
    with np.errstate(all="ignore"):
        return np.sqrt(residual2(S, T, a, s, t, dt))


def fit(S, T, R, triples, th, sym, dt=np.float64):
    """One part: S, T (K,3) fp32 members, R (3,3) fp32, triples (H,3) member ranks -> dict(score (H,), best, inliers (K,) bool,
    err (H,K), pose (s, t) of E on the inliers or None when fewer than three)."""
    with np.errstate(all="ignore"):
        Rp, s, t = estimator(S[triples], T[triples], R, sym, dt)
        err = errors(S, T, R, Rp, s, t, sym, dt)
        inl_all = err < dt(th)                       # a NaN error compares false: outside
        score = inl_all.sum(-1)
        best = int(np.argmax(score))
        inl = inl_all[best]
        pose = None
        if inl.sum() >= 3:
            _, s2, t2 = estimator(S[inl], T[inl], R, sym, dt)
            pose = (s2, t2)
    return dict(score=score, best=best, inliers=inl, err=err, pose=pose)


def plain(S, T, R, sym, dt=np.float64):
    """The plain estimator (captra_part_fit_st): E on ALL members -> (s, t)."""
    _, s, t = estimator(S, T, R, sym, dt)
    return s, t


# ----------------------------------------------------------------------------------------------------------------- batch
def judge_batch(case, ranks=None, dt=np.float64, prev=True):
    """The judge / mirror on a batch_case in the kernel's layouts; ranks (B,P,H,3) (default the case's; rank r = the (r mod count)-th
    member); prev=False: prev_* = NULL (an invalid fit writes 1 / 0).
    -> dict: scale (B,P), trans (B,P,3), valid (B,P) bool, num_inliers, best (B,P), inliers {(b,p): (N,) bool over the POINTS}."""
    ranks = case["ranks"] if ranks is None else ranks
    B, P, _, N = case["src"].shape
    th = float(case["th"])
    out = dict(scale=case["prev_scale"].astype(np.float64) if prev else np.ones((B, P)),
               trans=case["prev_trans"].astype(np.float64) if prev else np.zeros((B, P, 3)), valid=np.zeros((B, P), bool),
               num_inliers=np.zeros((B, P), np.int64), best=np.zeros((B, P), np.int64), inliers={})
    for b in range(B):
        for p in range(P):
            pts, S, T = members_of(case, b, p)
            mask = np.zeros(N, bool)
            out["inliers"][b, p] = mask
            if len(pts) < 3:
                continue
            j = fit(S, T, case["rot"][b, p], np.asarray(ranks[b, p]) % len(pts), th, case["sym"], dt)
            mask[pts[j["inliers"]]] = True
            out["best"][b, p], out["num_inliers"][b, p] = j["best"], int(j["inliers"].sum())
            if j["pose"] is None or len(pts) <= 3:           # count > 3: captra_part_fit_st's rule
                continue
            s, t = j["pose"]
            with np.errstate(all="ignore"):
                ok = np.isfinite(np.float32(s)) and np.isfinite(t.astype(np.float32)).all() and np.isfinite(case["rot"][b, p].astype(np.float64).sum())
            if ok:
                out["scale"][b, p], out["trans"][b, p], out["valid"][b, p] = s, t, True
    return out


def inlier_set(case, b, p, point_triple, dt=np.float64):
    """The inlier set (over the N points) of the hypothesis through the three POINT indices `point_triple` of part (b, p)."""
    pts, S, T = members_of(case, b, p)
    where = {int(i): k for k, i in enumerate(pts)}
    tri = np.array([[where[int(i)] for i in point_triple]])
    R = case["rot"][b, p]
    Rp, s, t = estimator(S[tri], T[tri], R, case["sym"], dt)
    err = errors(S, T, R, Rp, s, t, case["sym"], dt)[0]
    mask = np.zeros(case["labels"].shape[1], bool)
    mask[pts[err < dt(float(case["th"]))]] = True
    return mask


# ---------------------------------------------------------------------------------------------------------- preconditions
def check_precondition(S, T, R, triples, th, true_in, sym):
    """(a)-(c) of the module docstring, in float64; raises on a broken fixture.  Returns the judge's result."""
    j = fit(S, T, R, triples, th, sym)
    e = j["err"]
    best, ntrue = int(j["score"].max()), int(true_in.sum())
    assert best == ntrue and (j["inliers"] == true_in).all(), ("(a)", best, ntrue)
    lo = (e < 0.9 * th).sum(-1)
    assert (lo == best).any(), ("(b)", int(lo.max()), best)
    hiset = e < 1.1 * th
    for h in np.nonzero(hiset.sum(-1) >= best)[0]:
        assert (hiset[h] == true_in).all(), ("(c)", int(h))
    return j


def pinned_best(j, th):
    """The index of the best hypothesis is immune to a 10 % rounding: the first one that can reach the top within 1.1 th has it
    within 0.9 th."""
    e, top = j["err"], int(j["score"].max())
    first = int(np.nonzero((e < 1.1 * th).sum(-1) >= top)[0][0])
    return first == j["best"] and int((e[first] < 0.9 * th).sum()) == top


def check_batch(case, ranks=None, pin=False):
    """The preconditions of every part of >= 3 members of `case` under the member ranks `ranks`; pin: and `pinned_best`."""
    ranks = case["ranks"] if ranks is None else ranks
    th = float(case["th"])
    B, P = case["ranks"].shape[:2]
    for b in range(B):
        for p in range(P):
            pts, S, T = members_of(case, b, p)
            if len(pts) < 3:
                continue
            tri = np.asarray(ranks[b, p]) % len(pts)
            if (b, p) == case["outlier_part"]:
                j = fit(S, T, case["rot"][b, p], tri, th, case["sym"])
                assert ((j["err"] < 1.1 * th).sum(-1) < 3).all(), ("outlier part", b, p)
                lo, hi = (j["err"] < 0.9 * th).sum(-1), (j["err"] < 1.1 * th).sum(-1)
                assert (lo == hi).all(), ("outlier part: a residual within 10 % of th", b, p)
                assert not pin or lo.max() == 0 or pinned_best(j, th), ("outlier part: best not pinned", b, p)
            else:
                j = check_precondition(S, T, case["rot"][b, p], tri, th, case["true_in"][b, p], case["sym"])
                assert not pin or pinned_best(j, th), ("best not pinned", b, p)


# ----------------------------------------------------------------------------------------------------------------- cases
def batch_case(N, seed, per_part, with_mean, sym, num_hyps=64, B=3, P=3):
    """A (B,P) batch in the kernel's layouts whose every part of >= 3 members is a recipe cloud (one scale, hence one th, for the
    batch), labels arranged as ransac_judge.batch_case arranges them:
      trajectory 0: random labels in [-2, P+1] (negative, P and P+1 belong to no part); its LAST part holds gross outliers only
                    (targets uniform in a cube of side 1000 th);
      trajectory 1: parts of 2, 3 and 4 members, the rest no part (B, P >= 3);
      trajectory 2: every point in part 0, the other parts empty.
    With B = 1 only trajectory 0 exists and keeps recipe clouds in every part.  NaN / Inf sit in half of the points that are not
    members (src: of the part; tgt: of the part / of any part).  rot (B,P,3,3) fp32 = the recipe's true rotation (sym: times
    R_y(phi)); prev_scale (B,P), prev_trans (B,P,3) random and finite; ranks (B,P,H,3): triples without replacement.  The
    preconditions are asserted for every part, on the inputs as the kernel reads them (`check_batch`)."""
    rng = np.random.default_rng(seed)
    labels = np.empty((B, N), np.int32)
    labels[0] = rng.integers(-2, P + 2, N) if B > 1 else rng.choice(np.array([-1, 0, 0, 0, 1], np.int32), N)
    if B > 1:
        row = np.full(N, P, np.int32)
        row[:2], row[2:5], row[5:9] = 0, 1, 2
        row[9::2] = -1
        labels[1] = row[rng.permutation(N)]
        labels[2:] = 0
    ext = rng.uniform(0.05, 0.3)
    th = 0.02 * ext
    src = (rng.random((B, P, 3, N)) - 0.5).astype(np.float32)
    full = np.empty((B, P, 3, N))
    full[:] = np.array([0.0, 0.0, 2.0])[:, None] + (rng.random((B, P, 3, N)) - 0.5)
    rot = np.tile(np.eye(3), (B, P, 1, 1))
    true_in = {}
    outlier_part = (0, P - 1) if B > 1 else None
    for b in range(B):
        for p in range(P):
            pts = np.nonzero(labels[b] == p)[0]
            if len(pts) == 0:
                continue
            S, T, _, tin, (R, _, t) = recipe_cloud(rng, len(pts), ext=ext)
            T = T.astype(np.float64)
            if (b, p) == outlier_part:
                T = t + (rng.random((len(pts), 3)) - 0.5) * 1000 * th
                tin = np.zeros(len(pts), bool)
            elif sym:
                out = np.nonzero(~tin)[0]
                while len(out):      # outliers clear of the surface of revolution by 3 th
                    e = np.sqrt(residual2(S[out], T[out].astype(np.float32), R[:, 1], np.float64(ext), t))
                    out = out[e <= 3 * th]
                    T[out] = t + (rng.random((len(out), 3)) - 0.5) * 100 * th
            rot[b, p] = R @ rot_y(rng.uniform(0.5, 2.5)) if sym else R
            src[b, p][:, pts], full[b, p][:, pts], true_in[b, p] = S.T, T.T, tin
    if per_part:
        tgt = full
    else:           # one target cloud per trajectory: each point follows the part it is labelled with
        sel = np.where((labels >= 0) & (labels < P), labels, 0)
        tgt = np.take_along_axis(full, sel[:, None, None, :], axis=1)[:, 0]
    mean = None
    if with_mean:
        mean = tgt.reshape(B, -1, 3, N).mean((1, 3)).astype(np.float32) if per_part else tgt.mean(-1).astype(np.float32)
        tgt = tgt - (mean[:, None, :, None] if per_part else mean[:, :, None])
    tgt = tgt.astype(np.float32)
    bad = np.array([np.nan, np.inf, -np.inf], np.float32)
    member = labels[:, None, :] == np.arange(P)[None, :, None]
    hit = ~member & (rng.random((B, P, N)) < 0.5)
    src = np.where(hit[:, :, None, :], bad[rng.integers(0, 3, src.shape)], src)
    if per_part:
        hit_t = ~member & (rng.random((B, P, N)) < 0.5)
        tgt = np.where(hit_t[:, :, None, :], bad[rng.integers(0, 3, tgt.shape)], tgt)
    else:
        hit_t = ~member.any(1) & (rng.random((B, N)) < 0.5)
        tgt = np.where(hit_t[:, None, :], bad[rng.integers(0, 3, tgt.shape)], tgt)
    ranks = np.zeros((B, P, num_hyps, 3), np.int32)
    for b in range(B):
        for p in range(P):
            c = int((labels[b] == p).sum())
            if c >= 3:
                ranks[b, p] = draw_triples(rng, c, num_hyps)
    case = dict(labels=labels, src=np.ascontiguousarray(src, np.float32), tgt=np.ascontiguousarray(tgt, np.float32), tgt_mean=mean,
                th=np.float32(th), ranks=ranks, true_in=true_in, outlier_part=outlier_part, per_part=per_part, sym=bool(sym),
                rot=np.ascontiguousarray(rot, np.float32), prev_scale=rng.uniform(0.5, 2.0, (B, P)).astype(np.float32),
                prev_trans=rng.uniform(-1.0, 1.0, (B, P, 3)).astype(np.float32))
    check_batch(case)
    return case
