"""A float64 judge for the RANSAC similarity fit (captra_part_fit_ransac; tests/test_pose_ransac_gpu.py, tests/test_pose_ransac_cpu.py).

  * `fit(src, tgt, triples, th, dt)`: the semantics of include/captra_hip.h restated with numpy for ONE part (members only) --
    Umeyama on every three-point hypothesis, the inlier count of each, the first best one, the refit on its inliers.  dt =
    float64 is the judge (computed from the fp32 inputs as stored), dt = float32 the same algorithm in float32, the MIRROR.
  * `draw_ranks`: the numpy restatement of the kernel's counter-based draw generator, bit for bit.
  * `recipe_case` / `check_precondition`: the test inputs, and what makes them decidable: a RANSAC result is a function of an
    inlier SET, and a set can flip with the rounding of one residual.  Every case handed out satisfies, in float64,
      (a) the best score equals the number of true inliers;
      (b) some hypothesis has all of them below 0.9 th;
      (c) every hypothesis with at least that many points below 1.1 th has exactly the true inliers below 1.1 th,
    so any rounding of the residuals that stays within 10 % of th selects the same inlier set.  A case that fails them is a
    broken fixture: the builder raises.
  * `judge_batch`: the judge / mirror over a (B,P) batch in the kernel's layouts, with its validity rules.
"""
import numpy as np

M64 = (1 << 64) - 1
RECIPE_COUNTS = (3, 4, 5, 40, 257, 1500, 4096)
RECIPE_SEEDS = tuple(range(8))


# ------------------------------------------------------------------------------------------------------------- algorithm
def umeyama(S, T, dt=np.float64):
    """S, T (..., K, 3) -> R (...,3,3), s (...), t (...,3): centre both; R = U diag(1,1,det(UV^T)) V^T of tgt_c^T src_c;
    s = sum (R src_c).tgt_c / (sum |R src_c|^2 + 1e-6); t = mean(tgt - s R src)."""
    S, T = S.astype(dt), T.astype(dt)
    sc, tc = S - S.mean(-2, keepdims=True), T - T.mean(-2, keepdims=True)
    M = np.swapaxes(tc, -1, -2) @ sc
    U, _, Vh = np.linalg.svd(M)
    d = np.linalg.det(U @ Vh)
    mid = np.zeros_like(U)
    mid[..., 0, 0] = 1
    mid[..., 1, 1] = 1
    mid[..., 2, 2] = d
    R = U @ mid @ Vh
    rs = sc @ np.swapaxes(R, -1, -2)
    s = (rs * tc).sum((-1, -2)) / ((rs * rs).sum((-1, -2)) + dt(1e-6))
    t = (np.swapaxes(T, -1, -2) - s[..., None, None] * (R @ np.swapaxes(S, -1, -2))).mean(-1)
    return R.astype(dt), s.astype(dt), t.astype(dt)


def residuals(S, T, R, s, t, dt=np.float64):
    """|tgt - (s R src + t)| of every member under every hypothesis -> (H, K)."""
    S_, T_ = S.astype(dt), T.astype(dt)
    pred = s[:, None, None] * np.einsum("hij,nj->hni", R, S_) + t[:, None, :]
    return np.sqrt(((T_[None] - pred) ** 2).sum(-1))


def fit(S, T, triples, th, dt=np.float64):
    """One part: S, T (K,3) fp32 members, triples (H,3) member ranks -> dict(score (H,), best, inliers (K,) bool, err (H,K),
    pose (R, s, t) of the refit or None when fewer than three inliers)."""
    with np.errstate(all="ignore"):
        R, s, t = umeyama(S[triples], T[triples], dt)
        err = residuals(S, T, R, s, t, dt)
        inl_all = err < dt(th)                       # a NaN error compares false: outside
        score = inl_all.sum(-1)
        best = int(np.argmax(score))
        inl = inl_all[best]
        pose = None
        if inl.sum() >= 3:
            R2, s2, t2 = umeyama(S[inl], T[inl], dt)
            pose = (R2, s2, t2)
    return dict(score=score, best=best, inliers=inl, err=err, pose=pose)


# ------------------------------------------------------------------------------------------------------------- generator
def mix(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw_ranks(seed, b, p, num_hyps, count):
    """The three distinct member ranks of every hypothesis of (b, p): (H,3) int, as captra_part_fit_ransac draws them when no
    sample_rank is given (include/captra_hip.h).  count >= 3."""
    assert count >= 3
    key = mix(seed + 0x9E3779B97F4A7C15)
    out = np.empty((num_hyps, 3), np.int64)
    for h in range(num_hyps):
        u = [mix(key ^ ((b << 32) | (p << 24) | (h << 8) | d)) >> 32 for d in range(3)]
        r0 = u[0] % count
        r1 = u[1] % (count - 1)
        r1 += r1 >= r0
        r2 = u[2] % (count - 2)
        r2 += r2 >= min(r0, r1)
        r2 += r2 >= max(r0, r1)
        out[h] = (r0, r1, r2)
    return out


# ----------------------------------------------------------------------------------------------------------------- cases
def random_rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] *= -1
    return q


def recipe_cloud(rng, count, outliers=True, ext=None):
    """Sources uniform in [-0.5, 0.5]^3; target = s R src + t with s in [0.05, 0.3] and t 1..3 m away; th = 0.02 s; Gaussian
    noise of 0.02 th on every point; for count >= 8, 30 % of the members replaced by points uniform in a cube of side 100 th
    around t.  ext: the scale s given (a batch shares one th).  -> S, T (count,3) fp32, th, true-inlier mask, (R, s, t)."""
    ext = rng.uniform(0.05, 0.3) if ext is None else ext
    th = 0.02 * ext
    S = (rng.random((count, 3)) - 0.5).astype(np.float32)
    R = random_rotation(rng)
    t = np.array([rng.uniform(-.5, .5), rng.uniform(-.5, .5), rng.uniform(1, 3)])
    T = ext * (S.astype(np.float64) @ R.T) + t + rng.normal(0, 0.02 * th, (count, 3))
    nout = int(0.3 * count) if (outliers and count >= 8) else 0
    out = rng.choice(count, nout, replace=False)
    T[out] = t + (rng.random((nout, 3)) - 0.5) * 100 * th
    true_in = np.ones(count, bool)
    true_in[out] = False
    return S, T.astype(np.float32), th, true_in, (R, ext, t)


def draw_triples(rng, count, num_hyps=64):
    """num_hyps triples without replacement, as the reference's random_choice_noreplace draws them."""
    return np.argpartition(rng.random((num_hyps, count)), 2, axis=-1)[:, :3]


def check_precondition(S, T, triples, th, true_in):
    """(a)-(c) of the module docstring, in float64; raises on a broken fixture.  Returns the judge's result."""
    j = fit(S, T, triples, th, np.float64)
    e = j["err"]
    best = int(j["score"].max())
    ntrue = int(true_in.sum())
    assert best == ntrue and (j["inliers"] == true_in).all(), ("(a)", best, ntrue)
    lo = (e < 0.9 * th).sum(-1)
    assert (lo == best).any(), ("(b)", int(lo.max()), best)
    hiset = e < 1.1 * th
    for h in np.nonzero(hiset.sum(-1) >= best)[0]:
        assert (hiset[h] == true_in).all(), ("(c)", int(h))
    return j


def recipe_case(seed, count, num_hyps=64, rng=None):
    """One case of the recipe, its precondition asserted: dict(S, T, th, triples, true_in, judge)."""
    rng = np.random.default_rng(seed * 100 + count) if rng is None else rng
    S, T, th, true_in, gt = recipe_cloud(rng, count)
    triples = draw_triples(rng, count, num_hyps)
    j = check_precondition(S, T, triples, th, true_in)
    return dict(S=S, T=T, th=th, triples=triples, true_in=true_in, judge=j, gt=gt)


# ----------------------------------------------------------------------------------------------------------------- batch
def judge_batch(labels, src, tgt, th, ranks, tgt_mean=None, dt=np.float64):
    """The kernel's layouts: labels (B,N), src (B,P,3,N), tgt (B,3,N) or (B,P,3,N), tgt_mean (B,3) or None (the target is then
    the fp32 sum tgt + mean, the kernel's input by definition), ranks (B,P,H,3) (rank r = the (r mod count)-th member).
    -> dict: rot (B,P,3,3), scale (B,P), trans (B,P,3) [identity / 1 / 0 where invalid], valid (B,P) bool, num_inliers (B,P),
    best (B,P), inliers: {(b,p): (N,) bool over the POINTS}."""
    B, P, _, N = src.shape
    if tgt_mean is not None:
        mean = tgt_mean.astype(np.float32).reshape((B, 3, 1) if tgt.ndim == 3 else (B, 1, 3, 1))
        tgt = (tgt.astype(np.float32) + mean).astype(np.float32)
    out = dict(rot=np.tile(np.eye(3), (B, P, 1, 1)), scale=np.ones((B, P)), trans=np.zeros((B, P, 3)), valid=np.zeros((B, P), bool),
               num_inliers=np.zeros((B, P), np.int64), best=np.zeros((B, P), np.int64), inliers={})
    for b in range(B):
        for p in range(P):
            pts = np.nonzero(labels[b] == p)[0]
            count = len(pts)
            mask = np.zeros(N, bool)
            out["inliers"][b, p] = mask
            if count < 3:
                continue
            S = src[b, p][:, pts].T
            T = (tgt[b, p] if tgt.ndim == 4 else tgt[b])[:, pts].T
            j = fit(S, T, np.asarray(ranks[b, p]) % count, th, dt)
            mask[pts[j["inliers"]]] = True
            out["best"][b, p], out["num_inliers"][b, p] = j["best"], int(j["inliers"].sum())
            if j["pose"] is None:
                continue
            R, s, t = j["pose"]
            if not (np.isfinite(R.astype(np.float32)).all() and np.isfinite(np.float32(s)) and np.isfinite(t.astype(np.float32)).all()):
                continue
            out["rot"][b, p], out["scale"][b, p], out["trans"][b, p], out["valid"][b, p] = R, s, t, True
    return out


def inlier_set(labels_b, src_bp, tgt_b, th, point_triple, dt=np.float64):
    """The inlier set (over the N points) of the hypothesis through the three POINT indices `point_triple`, for the members of
    one part: labels_b (N,) bool membership, src_bp (3,N), tgt_b (3,N) (mean already added)."""
    pts = np.nonzero(labels_b)[0]
    S, T = src_bp[:, pts].T, tgt_b[:, pts].T
    with np.errstate(all="ignore"):
        R, s, t = umeyama(src_bp[:, point_triple].T[None], tgt_b[:, point_triple].T[None], dt)
        err = residuals(S, T, R, s, t, dt)[0]
    mask = np.zeros(labels_b.shape[0], bool)
    mask[pts[err < dt(th)]] = True
    return mask


# ------------------------------------------------------------------------------------------------------------ batch cases
def members_of(case, b, p):
    """(pts, S (K,3), T (K,3)) of part (b, p) exactly as the kernel reads them: fp32, the mean added with one fp32 addition."""
    pts = np.nonzero(case["labels"][b] == p)[0]
    tgt = case["tgt"][b, p] if case["tgt"].ndim == 4 else case["tgt"][b]
    if case["tgt_mean"] is not None:
        tgt = (tgt + case["tgt_mean"][b][:, None]).astype(np.float32)
    return pts, case["src"][b, p][:, pts].T, tgt[:, pts].T


def batch_case(N, seed, per_part, with_mean, num_hyps=64, B=3, P=3):
    """A (B,P) batch in the kernel's layouts whose every part of >= 3 members is a recipe cloud (one scale, hence one th, for
    the batch), labels arranged as fit_case of tests/test_pose_readout_gpu.py arranges them:
      trajectory 0: random labels in [-2, P+1] (negative, P and P+1 belong to no part); its LAST part holds gross outliers only (targets uniform in a cube of side
                    1000 th: three of them are never similar enough to their sources' triangle to fit within th);
      trajectory 1: parts of 2, 3 and 4 members, the rest no part (B, P >= 3);
      trajectory 2: every point in part 0, the other parts empty.
    With B = 1 only trajectory 0 exists and keeps recipe clouds in every part.  NaN / Inf sit in half of the points that are not
    members (src: of the part; tgt: of the part / of any part).  ranks (B,P,H,3): triples without replacement.  The
    precondition is asserted for every recipe part, on the inputs as the kernel reads them (`check_batch`)."""
    rng = np.random.default_rng(seed)
    labels = np.empty((B, N), np.int32)
    labels[0] = rng.integers(-2, P + 2, N) if B > 1 else rng.choice(np.array([-1, 0, 0, 0, 1], np.int32), N)
    if B > 1:
        row = np.full(N, P, np.int32)
        row[:2], row[2:5], row[5:9] = 0, 1, 2
        row[9::2] = -1
        labels[1] = row[rng.permutation(N)]
        labels[2] = 0
    ext = rng.uniform(0.05, 0.3)
    th = 0.02 * ext
    src = (rng.random((B, P, 3, N)) - 0.5).astype(np.float32)
    full = np.empty((B, P, 3, N))
    full[:] = np.array([0.0, 0.0, 2.0])[:, None] + (rng.random((B, P, 3, N)) - 0.5)
    true_in = {}
    outlier_part = (0, P - 1) if B > 1 else None
    for b in range(B):
        for p in range(P):
            pts = np.nonzero(labels[b] == p)[0]
            if len(pts) == 0:
                continue
            S, T, _, tin, (_, _, t) = recipe_cloud(rng, len(pts), ext=ext)
            if (b, p) == outlier_part:
                T = t + (rng.random((len(pts), 3)) - 0.5) * 1000 * th
                tin = np.zeros(len(pts), bool)
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
                th=np.float32(th), ranks=ranks, true_in=true_in, outlier_part=outlier_part, per_part=per_part)
    check_batch(case, ranks)
    return case


def check_batch(case, ranks):
    """The precondition of every recipe part of `case` under the member ranks `ranks` (B,P,H,3); for the part of gross outliers:
    no hypothesis has three points below 1.1 th, so that fewer than three inliers is as immune to rounding."""
    th = float(case["th"])
    B, P = case["ranks"].shape[:2]
    for b in range(B):
        for p in range(P):
            pts, S, T = members_of(case, b, p)
            if len(pts) < 3:
                continue
            if (b, p) == case["outlier_part"]:
                j = fit(S, T, np.asarray(ranks[b, p]) % len(pts), th)
                assert ((j["err"] < 1.1 * th).sum(-1) < 3).all(), ("outlier part", b, p)
                lo, hi = (j["err"] < 0.9 * th).sum(-1), (j["err"] < 1.1 * th).sum(-1)
                assert (lo == hi).all(), ("outlier part: a residual within 10 % of th", b, p)
            else:
                check_precondition(S, T, np.asarray(ranks[b, p]) % len(pts), th, case["true_in"][b, p])
