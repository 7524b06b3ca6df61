"""A float64 judge for the robust rotation read-out (captra_rot_pool_consensus; tests/test_rot_consensus_gpu.py,
tests/test_rot_consensus_cpu.py).

  * `votes` / `scores` / `pool` / `fit`: the semantics of include/captra_hip.h restated with numpy for ONE part, from the fp32 `raw`
    as stored to the per-point votes, the score of every hypothesis, the first best one, its inlier set and the pooled dR.
    dt = float64 is the judge, dt = float32 the same algorithm in float32 (every product and sum rounded separately, the dot
    products in the kernel's order), the MIRROR.
  * `hyp_ranks`: the kernel's draws (ransac_judge.draw_ranks' first column; its generator for parts of fewer than three members).
  * `recipe_part` / `check_precondition` / `pinned_best`: the test inputs and what makes them decidable, the rules of
    st_ransac_judge in terms of ANGLES: in float64
      (a) the best score equals the number of true votes and best's inliers are the true ones;
      (b) some hypothesis has all true votes inside 0.9 th;
      (c) every hypothesis with at least that many votes inside 1.1 th has exactly the true ones inside 1.1 th,
    so any rounding that moves an angle by less than 10 % of th selects the same inlier set; pinned_best: the first hypothesis
    that can reach the top score within 1.1 th reaches it within 0.9 th, so `best` itself is as immune.
  * `batch_case` / `check_batch` / `judge_batch`: a (B,P) batch in the kernel's layouts with every kind of part.
"""
import numpy as np

from tests.ransac_judge import draw_ranks, mix, random_rotation

TH_DEG = 15.0


def cos_th_of(angle_deg):
    """The kernel's threshold as the wrapper forms it: float32(cos(float64 radians))."""
    return np.float32(np.cos(np.deg2rad(np.float64(angle_deg))))


# ------------------------------------------------------------------------------------------------------------- algorithm
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _normalize3(v):
    """rotations.py:302-314 as the kernels write it: v / max(|v|, 1e-8) where |v| > 1e-8, else (1,0,0) -- a NaN magnitude too."""
    dt = v.dtype.type
    with np.errstate(all="ignore"):
        mag = np.sqrt(_dot(v, v))
        ok = mag > dt(1e-8)
        out = v / np.maximum(mag, dt(1e-8))[..., None]
    return np.where(ok[..., None], out, np.array([1, 0, 0], v.dtype))


def _cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def votes(raw, sym, dt=np.float64):
    """raw (R,K) fp32 -> sym: (K,1,3) the unit axis; else (K,3,3) with [k, c] = column c (x, y, z) of the ortho6d frame."""
    r = raw.astype(dt).T
    with np.errstate(all="ignore"):
        if sym:
            return _normalize3(r[:, :3])[:, None, :]
        x = _normalize3(r[:, :3])
        z = _normalize3(_cross(x, r[:, 3:6]))
        y = _cross(z, x)
    return np.stack([x, y, z], 1)


def agreement(Vh, V):
    """(H,K): sym d = v_h . v_i; else tr = ((x_h.x_i) + (y_h.y_i)) + (z_h.z_i).  Separately rounded in V's dtype."""
    with np.errstate(all="ignore"):
        d = _dot(Vh[:, None, :, :], V[None, :, :, :])          # (H,K,C)
        return d[..., 0] if d.shape[-1] == 1 else (d[..., 0] + d[..., 1]) + d[..., 2]


def angles(agree, sym):
    """The angle (radians, float64) an agreement value stands for; NaN stays NaN."""
    with np.errstate(all="ignore"):
        c = agree.astype(np.float64) if sym else (agree.astype(np.float64) - 1.0) / 2.0
        return np.arccos(np.clip(c, -1.0, 1.0))


def frame(mean, sym, nothing, dt):
    """The tail of the read-out: mean (3,) axis or (3,3) row-major matrix (columns x, y, z) -> dR (3,3)."""
    one = dt(1e-8)
    with np.errstate(all="ignore"):
        if sym:
            v = np.array([0, 1, 0], dt) if nothing else mean
            y = _normalize3(v)
            z = _normalize3(_cross(np.array([1, 0, 0], dt), y))
            x = _cross(y, z)
            return np.stack([x, y, z], 1)
        m = np.eye(3, dtype=dt) if nothing else mean
        a1, a2, a3 = m[:, 0], m[:, 1], m[:, 2]
        u2 = a2 - (_dot(a1, a2) / np.maximum(_dot(a1, a1), one)) * a1
        k13 = _dot(a1, a3) / np.maximum(_dot(a1, a1), one)
        k23 = _dot(u2, a3) / np.maximum(_dot(u2, u2), one)
        u3 = (a3 - k13 * a1) - k23 * u2
        return np.stack([_normalize3(a1), _normalize3(u2), _normalize3(u3)], 1)


def pool(V, mask, sym, dt=np.float64):
    """Masked mean of the votes V[mask] and its frame -> dR (3,3) in dt."""
    n = int(mask.sum())
    if n == 0:
        return frame(None, sym, True, dt)
    with np.errstate(all="ignore"):
        s = V[mask].sum(0, dtype=dt) / dt(n)                   # (C,3): [c] = column c
    return frame(s[0] if sym else s.T, sym, False, dt)


def fit(raw, ranks, cos_th, sym, dt=np.float64):
    """One part: raw (R,K) fp32 of the MEMBERS, ranks (H,) member ranks, cos_th the fp32 threshold -> dict(score (H,), best,
    inliers (K,) bool, agree (H,K), dR (3,3))."""
    K = raw.shape[1]
    if K == 0:
        return dict(score=np.zeros(len(ranks), np.int64), best=0, inliers=np.zeros(0, bool), agree=np.zeros((len(ranks), 0)),
                    dR=frame(None, sym, True, dt))
    V = votes(raw, sym, dt)
    agree = agreement(V[np.asarray(ranks) % K], V)
    thr = dt(cos_th) if sym else dt(1) + dt(2) * dt(cos_th)
    with np.errstate(all="ignore"):
        inl_all = agree > thr                                  # a NaN compares false
    score = inl_all.sum(-1)
    best = int(np.argmax(score))
    return dict(score=score, best=best, inliers=inl_all[best], agree=agree, dR=pool(V, inl_all[best], sym, dt))


def hyp_ranks(seed, b, p, num_hyps, count):
    """r_h of every hypothesis of (b, p) as the kernel draws it without sample_rank: u(0) mod count."""
    if count >= 3:
        return draw_ranks(seed, b, p, num_hyps, count)[:, 0]
    key = mix(seed + 0x9E3779B97F4A7C15)
    return np.array([(mix(key ^ ((b << 32) | (p << 24) | (h << 8))) >> 32) % max(count, 1) for h in range(num_hyps)], np.int64)


# ----------------------------------------------------------------------------------------------------------------- cases
def exp_so3(w):
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def _small(rng, bound):
    w = rng.normal(size=3)
    return w / np.linalg.norm(w) * rng.uniform(0, bound)


def rot_x(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])


def raw_of(rng, R, sym):
    """The head output that stands for the vote R (3,3): sym (3,) = R's y-axis times a positive length; else (6,) = the first column
    times a length, and a vector in the plane of the first two columns -- the second times a length, skewed by a multiple of the first."""
    if sym:
        return R[:, 1] * rng.uniform(0.2, 3.0)
    return np.concatenate([R[:, 0] * rng.uniform(0.2, 3.0), R[:, 1] * rng.uniform(0.2, 3.0) + R[:, 0] * rng.uniform(-1.0, 1.0)])


def recipe_part(rng, count, sym, th_deg=TH_DEG, outliers=True):
    """count members: 70 % true votes R_true Exp(w), |w| <= 0.3 th; half of the rest clustered at R_true R_x(90 deg) Exp(w) (the agreeing
    second surface); the other half uniform on SO(3), none closer than 2 th to R_true (sym: the y-axes compared).
    -> raw (R,count) fp32, true mask (count,), R_true."""
    th = np.deg2rad(th_deg)
    R_true = random_rotation(rng)
    ntrue = count - (int(0.3 * count) if outliers else 0)
    nclu = (count - ntrue) // 2
    kind = np.zeros(count, np.int64)
    kind[rng.permutation(count)[:count - ntrue]] = 1
    out = np.nonzero(kind == 1)[0]
    kind[out[nclu:]] = 2
    raw = np.empty((3 if sym else 6, count))
    for i in range(count):
        if kind[i] == 0:
            R = R_true @ exp_so3(_small(rng, 0.3 * th))
        elif kind[i] == 1:
            R = R_true @ rot_x(np.pi / 2) @ exp_so3(_small(rng, 0.3 * th))
        else:
            while True:
                R = random_rotation(rng)
                c = R[:, 1] @ R_true[:, 1] if sym else (np.trace(R_true.T @ R) - 1) / 2
                if np.arccos(np.clip(c, -1, 1)) >= 2 * th:
                    break
        raw[:, i] = raw_of(rng, R, sym)
    return raw.astype(np.float32), kind == 0, R_true


def check_precondition(raw, ranks, th_deg, true_in, sym):
    """(a)-(c) of the module docstring, in float64; raises on a broken fixture.  Returns the judge's result."""
    j = fit(raw, ranks, cos_th_of(th_deg), sym)
    ang, th = angles(j["agree"], sym), np.deg2rad(th_deg)
    top, ntrue = int(j["score"].max()), int(true_in.sum())
    assert top == ntrue and (j["inliers"] == true_in).all(), ("(a)", top, ntrue)
    lo = (ang < 0.9 * th).sum(-1)
    assert (lo == top).any(), ("(b)", int(lo.max()), top)
    hiset = ang < 1.1 * th
    for h in np.nonzero(hiset.sum(-1) >= top)[0]:
        assert (hiset[h] == true_in).all(), ("(c)", int(h))
    return j


def pinned_best(j, th_deg, sym):
    ang, th, top = angles(j["agree"], sym), np.deg2rad(th_deg), int(j["score"].max())
    first = int(np.nonzero((ang < 1.1 * th).sum(-1) >= top)[0][0])
    return first == j["best"] and int((ang[first] < 0.9 * th).sum()) == top


def plain_mean_angle(raw, sym, R_true, mask=None):
    """How far (degrees) the plain read-out's dR of the members (or of raw[:, mask]) is from R_true, in float64."""
    V = votes(raw, sym)
    dR = pool(V, np.ones(len(V), bool) if mask is None else mask, sym)
    c = dR[:, 1] @ R_true[:, 1] if sym else (np.trace(R_true.T @ dR) - 1) / 2
    return float(np.rad2deg(np.arccos(np.clip(c, -1, 1))))


# ----------------------------------------------------------------------------------------------------------------- batch
def batch_case(N, seed, sym, num_hyps=64, P=3, th_deg=TH_DEG, diag=True, outliers=True, nan_part=(0, 1)):
    """B = 3 trajectories of P = 3 parts in the kernel's layouts:
      trajectory 0: random labels in [-2, P+1] (negative, P and P+1 belong to no part): three recipe parts -- of which `nan_part`
                    (None: none) is replaced by members whose raw is all NaN;
      trajectory 1: parts of 0, 1 and 2 members (the two within 0.3 th of each other), the rest labelled P;
      trajectory 2: every point in part 0 (recipe), parts 1 and 2 empty.
    raw (B*P,R,N) (diag) or (B*P,P,R,N): random finite values everywhere, NaN in half of the points that are not members of the
    part, the recipe's values at the members (head p of cloud (b,p); the other heads of a non-diagonal raw stay random).
    prev_rot (B,P,3,3) random rotations; ranks (B,P,H) uniform member ranks.  The preconditions are asserted (`check_batch`)."""
    B = 3
    rng = np.random.default_rng(seed)
    R = 3 if sym else 6
    labels = np.empty((B, N), np.int32)
    labels[0] = rng.integers(-2, P + 2, N)
    row = np.full(N, P, np.int32)
    row[0], row[1:3] = 1, 2
    labels[1] = row[rng.permutation(N)]
    labels[2] = 0
    head = rng.normal(size=(B, P, R, N))
    member = labels[:, None, :] == np.arange(P)[None, :, None]
    head = np.where((~member & (rng.random((B, P, N)) < 0.5))[:, :, None, :], np.nan, head)
    true_in, R_true = {}, {}
    for b in range(B):
        for p in range(P):
            pts = np.nonzero(labels[b] == p)[0]
            if len(pts) == 0:
                continue
            if b == 1:       # one member; two members that agree
                Rt = random_rotation(rng)
                vals = np.stack([raw_of(rng, Rt @ exp_so3(_small(rng, 0.15 * np.deg2rad(th_deg))), sym) for _ in pts], 1)
                tin = np.ones(len(pts), bool)
            else:
                vals, tin, Rt = recipe_part(rng, len(pts), sym, th_deg, outliers)
            if (b, p) == nan_part:
                vals, tin = np.full_like(vals, np.nan), None
            head[b, p][:, pts], true_in[b, p], R_true[b, p] = vals, tin, Rt
    if diag:
        raw = head.reshape(B * P, R, N)
    else:
        raw = rng.normal(size=(B, P, P, R, N))
        for p in range(P):
            raw[:, p, p] = head[:, p]
        raw = raw.reshape(B * P, P, R, N)
    ranks = rng.integers(0, 1 << 20, (B, P, num_hyps)).astype(np.int32)
    prev = np.stack([random_rotation(rng) for _ in range(B * P)]).reshape(B, P, 3, 3)
    case = dict(labels=labels, raw=np.ascontiguousarray(raw, np.float32), head=np.ascontiguousarray(head, np.float32),
                prev_rot=np.ascontiguousarray(prev, np.float32), ranks=ranks, true_in=true_in, R_true=R_true, sym=bool(sym),
                th_deg=float(th_deg), nan_part=nan_part, diag=diag)
    check_batch(case)
    return case


def members_of(case, b, p):
    pts = np.nonzero(case["labels"][b] == p)[0]
    return pts, case["head"][b, p][:, pts]


def check_batch(case, ranks=None, pin=False):
    """The preconditions of every part of `case` that has members and is not the NaN part, under the member ranks `ranks` (B,P,H);
    pin: and `pinned_best`."""
    ranks = case["ranks"] if ranks is None else ranks
    B, P = case["ranks"].shape[:2]
    for b in range(B):
        for p in range(P):
            pts, raw = members_of(case, b, p)
            if len(pts) == 0 or case["true_in"][b, p] is None:
                continue
            j = check_precondition(raw, np.asarray(ranks[b, p]) % len(pts), case["th_deg"], case["true_in"][b, p], case["sym"])
            assert not pin or pinned_best(j, case["th_deg"], case["sym"]), ("best not pinned", b, p)


def judge_batch(case, ranks=None, dt=np.float64):
    """-> dict: rot, delta (B,P,3,3), count, num_inliers, best (B,P), inliers {(b,p): (N,) bool over the POINTS}."""
    ranks = case["ranks"] if ranks is None else ranks
    B, P = case["ranks"].shape[:2]
    N = case["labels"].shape[1]
    out = dict(rot=np.zeros((B, P, 3, 3), dt), delta=np.zeros((B, P, 3, 3), dt), count=np.zeros((B, P), np.int64),
               num_inliers=np.zeros((B, P), np.int64), best=np.zeros((B, P), np.int64), inliers={})
    cos_th = cos_th_of(case["th_deg"])
    for b in range(B):
        for p in range(P):
            pts, raw = members_of(case, b, p)
            j = fit(raw, np.asarray(ranks[b, p]) % max(len(pts), 1), cos_th, case["sym"], dt)
            mask = np.zeros(N, bool)
            mask[pts[j["inliers"]]] = True
            out["inliers"][b, p] = mask
            out["count"][b, p], out["num_inliers"][b, p], out["best"][b, p] = len(pts), int(j["inliers"].sum()), j["best"]
            out["delta"][b, p] = j["dR"]
            out["rot"][b, p] = case["prev_rot"][b, p].astype(dt) @ j["dR"]
    return out


def inlier_set(case, b, p, best_rank):
    """The inlier set (over the N points) of the vote of member rank `best_rank`, in float64."""
    pts, raw = members_of(case, b, p)
    mask = np.zeros(case["labels"].shape[1], bool)
    if len(pts):
        V = votes(raw, case["sym"])
        a = agreement(V[[best_rank % len(pts)]], V)[0]
        c = np.float64(cos_th_of(case["th_deg"]))
        with np.errstate(all="ignore"):
            mask[pts[a > (c if case["sym"] else 1.0 + 2.0 * c)]] = True
    return mask
