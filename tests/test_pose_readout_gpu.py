"""The pose read-out kernels against plain numpy float64 references, on the shapes and the degenerate inputs where they go wrong.

  * captra_procrustes_rot3 (pose_fit.hip): conditioning sweep over chosen singular values, both signs of det, three overall
    scales; rank <= 1, tiny and empty clouds.  Every result must be a finite proper rotation that maximises tr(R^T M) -- the
    assertion that stays meaningful where the optimal rotation is not unique -- and, where it is unique, equal the float64
    U diag(1,1,d) V^T.
  * captra_part_fit_st / captra_part_fit_st_track (pose_fit.hip): the algebra of the kernel's header comment restated in
    float64, on targets shaped like a depth crop (small extent, metres away: t - t_bar cancels), with part sizes 0 / 3 / 4 / N,
    labels outside [0, P), NaN / Inf in non-member and in member points, a non-orthonormal rotation, a zero 2x2
    cross-covariance.
  * captra_seg_softmax_argmax (track_ops.hip): softmax / first-index arg max in float64 with logits at +-1e4 and +-80, a
    class at -inf, exact ties, both nullable outputs, the refused S = 9, and a NaN logit.

Every reference is computed from the fp32 inputs as stored, so input rounding is not counted as kernel error.  The case
builders and references need numpy only; tests/test_oracle_properties.py runs the Procrustes ones against the CPU oracle.
"""
import numpy as np
import pytest

F32_EPS = float(np.finfo(np.float32).eps)      # 2^-23


# ===================================================================================== 3x3 Procrustes: cases and reference
SIGMA_PATTERNS = {
    "reference": (1.0, 1.0, 1.0),
    "mild_spread": (1.0, 0.5, 0.25),
    "rank2": (1.0, 0.5, 0.0),
    "near_rank1": (1.0, 1e-3, 1e-6),
    "wide_spread": (1.0, 1e-6, 1e-6 * 0.5),
}
SWEEP_SCALES = (1e-12, 1.0, 1e12)
SWEEP_N = (255, 256, 257, 4096, 100000)
UNIQUE_MIN = 1e-3          # the optimum counts as unique where (sigma_2 + d sigma_3) / sigma_1 >= this
# The sweep cases whose optimum is unique by that rule; every one of them is compared as a matrix (the sweep functions assert
# that exactly these were).  The others -- isotropic with d = -1 (ratio 0), near_rank1 with d = -1 (0.999e-3) and wide_spread
# (1.5e-6, 0.5e-6) -- are held to finiteness, orthonormality, det = +1 and optimality.
SWEEP_UNIQUE = {("reference", 1), ("mild_spread", 1), ("mild_spread", -1), ("rank2", 1), ("rank2", -1), ("near_rank1", 1)}

# |R^T R - I| <= 1e-6: fp32 rounding of the nine entries (each off by <= 2^-24 |r|, three products per entry of R^T R, two
# entries per product: <= 6 * 6e-8 = 3.6e-7 at worst).  Measured: CPU oracle 7.4e-8 over the whole sweep and all named cases.
ORTHO_ATOL = 1e-6
# det R = +1: |det R|^2 = det(R^T R), and |R^T R - I| <= 1e-6 entrywise bounds |det(R^T R) - 1| by 3e-6, so a proper rotation
# that passes the line above has |det R - 1| <= 1.5e-6; 2e-6 leaves the rounding of the check itself.  Measured: oracle 7.6e-8.
DET_ATOL = 2e-6
# Optimality tol: 8 x the worst gap (sigma_1 + sigma_2 + d sigma_3 - tr(R^T M)) / sigma_1 of the CPU oracle over the sweep at
# every n of SWEEP_N and the named cases.  Measured worst gap: 7.57e-8 (reference/d=+1/scale=1e12/n=256; the first-order effect of rounding R to fp32); the
# factor covers a different rounding of R, M being the float64 one in both.
OPT_TOL = 8 * 7.6e-8
# Matrix comparison: the atol of test_procrustes_rot3_vs_golden where (sigma_2 + d sigma_3) / sigma_1 >= 0.1, scaled by
# sigma_1 / (sigma_2 + d sigma_3), the conditioning of the rotation, below.  Measured: oracle 3.0e-8 where the ratio is
# >= 0.1, 3.0e-8 at near_rank1 d=+1 (ratio 1.001e-3, bound 2e-2).
MATRIX_ATOL = 2e-5


def _random_rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 2] = -q[:, 2]
    return q


def sweep_cloud(n, sigma, d, scale, seed):
    """src = sqrt(n) x three orthonormal centred columns (src^T src = n I), tgt = scale * src A^T with
    A = U diag(sigma_1, sigma_2, d sigma_3) V^T: M = tgt^T src = scale n A has the singular values chosen.  fp32 (n,3) x2."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((n, 3))
    q, _ = np.linalg.qr(g - g.mean(0))
    src = np.sqrt(n) * q
    a = _random_rotation(rng) @ np.diag([sigma[0], sigma[1], d * sigma[2]]) @ _random_rotation(rng).T
    return src.astype(np.float32), (scale * (src @ a.T)).astype(np.float32)


def sweep_cases(n):
    """[(name, pattern, d, src, tgt)]: every sigma pattern x both signs of det(A) x the three overall scales, at n points."""
    out = []
    for pi, (pat, sigma) in enumerate(SIGMA_PATTERNS.items()):
        for d in (1, -1):
            for si, scale in enumerate(SWEEP_SCALES):
                src, tgt = sweep_cloud(n, sigma, d, scale, seed=1000 * n + 100 * pi + 10 * (d < 0) + si)
                out.append((f"{pat}/d={d:+d}/scale={scale:g}/n={n}", pat, d, src, tgt))
    return out


def degenerate_cases():
    """[(name, src, tgt)] fp32 (n,3): rank <= 1 cross-covariances, tiny and empty clouds, a non-unique optimum."""
    rng = np.random.default_rng(77)
    out = []
    # collinear, exactly: small-integer multiples of two vectors with short mantissas -- every product is exact, M has rank 1
    a, b = rng.integers(-8, 9, 64).astype(np.float64), rng.integers(-8, 9, 64).astype(np.float64)
    s, t = np.array([0.5, -1.25, 2.0]), np.array([-0.75, 0.5, 1.5])
    out.append(("collinear_exact", a[:, None] * s, b[:, None] * t))
    # collinear up to the fp32 rounding of the points: sigma_2 / sigma_1 ~ 1e-8
    a, b = rng.standard_normal(300), rng.standard_normal(300)
    s, t = rng.standard_normal(3), rng.standard_normal(3)
    out.append(("collinear_rounded", a[:, None] * s, b[:, None] * t))
    out.append(("collinear_along_x", a[:, None] * np.array([1.0, 0, 0]), b[:, None] * np.array([1.0, 0, 0])))
    out.append(("collinear_src_only", a[:, None] * s, rng.standard_normal((300, 3))))
    out.append(("all_identical", np.tile(rng.standard_normal(3), (100, 1)), np.tile(rng.standard_normal(3), (100, 1))))
    # the same along coordinate axes: M has a single non-zero entry, M v2 is exactly 0 (no rounding noise to normalise)
    out.append(("all_identical_on_axes", np.tile([0.0, 0.0, 1.5], (100, 1)), np.tile([2.0, 0.0, 0.0], (100, 1))))
    out.append(("n=1_on_axes", np.array([[1.0, 0.0, 0.0]]), np.array([[0.0, -2.0, 0.0]])))
    out.append(("all_zero", np.zeros((50, 3)), np.zeros((50, 3))))
    out.append(("src_zero", np.zeros((50, 3)), rng.standard_normal((50, 3))))
    for n in (0, 1, 2, 3):
        out.append((f"n={n}", rng.standard_normal((n, 3)), rng.standard_normal((n, 3))))
    p = rng.standard_normal((2, 3))
    out.append(("n=2_centred", p - p.mean(0), (p - p.mean(0)) @ _random_rotation(rng).T))      # rank 1
    p = rng.standard_normal((3, 3))
    out.append(("n=3_centred", p - p.mean(0), (p - p.mean(0)) @ _random_rotation(rng).T))      # rank 2
    src, tgt = sweep_cloud(256, (1.0, 1.0, 1.0), -1, 1.0, seed=5)
    out.append(("isotropic_reflected", src, tgt))                                              # sigma_2 = sigma_3, d = -1
    return [(name, np.ascontiguousarray(s_, np.float32), np.ascontiguousarray(t_, np.float32)) for name, s_, t_ in out]


def procrustes_ref(src, tgt):
    """float64 from the fp32 points: M = tgt^T src = U S V^T -> (M, sigma (3,), d = det(U V^T), R = U diag(1,1,d) V^T)."""
    m = tgt.astype(np.float64).T @ src.astype(np.float64)
    u, sig, vt = np.linalg.svd(m)
    d = 1.0 if np.linalg.det(u) * np.linalg.det(vt) >= 0 else -1.0
    return m, sig, d, u @ np.diag([1.0, 1.0, d]) @ vt


def rotation_figures(rot, src, tgt):
    """The measured figures of one result: (finite, max |R^T R - I|, |det R - 1|, optimality gap / sigma_1, max |R - R_ref|,
    (sigma_2 + d sigma_3) / sigma_1)."""
    m, sig, d, ref = procrustes_ref(src, tgt)
    r = np.asarray(rot, np.float64)
    finite = bool(np.isfinite(r).all())
    s1 = sig[0]
    gap = (sig[0] + sig[1] + d * sig[2]) - np.trace(r.T @ m)
    return (finite, np.abs(r.T @ r - np.eye(3)).max(), abs(np.linalg.det(r) - 1.0), gap / s1 if s1 > 0 else gap,
            np.abs(r - ref).max(), (sig[1] + d * sig[2]) / s1 if s1 > 0 else 0.0)


def check_rotation(rot, src, tgt, name, compare_matrix):
    """Assert what every result must satisfy, and the matrix comparison where the optimum is unique.  Returns the figures."""
    fig = rotation_figures(rot, src, tgt)
    finite, ortho, det, gap, diff, ratio = fig
    assert finite, (name, np.asarray(rot))
    assert ortho <= ORTHO_ATOL, (name, ortho)                    # oracle measured 7.4e-8, see ORTHO_ATOL
    assert det <= DET_ATOL, (name, det)                          # oracle measured 7.6e-8, see DET_ATOL
    assert gap <= OPT_TOL, (name, gap)                           # oracle measured 7.57e-8 sigma_1, see OPT_TOL
    if compare_matrix:
        assert ratio >= UNIQUE_MIN, (name, ratio)
        atol = MATRIX_ATOL if ratio >= 0.1 else MATRIX_ATOL / ratio
        assert diff <= atol, (name, diff, atol)                  # oracle measured 3.0e-8 / 3.0e-8, see MATRIX_ATOL
    return fig


def check_sweep(n, solve):
    """The whole sweep at n points through `solve(src (n,3), tgt (n,3)) -> (3,3)`; returns {name: rotation}."""
    compared, got = set(), {}
    for name, pat, d, src, tgt in sweep_cases(n):
        unique = (pat, d) in SWEEP_UNIQUE
        got[name] = np.asarray(solve(src, tgt))
        check_rotation(got[name], src, tgt, name, compare_matrix=unique)
        if unique:
            compared.add((pat, d))
    assert compared == SWEEP_UNIQUE          # no case with a unique optimum was left out of the matrix comparison
    return got


# ============================================================================================ scale / translation fit
def part_fit_ref(labels, src, tgt, rot, sym, given_scale=None, tgt_mean=None):
    """The algebra of pose_fit.hip's header comment in float64.  labels (B,N) int, src (B,P,3,N), tgt (B,3,N) or (B,P,3,N),
    rot (B,P,3,3), given_scale (B,P) or None, tgt_mean (B,3) or None (the target is then the fp32 sum tgt + mean, the
    kernel's input by definition) -> scale (B,P), trans (B,P,3), valid (B,P) bool."""
    B, P, _, N = src.shape
    if tgt_mean is not None:
        tgt = (tgt.astype(np.float32) + tgt_mean.astype(np.float32)[:, :, None]).astype(np.float32)
    scale, trans, valid = np.zeros((B, P)), np.zeros((B, P, 3)), np.zeros((B, P), bool)
    with np.errstate(all="ignore"):
        for b in range(B):
            for p in range(P):
                m = labels[b] == p
                c = int(m.sum())
                S = src[b, p][:, m].astype(np.float64)
                T = (tgt[b, p] if tgt.ndim == 4 else tgt[b])[:, m].astype(np.float64)
                sb, tb = S.sum(1) / max(c, 1), T.sum(1) / max(c, 1)
                Sc, Tc = S - sb[:, None], T - tb[:, None]
                C = Tc @ Sc.T
                R = rot[b, p].astype(np.float64)
                Rf = R
                if sym:
                    M = (R.T @ C)[np.ix_([0, 2], [0, 2])]
                    a, cc = M[0, 0] + M[1, 1], M[1, 0] - M[0, 1]
                    h = np.sqrt(a * a + cc * cc)
                    cs, sn = (a / h, cc / h) if h > 0 else ((np.nan, np.nan) if h != h else (1.0, 0.0))
                    Rf = R @ np.array([[cs, 0, -sn], [0, 1, 0], [sn, 0, cs]])
                num = (Rf * C).sum()
                dn = ((Rf @ Sc) ** 2).sum()
                sca = float(given_scale[b, p]) if given_scale is not None else num / (dn + 1e-6)
                tr = tb - sca * (Rf @ sb) if c > 0 else np.zeros(3)
                scale[b, p], trans[b, p] = sca, tr
                valid[b, p] = (c > 3 and np.isfinite(np.float32(sca)) and np.isfinite(tr.astype(np.float32).sum())
                               and np.isfinite(R.sum()))
    return scale, trans, valid


def part_fit_mirror(labels, src, tgt, rot, sym, given_scale=None, tgt_mean=None):
    """The package's own fp32 torch mirror, procrustes.transform_pts_mask with the rotation given, on CPU tensors (no kernel
    is launched) -> scale (B,P), trans (B,P,3) as float64.  The mirror multiplies by the mask, and NaN * 0 is NaN: points that
    are not members of a part are zeroed in its inputs, which changes none of its sums."""
    import torch
    from captra_amd.pose_utils import procrustes as PR
    B, P, _, N = src.shape
    if tgt_mean is not None:
        tgt = (tgt.astype(np.float32) + tgt_mean.astype(np.float32)[:, :, None]).astype(np.float32)
    mask = labels[:, None, :] == np.arange(P)[None, :, None]                                   # (B,P,N)
    tgt_pp = tgt if tgt.ndim == 4 else np.broadcast_to(tgt[:, None], src.shape)
    s_ = np.where(mask[:, :, None, :], src, np.float32(0)).transpose(0, 1, 3, 2)
    t_ = np.where(mask[:, :, None, :], tgt_pp, np.float32(0)).transpose(0, 1, 3, 2)
    tt = lambda a, dt=np.float32: torch.from_numpy(np.ascontiguousarray(a, dtype=dt))        # noqa: E731
    w = tt(mask[..., None])
    gs = None if given_scale is None else tt(given_scale)
    _, scale, trans = PR.transform_pts_mask(tt(s_), tt(t_), w, w, given_scale=gs, rotation=tt(rot), sym=sym)
    return scale.numpy().astype(np.float64), trans.numpy()[..., 0].astype(np.float64)


def fit_bounds(ref_s, ref_t, mir_s, mir_t):
    """Per part: the kernel may be at most 2 x as far from float64 as the fp32 mirror, with a floor of 4 fp32 ulps of the
    output's magnitude (for the translation: of its largest component, the three mix under the rotation)."""
    bs = np.maximum(2 * np.abs(mir_s - ref_s), 4 * F32_EPS * np.abs(ref_s))
    bt = np.maximum(2 * np.abs(mir_t - ref_t).max(-1), 4 * F32_EPS * np.abs(ref_t).max(-1))
    return bs, bt


def fit_case(N, seed, per_part=False, poison=False, skew_rot=False):
    """A batch of B = 3 trajectories x P = 3 parts shaped like a depth crop: NOCS-like sources in [-0.5, 0.5]^3, targets
    s R src + t with s in [0.05, 0.2] (the extent) and t 1..3 m away, plus 1 mm noise.
      trajectory 0: random labels in [-2, P+1] -- negative, the background P and P+1 all belong to no part;
      trajectory 1: part 0 empty, part 1 three points (invalid), part 2 four (the first valid size), the rest no part
                    (as far as N allows);
      trajectory 2: every point in part 0.
    poison: NaN and +-Inf in points that are NOT members of the part (src) / of any part the target serves (tgt).
    skew_rot: the given rotation is not orthonormal (scaled and sheared)."""
    rng = np.random.default_rng(seed)
    B, P = 3, 3
    labels = np.empty((B, N), np.int32)
    labels[0] = rng.integers(-2, P + 2, N)
    row = np.full(N, P, np.int32)
    row[:3] = 1
    row[3:7] = 2
    row[7::2] = -1
    labels[1] = row[rng.permutation(N)] if N > 7 else row
    labels[2] = 0
    src = (rng.random((B, P, 3, N)) - 0.5).astype(np.float32)
    rot = np.stack([_random_rotation(rng) for _ in range(B * P)]).reshape(B, P, 3, 3)
    s_gt = rng.uniform(0.05, 0.2, (B, P))
    t_gt = np.concatenate([rng.uniform(-0.5, 0.5, (B, P, 2)), rng.uniform(1.0, 3.0, (B, P, 1))], -1)
    full = s_gt[..., None, None] * np.einsum("bpij,bpjn->bpin", rot, src.astype(np.float64)) + t_gt[..., None]
    full += rng.normal(0, 1e-3, full.shape)
    if per_part:
        tgt = full.astype(np.float32)
    else:       # one target cloud per trajectory: each point follows the part it is labelled with, the others part 0
        sel = np.clip(labels, 0, P - 1)
        sel = np.where((labels >= 0) & (labels < P), sel, 0)
        tgt = np.take_along_axis(full, sel[:, None, None, :], axis=1)[:, 0].astype(np.float32)
    if skew_rot:
        rot = rot @ (np.eye(3) + np.array([[0.3, 0.2, 0.0], [0.0, -0.2, 0.1], [0.1, 0.0, 0.4]]))
    rot = rot.astype(np.float32)
    if poison:
        bad = np.array([np.nan, np.inf, -np.inf], np.float32)
        member = labels[:, None, :] == np.arange(P)[None, :, None]                             # (B,P,N)
        hit = ~member & (rng.random((B, P, N)) < 0.5)
        src = np.where(hit[:, :, None, :], bad[rng.integers(0, 3, src.shape)], src)
        if per_part:
            hit_t = ~member & (rng.random((B, P, N)) < 0.5)
            tgt = np.where(hit_t[:, :, None, :], bad[rng.integers(0, 3, tgt.shape)], tgt)
        else:
            hit_t = ~member.any(1) & (rng.random((B, N)) < 0.5)
            tgt = np.where(hit_t[:, None, :], bad[rng.integers(0, 3, tgt.shape)], tgt)
    return dict(labels=labels, src=np.ascontiguousarray(src, np.float32), tgt=np.ascontiguousarray(tgt, np.float32), rot=rot)


FIT_N = (1, 7, 255, 256, 257, 1001, 4096, 16384)


def check_fit(got, case, sym, given_scale=None, tgt_mean=None, prev=None):
    """got = (scale (B,P), trans (B,P,3), valid (B,P)) of the kernel as numpy; prev = (prev_scale, prev_trans) for the track
    form, where an invalid fit must return them bit for bit."""
    s, t, v = (np.asarray(x) for x in got)
    args = (case["labels"], case["src"], case["tgt"], case["rot"], sym)
    rs, rt, rv = part_fit_ref(*args, given_scale=given_scale, tgt_mean=tgt_mean)
    ms, mt = part_fit_mirror(*args, given_scale=given_scale, tgt_mean=tgt_mean)
    bs, bt = fit_bounds(rs, rt, ms, mt)
    es, et = np.abs(s.astype(np.float64) - rs), np.abs(t.astype(np.float64) - rt).max(-1)
    np.testing.assert_array_equal(v.astype(bool), rv)
    ok = rv if prev is not None else np.isfinite(rs) & np.isfinite(rt).all(-1)
    assert np.isfinite(s[ok]).all() and np.isfinite(t[ok]).all()
    if rv.any():                                # the figures, before anything is asserted about them
        rel = lambda e: (e[rv] / np.abs(rs[rv])).max()                                           # noqa: E731
        print(f"N={case['labels'].shape[1]} sym={sym}: scale err / |s| kernel {rel(es):.2e} mirror {rel(np.abs(ms - rs)):.2e}; "
              f"trans err kernel {et[rv].max():.2e} mirror {np.abs(mt - rt)[rv].max():.2e} at |t| <= {np.abs(rt[rv]).max():.2f}")
    # Measured on the CPU over every case of this file, valid parts: the oracle in place of the kernel is within 5.7e-8 |s| and
    # 1.2e-7 (|t| <= 3.1) of float64; the fp32 mirror within 2.1e-7 |s| and 4.0e-7.  The kernel gets 2 x the mirror's own error
    # on the same inputs, per part, and never less than 4 fp32 ulps of the output (4.8e-7 relative)
    assert (es[ok] <= bs[ok]).all(), (es[ok], bs[ok])
    assert (et[ok] <= bt[ok]).all(), (et[ok], bt[ok])
    if prev is not None:                        # invalid: the previous scale / translation, untouched
        np.testing.assert_array_equal(s[~rv], prev[0][~rv])
        np.testing.assert_array_equal(t[~rv], prev[1].reshape(t.shape)[~rv])
    return rv


# ================================================================================================== segmentation read-out
def seg_logits(B, S, N, seed):
    """(B,S,N) fp32 logits; the point index modulo 8 selects the regime: 0 order 1, 1 every class at +-1e4 (ties at the
    maximum wherever two classes draw +1e4), 2 every class at +-80, 3 normal x 1e4, 4 one class at -inf (S >= 2), 5 two classes tied
    at the maximum (positions vary with the point), 6 all classes equal, 7 normal x 80."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, S, N)).astype(np.float32)
    k = np.arange(N) % 8
    x = np.where(k == 1, rng.choice(np.array([-1e4, 1e4], np.float32), (B, S, N)), x)
    x = np.where(k == 2, rng.choice(np.array([-80.0, 80.0], np.float32), (B, S, N)), x)
    x = np.where(k == 3, x * np.float32(1e4), x)
    x = np.where(k == 7, x * np.float32(80), x)
    x = np.where(k == 6, x[:, :1], x)
    cls = np.arange(S)[None, :, None]
    if S >= 2:
        x = np.where((k == 4) & (cls == rng.integers(0, S, (B, 1, N))), np.float32(-np.inf), x)
        c1 = rng.integers(0, S, (B, 1, N))
        c2 = (c1 + rng.integers(1, S, (B, 1, N))) % S
        top = x.max(1, keepdims=True) + np.float32(1.0)
        x = np.where((k == 5) & ((cls == c1) | (cls == c2)), top, x)
    return np.ascontiguousarray(x, np.float32)


def softmax_argmax_ref(x):
    """float64 softmax over axis 1 and the FIRST index of the largest logit."""
    x = x.astype(np.float64)
    with np.errstate(all="ignore"):
        e = np.exp(x - x.max(1, keepdims=True))
        return e / e.sum(1, keepdims=True), np.argmax(x, 1).astype(np.int32)


# ============================================================================================================ GPU tests
def _dev(a, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _abi_procrustes(src, tgt):
    """captra_procrustes_rot3 through the C ABI on device tensors (nb,n,3) -> (nb,3,3), NaN-prefilled."""
    import torch
    from captra_amd import _lib as L
    nb, n = src.shape[0], src.shape[1]
    rot = torch.full((nb, 3, 3), float("nan"), dtype=torch.float32, device=src.device)
    with torch.cuda.device(src.device):
        err = L.lib().captra_procrustes_rot3(nb, n, L.ptr(src), L.ptr(tgt), L.ptr(rot), L.stream_ptr())
    assert err == 0, err
    return rot


@pytest.mark.gpu
@pytest.mark.parametrize("n", SWEEP_N)
def test_procrustes_rot3_conditioning_sweep(device, n):
    """The 30 sweep cases at n points, each solved alone (nb = 1, procrustes.rotate_pts_batch) and held to every assertion;
    then in batches of nb = 7 (rotate_pts_batch) and, for n <= 4096, nb = 5000 (C ABI; 5000 x 100000 points would be 12 GB):
    one workgroup reduces one problem in a fixed order, so a problem's rotation must not depend on where in which batch it
    sits -- bit for bit."""
    import torch
    from captra_amd.pose_utils.procrustes import rotate_pts_batch
    cases = sweep_cases(n)
    got = check_sweep(n, lambda s, t: rotate_pts_batch(_dev(s[None], device), _dev(t[None], device))[0].cpu().numpy())
    alone = np.stack([got[c[0]] for c in cases])
    src, tgt = _dev(np.stack([c[3] for c in cases]), device), _dev(np.stack([c[4] for c in cases]), device)
    for start in range(0, len(cases), 7):
        idx = torch.arange(start, start + 7, device=device) % len(cases)
        r7 = rotate_pts_batch(src[idx], tgt[idx]).cpu().numpy()
        np.testing.assert_array_equal(r7, alone[idx.cpu().numpy()])
    if n <= 4096:
        idx = (torch.arange(5000, device=device) * 7 + 3) % len(cases)
        r5k = _abi_procrustes(src[idx].contiguous(), tgt[idx].contiguous()).cpu().numpy()
        np.testing.assert_array_equal(r5k, alone[idx.cpu().numpy()])


@pytest.mark.gpu
def test_procrustes_rot3_degenerate(device):
    """Rank <= 1 cross-covariances (collinear, identical and all-zero points, n = 0, 1, 2), n = 3 and the isotropic reflected
    cloud: a finite proper rotation that attains the optimum, through the C ABI (the only way to n = 0), through
    rotate_pts_batch, and all in one batch beside well-conditioned problems."""
    from captra_amd.pose_utils.procrustes import rotate_pts_batch
    cases = degenerate_cases()
    for name, src, tgt in cases:
        r = _abi_procrustes(_dev(src[None], device), _dev(tgt[None], device))[0].cpu().numpy()
        check_rotation(r, src, tgt, name, compare_matrix=False)
        if len(src):
            r2 = rotate_pts_batch(_dev(src[None], device), _dev(tgt[None], device))[0].cpu().numpy()
            np.testing.assert_array_equal(r2, r)
    # one launch, nb = 7, every problem padded with zero points (they add nothing to M) to a common n = 300
    batch = ("collinear_exact", "all_identical", "n=3", "all_zero", "isotropic_reflected", "n=1", "collinear_rounded")
    pick = [c for name in batch for c in cases if c[0] == name]
    assert len(pick) == 7
    pad = lambda a: np.concatenate([a, np.zeros((300 - len(a), 3), np.float32)])         # noqa: E731
    rb = rotate_pts_batch(_dev(np.stack([pad(c[1]) for c in pick]), device), _dev(np.stack([pad(c[2]) for c in pick]), device))
    for (name, src, tgt), r in zip(pick, rb.cpu().numpy()):
        check_rotation(r, src, tgt, name + "/batched", compare_matrix=False)


def _fit_cn(case, device, sym, given_scale=None):
    from captra_amd.pose_utils.pose_fit import part_fit_st_cn
    gs = None if given_scale is None else _dev(given_scale, device)
    s, t, v = part_fit_st_cn(_dev(case["labels"], device), _dev(case["src"], device), _dev(case["tgt"], device),
                             _dev(case["rot"], device), sym, given_scale=gs, tgt_per_part=case["tgt"].ndim == 4)
    return s.cpu().numpy(), t[..., 0].cpu().numpy(), v.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("sym", [False, True])
@pytest.mark.parametrize("N", FIT_N)
def test_part_fit_st_vs_float64(device, N, sym):
    """captra_part_fit_st through part_fit_st_cn: one target per trajectory and one per part, each clean and with NaN / Inf in
    every kind of non-member point (none may reach an output), with the scale fitted and given, and with a rotation that is
    not orthonormal (the denominator sum |R'(s - s_bar)|^2 honours it)."""
    rng = np.random.default_rng(N)
    for per_part in (False, True):
        for poison in (False, True):
            case = fit_case(N, seed=10 * N + 2 * per_part + poison, per_part=per_part, poison=poison)
            valid = check_fit(_fit_cn(case, device, sym), case, sym)
            if N >= 7:
                assert not valid[1, 0] and not valid[1, 1] and valid[1, 2] and not valid[2, 1]   # sizes 0, 3, 4, 0
                assert valid[2, 0] == (N > 3)
            gs = rng.uniform(0.05, 0.2, (3, 3)).astype(np.float32)
            check_fit(_fit_cn(case, device, sym, gs), case, sym, given_scale=gs)
    case = fit_case(N, seed=10 * N + 5, skew_rot=True)
    check_fit(_fit_cn(case, device, sym), case, sym)


@pytest.mark.gpu
@pytest.mark.parametrize("sym", [False, True])
@pytest.mark.parametrize("N", FIT_N)
def test_part_fit_st_no_ransac_vs_float64(device, N, sym):
    """The reference-signature entry point (labels int64, (B,P,N,3) clouds, one target per part), scale fitted and given."""
    import torch
    from captra_amd.pose_utils.pose_fit import part_fit_st_no_ransac
    rng = np.random.default_rng(N + 1)
    for poison in (False, True):
        case = fit_case(N, seed=10 * N + 6 + poison, per_part=True, poison=poison)
        for gs in (None, rng.uniform(0.05, 0.2, (3, 3)).astype(np.float32)):
            model, valid = part_fit_st_no_ransac(
                _dev(case["labels"].astype(np.int64), device), _dev(case["src"].transpose(0, 1, 3, 2), device),
                _dev(case["tgt"].transpose(0, 1, 3, 2), device), _dev(case["rot"], device), {"num_parts": 3, "sym": sym},
                given_scale=None if gs is None else _dev(gs, device))
            assert torch.equal(model["rotation"], _dev(case["rot"], device))
            check_fit((model["scale"].cpu().numpy(), model["translation"][..., 0].cpu().numpy(), valid.cpu().numpy()), case, sym,
                      given_scale=gs)


@pytest.mark.gpu
@pytest.mark.parametrize("sym", [False, True])
@pytest.mark.parametrize("N", FIT_N)
def test_part_fit_st_track_vs_float64(device, N, sym):
    """captra_part_fit_st_track: the target is pts + mean (one fp32 addition, the reference's `points + points_mean`), and a
    part whose fit is invalid -- empty, three points, or a NaN in a MEMBER point -- keeps prev_scale / prev_trans bit for bit."""
    from captra_amd.pose_utils.pose_fit import part_fit_st_track
    rng = np.random.default_rng(N + 2)
    for poison in (False, True):
        case = fit_case(N, seed=10 * N + 8 + poison, poison=poison)
        with np.errstate(invalid="ignore"):
            mean = case["tgt"][:, :, : max(N // 2, 1)].mean(-1)
        mean = np.where(np.isfinite(mean), mean, np.float32(1.5)).astype(np.float32)           # (B,3): ~ the offset
        pts = (case["tgt"] - mean[:, :, None]).astype(np.float32)
        if N >= 257:        # a NaN in one member point of (trajectory 0, part 1): that fit is invalid, its neighbours are not
            n_bad = int(np.nonzero(case["labels"][0] == 1)[0][0])
            case["src"][0, 1, 1, n_bad] = np.nan
        prev_s = rng.uniform(0.5, 1.5, (3, 3)).astype(np.float32)
        prev_t = rng.standard_normal((3, 3, 3, 1)).astype(np.float32)
        s, t, v = part_fit_st_track(_dev(case["labels"], device), _dev(case["src"], device), _dev(pts, device),
                                    _dev(mean[..., None], device), _dev(case["rot"], device), _dev(prev_s, device),
                                    _dev(prev_t, device), sym)
        tcase = dict(case, tgt=pts)
        valid = check_fit((s.cpu().numpy(), t[..., 0].cpu().numpy(), v.cpu().numpy()), tcase, sym, tgt_mean=mean, prev=(prev_s, prev_t))
        if N >= 257:
            assert not valid[0, 1] and valid[0, 0] and valid[0, 2]


@pytest.mark.gpu
@pytest.mark.parametrize("N", [7, 256, 4096])
def test_part_fit_st_nan_member_is_invalid(device, N):
    """A NaN (or Inf) in a MEMBER point of src or of tgt: valid = 0 for that part and only for it."""
    for sym in (False, True):
        for where, bad in (("src", np.nan), ("tgt", np.nan), ("src", np.inf), ("tgt", -np.inf)):
            case = fit_case(N, seed=N + 3, per_part=True)
            case[where][2, 0, 1, N // 2] = bad                   # trajectory 2: every point is a member of part 0
            case[where][1, 2, 0, int(np.nonzero(case["labels"][1] == 2)[0][0])] = bad      # the four-point part
            s, t, v = _fit_cn(case, device, sym)
            _, _, rv = part_fit_ref(case["labels"], case["src"], case["tgt"], case["rot"], sym)
            np.testing.assert_array_equal(v, rv)
            assert not v[2, 0] and not v[1, 2]
            clean = fit_case(N, seed=N + 3, per_part=True)
            s0, t0, v0 = _fit_cn(clean, device, sym)
            keep = np.ones((3, 3), bool)
            keep[2, 0] = keep[1, 2] = False
            np.testing.assert_array_equal(s[keep], s0[keep])     # the other parts: the same launch geometry, the same bits
            np.testing.assert_array_equal(t[keep], t0[keep])
            np.testing.assert_array_equal(v[keep], v0[keep])


@pytest.mark.gpu
@pytest.mark.parametrize("N", [7, 257, 4096])
def test_part_fit_st_sym_zero_cross_covariance(device, N):
    """sym with a zero 2x2 cross-covariance: the member points share the same (x, z) -- short-mantissa values, so that every
    partial sum and the centroid are exact in fp32 and the centred x, z are exactly 0 -- hence h == 0 and the in-plane rotation
    is the identity: the fit equals the sym = False one bit for bit, and the float64 reference."""
    case = fit_case(N, seed=N + 4)
    case["src"][:, :, 0, :] = np.float32(0.25)
    case["src"][:, :, 2, :] = np.float32(-0.375)
    got = _fit_cn(case, device, True)
    check_fit(got, case, True)
    plain = _fit_cn(case, device, False)
    for a, b in zip(got, plain):
        np.testing.assert_array_equal(a, b)


def _abi_seg(logits, want_seg, want_labels, S=None):
    """captra_seg_softmax_argmax through the C ABI with sentinel-filled outputs -> (err, seg, labels)."""
    import torch
    from captra_amd import _lib as L
    B, s_, N = logits.shape
    seg = torch.full((B, s_, N), -7.0, dtype=torch.float32, device=logits.device)
    labels = torch.full((B, N), -7, dtype=torch.int32, device=logits.device)
    with torch.cuda.device(logits.device):
        err = L.lib().captra_seg_softmax_argmax(B, s_ if S is None else S, N, L.ptr(logits), L.ptr(seg) if want_seg else None,
                                                L.ptr(labels) if want_labels else None, L.stream_ptr())
    torch.cuda.synchronize(logits.device)
    return err, seg.cpu().numpy(), labels.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 255, 256, 257, 4096, 5000])
@pytest.mark.parametrize("S", range(1, 9))
def test_seg_softmax_argmax_vs_float64(device, S, N):
    """Probabilities within the atol = 1e-6 of test_seg_readout_and_track_fit_one_launch_forms of the float64 softmax (fp32
    expf and one division: a few 6e-8 ulps of values <= 1), labels exactly the first index of the maximum; logits at +-1e4 and
    +-80 (a wrong max-subtraction overflows there), a class at -inf, ties; then each output alone, the other pointer NULL."""
    from captra_amd import fused
    x = seg_logits(2, S, N, seed=100 * S + N)
    ref_p, ref_l = softmax_argmax_ref(x)
    assert np.isfinite(ref_p).all()
    xd = _dev(x, device)
    seg, lab = fused.seg_softmax_argmax(xd)
    np.testing.assert_allclose(seg.cpu().numpy(), ref_p, atol=1e-6, rtol=0)
    np.testing.assert_array_equal(lab.cpu().numpy(), ref_l)
    err, seg1, lab1 = _abi_seg(xd, True, False)
    assert err == 0 and (lab1 == -7).all()
    np.testing.assert_array_equal(seg1, seg.cpu().numpy())
    err, seg2, lab2 = _abi_seg(xd, False, True)
    assert err == 0 and (seg2 == -7).all()
    np.testing.assert_array_equal(lab2, ref_l)


@pytest.mark.gpu
def test_seg_softmax_argmax_refuses_nine_classes(device):
    """S = 9 is beyond the kernel's register array: the ABI returns non-zero and writes nothing."""
    x = _dev(seg_logits(2, 9, 300, seed=9), device)
    err, seg, lab = _abi_seg(x, True, True)
    assert err != 0
    assert (seg == -7).all() and (lab == -7).all()
    err, seg, lab = _abi_seg(x[:, :8].contiguous(), True, True, S=0)
    assert err != 0 and (seg == -7).all() and (lab == -7).all()


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 2, 5, 8])
def test_seg_softmax_argmax_nan_logit(device, S):
    """What the kernel does with a NaN logit, pinned (the kernel is not changed for it): the NaN never wins the strict `>` of
    the arg max unless it sits in class 0, where the running maximum starts -- so the label is the first index of the largest
    non-NaN logit, or 0 when class 0 is NaN (torch.argmax would return the NaN's index); exp(NaN - m) makes the sum NaN, so all
    S probabilities of that point are NaN.  The points beside it are not touched."""
    N = 515
    x = seg_logits(2, S, N, seed=S)
    x[:, :, 4::8] = np.random.default_rng(S).standard_normal((2, S, len(range(4, N, 8)))).astype(np.float32)   # no -inf here
    clean_p, clean_l = softmax_argmax_ref(x)
    pts = np.arange(3, N, 5)
    cls = pts % S
    x[:, cls, pts] = np.nan
    err, seg, lab = _abi_seg(_dev(x, device), True, True)
    assert err == 0
    hit = np.zeros(N, bool)
    hit[pts] = True
    np.testing.assert_allclose(seg[:, :, ~hit], clean_p[:, :, ~hit], atol=1e-6, rtol=0)
    np.testing.assert_array_equal(lab[:, ~hit], clean_l[:, ~hit])
    assert np.isnan(seg[:, :, hit]).all()
    masked = np.where(np.isnan(x), -np.inf, x.astype(np.float64))
    want = np.where(np.isnan(x[:, 0]), 0, np.argmax(masked, 1)).astype(np.int32)
    np.testing.assert_array_equal(lab[:, hit], want[:, hit])
