"""Judge for the geometry kernels: furthest point sampling, ball query, three_nn / knn and the 3-NN weights
(tests/test_z_geom_edges_gpu.py; proven by tests/test_geom_judge_cpu.py).  numpy and Python integers only.

Every index the network consumes comes from three decisions made in fp32:
  distance ((dx*dx + dy*dy) + dz*dz), every operation rounded separately; strict '<' against radius*radius computed in float;
  strict '>' for the sampler's arg max (lowest index among equal maxima); strict '<' for insertion (earlier index among equals).
On uniform or NOCS clouds a kernel that fuses, re-associates or evaluates the distance in double flips about one membership per cloud
or none, so parity runs on such clouds cannot tell.  This file holds
  * evaluators of ONE squared distance: `contract` and the deviations a kernel could plausibly carry (DEVIATIONS), each computed
    exactly -- rational arithmetic (fractions.Fraction) and one rounding to the fp32 grid per modelled operation;
  * plain references of the five operations, written from the reference's loops (sampling_gpu.cu:93-209, ball_query_gpu.cu:9-45,
    interpolate_gpu.cu:9-57 / 81-124, pointnet_utils.py:284-287), which take the distance evaluator and the comparisons as
    parameters and so run as themselves or as MUTANTS;
  * seeded cloud builders that put points ON the knife edge: a coordinate is walked in single-ulp steps until `contract` and a
    deviation fall on different sides of the decision (every kept position verified with the exact evaluators), plus ties,
    scaled, non-finite and thin clouds;
  * RUNS: the table of (op, route, cloud) rows shared by the CPU and the GPU test.
A mutant applies its deviation at the knife pairs of the cloud (`overridden`): that is where a real kernel carrying the deviation
must differ, and the CPU test asserts that every such mutant changes an output index -- a knife-edge cloud that does not bite is a
broken test.
"""
from __future__ import annotations

import functools
import hashlib
from fractions import Fraction

import numpy as np

F32 = np.float32
U = 2.0 ** -24
GAMMA8 = 8 * U / (1 - 8 * U)
FPS_START = F32(1e10)
EPS_W = F32(1e-8)

DISTANCE_DEVIATIONS = ("fused_a", "fused_b", "assoc_r", "expanded", "double_once")
DECISION_DEVIATIONS = ("le", "r2_double")
DEVIATIONS = DISTANCE_DEVIATIONS + DECISION_DEVIATIONS


# ---- exact arithmetic ----------------------------------------------------------------------------------------------------------------
def _fr(v) -> Fraction:
    return Fraction(float(v))            # a float32 widens to a double exactly, a double is a rational exactly


def _rn(x: Fraction) -> Fraction:
    """x rounded to the nearest float32 (ties to even, subnormals kept), as a rational."""
    if x == 0:
        return x
    a = abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()      # 2^(e-1) < a < 2^(e+1)
    if a < Fraction(2) ** e:
        e -= 1
    e = max(e, -126)
    q = Fraction(2) ** (e - 23)
    n = a / q
    fl = n.numerator // n.denominator
    rem = n - fl
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl & 1):
        fl += 1
    r = fl * q
    assert r < Fraction(2) ** 128, "overflow: the exact evaluators are for finite knife pairs"
    return r if x > 0 else -r


def _diffs(a, b):
    return [_rn(_fr(a[i]) - _fr(b[i])) for i in range(3)]


def _ex_contract(a, b):
    dx, dy, dz = _diffs(a, b)
    return _rn(_rn(_rn(dx * dx) + _rn(dy * dy)) + _rn(dz * dz))


def _ex_fused_a(a, b):                    # fma(dz,dz, fma(dy,dy, dx*dx))
    dx, dy, dz = _diffs(a, b)
    return _rn(dz * dz + _rn(dy * dy + _rn(dx * dx)))


def _ex_fused_b(a, b):                    # fma(dz,dz, fma(dx,dx, dy*dy))
    dx, dy, dz = _diffs(a, b)
    return _rn(dz * dz + _rn(dx * dx + _rn(dy * dy)))


def _ex_assoc_r(a, b):                    # dx*dx + (dy*dy + dz*dz)
    dx, dy, dz = _diffs(a, b)
    return _rn(_rn(dx * dx) + _rn(_rn(dy * dy) + _rn(dz * dz)))


def _ex_double_once(a, b):                # the whole sum exactly, rounded once
    dx, dy, dz = _diffs(a, b)
    return _rn(dx * dx + dy * dy + dz * dz)


def _ex_expanded(a, b):                   # (|a|^2 + |b|^2) - 2 a.b, every operation in fp32
    fa, fb = [_fr(v) for v in a], [_fr(v) for v in b]
    sq = lambda p, q: _rn(_rn(_rn(p[0] * q[0]) + _rn(p[1] * q[1])) + _rn(p[2] * q[2]))      # noqa: E731
    return _rn(_rn(sq(fa, fa) + sq(fb, fb)) - _rn(2 * sq(fa, fb)))


_EXACT = {"contract": _ex_contract, "fused_a": _ex_fused_a, "fused_b": _ex_fused_b, "assoc_r": _ex_assoc_r,
          "double_once": _ex_double_once, "expanded": _ex_expanded}


def exact(name: str, a, b) -> np.float32:
    """One squared distance between the float32 points a and b under evaluator `name`, computed exactly."""
    return F32(float(_EXACT[name](a, b)))


def contract(P, q) -> np.ndarray:
    """The contract expression in numpy float32 (every ufunc call is one correctly rounded operation): P (..., 3), q (3,)."""
    P, q = np.asarray(P, F32), np.asarray(q, F32)
    with np.errstate(all="ignore"):
        dx, dy, dz = P[..., 0] - q[0], P[..., 1] - q[1], P[..., 2] - q[2]
        return (dx * dx + dy * dy) + dz * dz


def _estimate(name: str, P, q) -> np.ndarray:
    """A FILTER for the knife search only, never a verdict: the deviation emulated with float64 products (exact) and float64 sums
    (a double rounding is possible); every position the search keeps is re-decided by `exact`."""
    P, q = np.asarray(P, F32), np.asarray(q, F32)
    f = lambda v: v.astype(F32).astype(np.float64)      # noqa: E731
    with np.errstate(all="ignore"):
        if name == "expanded":
            sq = lambda a, b: (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]    # noqa: E731
            return (sq(P, P) + sq(q, q)) - F32(2) * sq(P, q)
        d = (P - q).astype(np.float64)
        X, Y, Z = d[..., 0] ** 2, d[..., 1] ** 2, d[..., 2] ** 2
        if name == "fused_a":
            return f(Z + f(Y + f(X))).astype(F32)
        if name == "fused_b":
            return f(Z + f(X + f(Y))).astype(F32)
        if name == "assoc_r":
            return f(f(X) + f(f(Y) + f(Z))).astype(F32)
        if name == "double_once":
            return f(X + Y + Z).astype(F32)
    raise KeyError(name)


def r2_float(r: float) -> np.float32:
    """radius * radius as the launchers and the oracle compute it: both factors and the product in float."""
    return F32(F32(r) * F32(r))


def r2_double(r: float) -> np.float32:
    """The deviation: the square taken in double and rounded once."""
    return F32(np.float64(r) ** 2)


def lt(a, b):
    with np.errstate(invalid="ignore"):
        return a < b


def le(a, b):
    with np.errstate(invalid="ignore"):
        return a <= b


def overridden(name: str, pairs):
    """A distance evaluator that is `contract` except at the given (point, point) pairs, where it is deviation `name`, exactly."""
    table = [(np.asarray(a, F32), np.asarray(b, F32), exact(name, a, b)) for a, b in pairs]

    def d2(P, q):
        P, q = np.asarray(P, F32), np.asarray(q, F32)
        out = contract(P, q)
        for a, b, v in table:
            for x, y in ((a, b), (b, a)):
                if np.array_equal(y.view(np.uint32), q.view(np.uint32)):
                    out[(P.view(np.uint32) == x.view(np.uint32)).all(-1)] = v
        return out
    return d2


# ---- the plain references (one cloud each; *_batch below) ------------------------------------------------------------------------------
def fps(xyz, m: int, temp=None, d2=contract, later_wins: bool = False, tmin: str = "ternary", j0: int = 0, idx=None):
    """sampling_gpu.cu:93-209 with the oracle's tie rule: start at 0, temp[k] = min(d, temp[k]), arg max with strict '>' over
    ascending k from best = -1.  -> (idx (m,), temp (N,) after every pick but the last was applied).
    tmin: "ternary" = d < temp ? d : temp (the oracle, the reference's torch path: a NaN temp stays); "fminf" = the CUDA kernel's
    min(d, temp) (a NaN temp is replaced by d).  The two differ on a NaN temp only.  later_wins: the '>=' mutant.
    j0 > 0 with the earlier picks in `idx` and their running minima in `temp`: picks j0.. of a sampling resumed there."""
    xyz = np.asarray(xyz, F32)
    n = xyz.shape[0]
    temp = np.full(n, FPS_START, F32) if temp is None else np.array(temp, F32)
    idx = np.zeros(m, np.int32) if idx is None else np.array(idx, np.int32)
    old = int(idx[j0 - 1]) if j0 > 0 else 0
    for j in range(max(j0, 1), m):
        d = d2(xyz, xyz[old])
        temp = np.where(lt(d, temp), d, temp) if tmin == "ternary" else np.fmin(d, temp)
        v = np.where(np.isnan(temp), F32(-np.inf), temp)           # NaN > best is false: never taken
        mx = v.max()
        old = 0
        if mx > -1.0:
            hit = np.flatnonzero(v == mx)
            old = int(hit[-1] if later_wins else hit[0])
        idx[j] = old
    return idx, temp


def ball_query(r2, k: int, xyz, centres, d2=contract, cmp=lt):
    """ball_query_gpu.cu:9-45: the first k points with d2 < r2 in index order, the tail filled with the first hit, zeros if none."""
    xyz, centres = np.asarray(xyz, F32), np.asarray(centres, F32)
    out = np.zeros((centres.shape[0], k), np.int32)
    for c in range(centres.shape[0]):
        hits = np.flatnonzero(cmp(d2(xyz, centres[c]), r2))[:k]
        if hits.size:
            out[c] = hits[0]
            out[c, :hits.size] = hits
    return out


def knn(k: int, unknown, known, d2=contract, cmp=lt):
    """interpolate_gpu.cu:9-57: double best[k] = 1e40, for every known point in order the first slot j with d < best[j] takes it and
    the slots behind shift.  -> (dist2 (N,k) float32, idx (N,k)).  The loop over known points is the reference's; the unknown points
    (independent threads there) are the numpy axis."""
    unknown, known = np.asarray(unknown, F32), np.asarray(known, F32)
    n = unknown.shape[0]
    best = np.full((n, k), 1e40, np.float64)
    bi = np.zeros((n, k), np.int32)
    cols = np.arange(k)[None]
    # every distance up front (the expression is symmetric in its two points bit for bit), then the reference's loop
    D = np.stack([d2(known, u) for u in unknown]).astype(np.float64) if n else np.zeros((0, known.shape[0]))
    for i in range(known.shape[0]):
        d = D[:, i:i + 1]
        c = cmp(d, best)
        if not c.any():
            continue
        has, j = c.any(1)[:, None], c.argmax(1)[:, None]
        sb, si = np.roll(best, 1, 1), np.roll(bi, 1, 1)
        nb = np.where(cols < j, best, np.where(cols == j, d, sb))
        ni = np.where(cols < j, bi, np.where(cols == j, i, si))
        best, bi = np.where(has, nb, best), np.where(has, ni, bi).astype(np.int32)
    with np.errstate(over="ignore"):
        return best.astype(F32), bi


def three_nn(unknown, known, d2=contract, cmp=lt):
    """interpolate_gpu.cu:81-124: the three-slot case of the same insertion (if / else if / else if)."""
    return knn(3, unknown, known, d2, cmp)


def weights_f32(dist2):
    """pointnet_utils.py:284-287 on the SQUARED distances, the kernel's operations in numpy float32 (sqrt and divide are correctly
    rounded): r_j = 1 / (sqrt(d2_j) + 1e-8); norm = (r0 + r1) + r2; w_j = r_j / norm."""
    d = np.asarray(dist2, F32)
    with np.errstate(all="ignore"):
        r = F32(1) / (np.sqrt(d) + EPS_W)
        norm = (r[..., 0] + r[..., 1]) + r[..., 2]
        return r / norm[..., None]


def weights_f64(dist2):
    """The same function of the fp32 squared distances evaluated in float64 (the constant is the kernel's float 1e-8f)."""
    d = np.asarray(dist2, F32).astype(np.float64)
    with np.errstate(all="ignore"):
        r = 1.0 / (np.sqrt(d) + np.float64(EPS_W))
        return r / ((r[..., 0] + r[..., 1]) + r[..., 2])[..., None]


def fps_batch(xyz, m, temp=None, **kw):
    res = [fps(x, m, None if temp is None else temp[b], **kw) for b, x in enumerate(xyz)]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def ball_query_batch(r2, k, xyz, centres, **kw):
    return np.stack([ball_query(r2, k, x, c, **kw) for x, c in zip(xyz, centres)])


def knn_batch(k, unknown, known, **kw):
    res = [knn(k, u, kn, **kw) for u, kn in zip(unknown, known)]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


# ---- the knife search ------------------------------------------------------------------------------------------------------------------
def _walk(p, axis: int, steps: int):
    """p with coordinate `axis` moved by -steps..steps ulps: (2*steps+1, 3) float32."""
    out = np.repeat(np.asarray(p, F32)[None], 2 * steps + 1, 0)
    bits = out[:, axis].copy().view(np.int32)
    bits += np.arange(-steps, steps + 1, dtype=np.int32) * (1 if p[axis] > 0 else -1)
    out[:, axis] = bits.view(F32)
    return out


def _direction(rng):
    """A unit vector whose three components are of comparable size (a fused chain flips almost nothing when one dominates)."""
    v = rng.uniform(0.4, 0.75, 3) * rng.choice([-1.0, 1.0], 3)
    return v / np.linalg.norm(v)


def _candidates(rng, ref, dist, steps):
    p = (np.asarray(ref, np.float64) + dist * _direction(rng)).astype(F32)
    axis = int(np.argmin(np.abs(p.astype(np.float64) - np.asarray(ref, np.float64))))
    if p[axis] == 0:
        return None
    return _walk(p, axis, steps)


def knife_ball_points(dev: str, centre, r: float, seed: int, count: int, steps: int = 2000):
    """`count` points on the knife edge of the ball (centre, r) for deviation `dev`: `contract` and the deviation decide the
    membership differently.  distance deviations: contract < r2 xor deviation < r2; "le": contract == r2 exactly; "r2_double":
    contract lies between the two squares (in one, out of the other).  Every point is verified with the exact evaluators.
    -> [(point (3,) float32, inside under the contract)], alternating inside / outside where the deviation allows both."""
    rng = np.random.default_rng(seed)
    centre = np.asarray(centre, F32)
    r2 = r2_float(r)
    lo, hi = min(r2, r2_double(r)), max(r2, r2_double(r))
    out, want_inside = [], True
    for _ in range(4000):
        if len(out) >= count:
            break
        P = _candidates(rng, centre, float(F32(r)), steps)
        if P is None:
            continue
        dc = contract(P, centre)
        near = np.flatnonzero(np.abs(dc - r2) <= 4 * np.spacing(r2))    # only the steps next to the sphere can decide differently
        P, dc = P[near], dc[near]
        if dev == "le":
            sel = np.flatnonzero(dc == r2)
        elif dev == "r2_double":
            assert lo < hi, "choose a radius whose two squares differ"
            sel = np.flatnonzero((dc >= lo) & (dc < hi))
        else:
            dd = _estimate(dev, P, centre)
            sel = np.flatnonzero((dc < r2) != (dd < r2))
            both = sel[(dc[sel] < r2) == want_inside]
            sel = both if both.size else sel
        for i in rng.permutation(sel)[:8]:
            p = P[i]
            c = exact("contract", p, centre)
            assert c == dc[i]
            if dev in DISTANCE_DEVIATIONS and (c < r2) == (exact(dev, p, centre) < r2):
                continue                                           # the filter's double rounding: not a knife
            out.append((p.copy(), bool(c < r2)))
            want_inside = not want_inside
            break
    assert len(out) >= count, (dev, len(out))
    return out


def knife_pair(dev: str, ref, dist: float, kind: str, seed: int, steps: int = 2000):
    """Two points a, b at about `dist` from `ref` whose ORDER of distance the deviation changes (verified exactly):
    "swap": contract d(b) > d(a), deviation d(b) < d(a);  "eq_up" / "eq_dn": contract d(b) == d(a), deviation d(b) > / < d(a)."""
    rng = np.random.default_rng(seed)
    ref = np.asarray(ref, F32)
    for _ in range(4000):
        A = _candidates(rng, ref, dist, 0)
        B = _candidates(rng, ref, dist, steps)
        if A is None or B is None:
            continue
        a = A[0]
        ca, da = contract(a, ref), _estimate(dev, a, ref)
        cb = contract(B, ref)
        near = np.flatnonzero(np.abs(cb - ca) <= 4 * np.spacing(ca))     # only the steps next to equality can change the order
        B, cb = B[near], cb[near]
        db = _estimate(dev, B, ref)
        if kind == "swap":
            sel = np.flatnonzero((cb > ca) & (db < da))
        elif kind == "eq_up":
            sel = np.flatnonzero((cb == ca) & (db > da))
        else:
            sel = np.flatnonzero((cb == ca) & (db < da))
        for i in rng.permutation(sel)[:8]:
            b = B[i]
            xa, xb = exact(dev, a, ref), exact(dev, b, ref)
            assert exact("contract", b, ref) == cb[i] and exact("contract", a, ref) == ca
            if (kind == "eq_up" and xb > xa) or (kind != "eq_up" and xb < xa):
                return a.copy(), b.copy()
    raise AssertionError(("no knife pair", dev, kind))


# ---- clouds ----------------------------------------------------------------------------------------------------------------------------
KNIFE_R = 0.1
# two radii that straddle every knife point of KNIFE_R: the knives lie within 4 ulps of r2, these squares 21 ulps to either side
KNIFE_R_LO, KNIFE_R_HI = float(F32(KNIFE_R * (1 - 1e-6))), float(F32(KNIFE_R * (1 + 1e-6)))
LATTICE_R = 0.25
LATTICE_H = 2.0 ** -6
LATTICE_TIE_R = 9.0 / 64.0
SA_RADII, SA_KS = (0.05, 0.1, 0.2), (32, 64, 128)
NAN_POS = np.array([0x7FC00000], np.uint32).view(F32)[0]
NAN_NEG = np.array([0xFFC00000], np.uint32).view(F32)[0]
INF = F32(np.inf)


def _rng(*key):
    return np.random.default_rng(int.from_bytes(hashlib.sha256(repr(key).encode()).digest()[:8], "little"))


def _uniform(rng, n, half=0.5):
    return ((rng.random((n, 3)) - 0.5) * 2 * half).astype(F32)


def lattice_points(rng, n, side=64):
    """n points with coordinates multiples of 2^-6 (every difference, square and sum of squares below is exact in fp32)."""
    return (rng.integers(0, side, (n, 3)).astype(F32) - F32(side // 2)) * F32(LATTICE_H)


def on_sphere_lattice(centre):
    """The six lattice points at exactly LATTICE_R from a lattice centre: d2 == r2 bit for bit."""
    off = np.zeros((6, 3), F32)
    for a in range(3):
        off[2 * a, a], off[2 * a + 1, a] = LATTICE_R, -LATTICE_R
    return np.asarray(centre, F32) + off


@functools.lru_cache(maxsize=None)
def ball_knife_cloud(dev: str, n: int):
    """One cloud of n points in [-0.5, 0.5]^3 and 64 centres.  Centre 0 is the knife centre for (dev, KNIFE_R): its knife points sit
    at the lane / chunk / tile edges (indices 63, 64, 255, 256 and, where n allows, 8191, 8192) and at a few other places; the rest
    of the cloud keeps clear of its sphere, so the ball holds fewer than 64 points.  Centre 1 is a lattice point with its six
    exact-on-r2 lattice neighbours for LATTICE_R (indices 62, 65, 254, 257, 300, 301).  Point 0 of the cloud is centre 0 itself.
    -> dict(xyz, centres, positions, kth, kth_pos, pairs)."""
    rng = _rng("ball", dev, n)
    xyz = _uniform(rng, n)
    c0 = np.array([0.21, -0.17, 0.13], F32)
    c1 = np.array([-8, 6, -10], F32) * F32(LATTICE_H)
    # keep the random bulk off the knife sphere's shell (no accidental near-edge point): pushed out radially to 2 r
    d0 = np.sqrt(contract(xyz, c0).astype(np.float64))
    near = (d0 > 0.5 * KNIFE_R) & (d0 < 1.5 * KNIFE_R)
    xyz[near] = (c0 + (xyz[near] - c0).astype(np.float64) * (2 * KNIFE_R / d0[near])[:, None]).astype(F32)
    xyz[0] = c0                                                     # the sampler's first pick: the level-1 stream kernel's centre 0
    positions = [p for p in (63, 64, 255, 256, 8191, 8192) if p < n] + [7, n - 1]
    pts = knife_ball_points(dev, c0, KNIFE_R, seed=len(dev) * 1000 + n, count=len(positions))
    for p, (pt, _) in zip(positions, pts):
        xyz[p] = pt
    for p, pt in zip((62, 65, 254, 257, 300, 301), on_sphere_lattice(c1)):
        xyz[p] = pt
    certain = [3, 40, 100, 270, n - 3]                              # certainly inside centre 0's ball, before and after the knives
    for i, p in enumerate(certain):
        xyz[p] = c0 + F32(0.02) * np.array([1 + i, -1, 2], F32) / F32(4)
    centres = np.concatenate([c0[None], c1[None], xyz[rng.choice(n, 62, replace=False)]]).astype(F32)
    # the K that makes a knife point the K-th hit: the knife of the lowest index (no other knife shifts the ranks before it)
    hits = np.flatnonzero(contract(xyz, c0) < r2_float(KNIFE_R))
    assert hits.size < 64, hits.size
    kth_pos = min(positions)
    kth = int((hits < kth_pos).sum()) + 1
    assert (hits > kth_pos).any()
    return dict(xyz=xyz, centres=centres, positions=positions, kth=kth, kth_pos=kth_pos, pairs=[(xyz[p], c0) for p in positions])


@functools.lru_cache(maxsize=None)
def fps_knife_cloud(dev: str, n: int, kind: str, pick: int):
    """The bulk huddled within 0.01 of point 0 (never picked in the first rounds) and, far away, a pair a, b with index(a) < index(b)
    whose order of distance the deviation changes -- from point 0 (pick 1) or from the unambiguous first pick at (10, 0, 0) (pick 2:
    the running minimum against the first pick decides).  -> dict(xyz, pairs)."""
    rng = _rng("fps", dev, n, kind, pick)
    xyz = (rng.standard_normal((n, 3)) * 0.003).clip(-0.01, 0.01).astype(F32)
    ia, ib = sorted(int(v) for v in rng.choice(np.arange(1, n), 2, replace=False))
    if pick == 1:
        ref = xyz[0]
        a, b = knife_pair(dev, ref, 3.0, kind, seed=n + pick)
    else:
        far = int(rng.integers(1, n))
        while far in (ia, ib):
            far = int(rng.integers(1, n))
        xyz[far] = (10.0, 0.0, 0.0)
        ref = xyz[far]
        for s in range(50):
            a, b = knife_pair(dev, ref, 4.7, kind, seed=n + pick + 100 * s)
            # the pair's running minimum must be the distance to the first pick, not to point 0
            # ... and the first pick stays the far point (squared distance 100 from point 0)
            if all(1.2 * contract(p, ref) < contract(p, xyz[0]) < 90.0 for p in (a, b)):
                break
        else:
            raise AssertionError("no pair on the first pick's side")
    xyz[ia], xyz[ib] = a, b
    return dict(xyz=xyz, pairs=[(a, ref), (b, ref)], ia=ia, ib=ib, pick=pick)


FPS_KINDS = ("swap", "eq_up")


@functools.lru_cache(maxsize=None)
def fps_knife_batch(n: int):
    """All (deviation, kind, pick) clouds of n points as one batch.  -> dict(xyz (B,n,3), meta [dict per cloud])."""
    meta = [dict(dev=d, kind=k, **fps_knife_cloud(d, n, k, p)) for d in DISTANCE_DEVIATIONS for k in FPS_KINDS for p in (1, 2)]
    return dict(xyz=np.stack([m["xyz"] for m in meta]), meta=meta)


@functools.lru_cache(maxsize=None)
def tie_clouds(n: int):
    """(2, n, 3): a lattice cloud (hundreds of exactly equal distances, some points repeated) and a cloud in which every point
    appears exactly twice."""
    rng = _rng("ties", n)
    a = lattice_points(rng, n, side=16 if n <= 4096 else 32)
    half = _uniform(rng, (n + 1) // 2)
    b = rng.permutation(np.concatenate([half, half]))[:n] if n % 2 == 0 else np.concatenate([half, half])[:n]
    return np.stack([a, b.astype(F32)])


SCALES = (-20, 10, -60, -64, 40)


def scaled(xyz, e: int):
    return (np.asarray(xyz, F32) * F32(2.0 ** e)).astype(F32)


@functools.lru_cache(maxsize=None)
def nonfinite_clouds(n: int):
    """(10, n, 3) uniform clouds poisoned in place.  0: a NaN point; 1: a point with one NaN coordinate; 2: a +Inf point; 3: a -Inf
    point; 4: two equal Inf points (inf - inf); 5: point 0 NaN (the sampler's start); 6: all NaN; 7: one axis NaN throughout;
    8: sign-set NaNs; 9: a mix of all of them.  -> (xyz, names)."""
    rng = _rng("nonfinite", n)
    xyz = np.stack([_uniform(rng, n) for _ in range(10)])
    i, j, k = n // 3, n // 2, n - 2
    xyz[0, i] = NAN_POS
    xyz[1, j, 1] = NAN_POS
    xyz[2, k] = INF
    xyz[3, i] = -INF
    xyz[4, i] = INF; xyz[4, k] = INF
    xyz[5, 0] = NAN_POS
    xyz[6] = NAN_POS
    xyz[7, :, 2] = NAN_POS
    xyz[8, i] = NAN_NEG; xyz[8, j, 0] = NAN_NEG
    xyz[9, i] = NAN_POS; xyz[9, j, 2] = NAN_NEG; xyz[9, k] = (INF, -INF, 0.25); xyz[9, 5] = INF; xyz[9, 6] = INF
    names = ("nan_point", "nan_coordinate", "pinf_point", "ninf_point", "equal_inf_points", "start_point_nan", "all_nan",
             "one_axis_nan", "sign_set_nans", "mixed")
    return xyz, names


def nonfinite_centres(xyz, m: int, seed: int):
    """m centres per cloud: cloud points (the poisoned ones among them) plus a NaN, a +Inf and a far centre."""
    rng = _rng("nfc", seed, m)
    B, n, _ = xyz.shape
    pick = rng.choice(n, m, replace=False)
    pick[:6] = (n // 3, n // 2, n - 2, 0, 5, 6)
    c = xyz[:, pick].copy()
    c[:, 6] = NAN_POS
    c[:, 7] = INF
    c[:, 8] = 50.0
    c[:, 9, 0] = NAN_NEG
    return c


@functools.lru_cache(maxsize=None)
def thin_clouds():
    """(3, 4096, 3): 4096 collinear points with spacing h along x, y and z constant; the same with a jitter of 1e-3 h; the same offset to
    about (3, -3, 3).  With r = h (1 + 3e-5) a ball holds a point and its two neighbours, and the grid path gets about 4095 cells on one axis."""
    rng = _rng("thin")
    h = 2.44e-4
    t = (np.arange(4096) * h).astype(F32)
    base = np.stack([t, np.full(4096, 0.125, F32), np.full(4096, -0.25, F32)], -1).astype(F32)
    jit = base.copy()
    jit[:, 0] += (rng.uniform(-1e-3, 1e-3, 4096) * h).astype(F32)
    off = (base.astype(np.float64) + np.array([3.0, -3.0, 3.0])).astype(F32)
    return np.stack([base, jit, off]), F32(h * (1 + 3e-5))


@functools.lru_cache(maxsize=None)
def nn_knife_cloud(dev: str, k: int, s: int, cut: int = -1):
    """Unknown points far apart (10 units), each with a cluster of known points of its own: `j - 1` clearly nearer points, a knife
    pair at about 0.5 whose order the deviation changes, and k clearly farther points -- so the pair sits at the rank boundary j / j + 1;
    j runs over 1, k - 1, k (the last changes the MEMBERSHIP of the list) and all three kinds of pair.  The known cloud is padded
    with far points to s; cut >= 0 puts the first pair across known indices cut - 1 / cut (a tile edge).
    -> dict(unknown (n,3), known (s,3), pairs, rows: [(unknown index, j, kind, ia, ib)])."""
    rng = _rng("nn", dev, k, s, cut)
    bounds = sorted({1, max(k - 1, 1), k})
    rows, unknown, chunks, pairs = [], [], [], []
    for t, (j, kind) in enumerate([(j, kd) for j in bounds for kd in ("swap", "eq_dn")]):
        u = np.array([10.0 * (t + 1), -3.0 + t, 2.0], F32) + _uniform(rng, 1, 0.2)[0]
        a, b = knife_pair(dev, u, 0.5, kind, seed=k * 100 + t)
        near = (u + (_uniform(rng, j - 1, 1.0) * F32(0.2))).astype(F32)
        dirs = rng.standard_normal((k, 3))
        farp = (u + (dirs / np.linalg.norm(dirs, axis=1, keepdims=True) * rng.uniform(1.0, 1.5, (k, 1)))).astype(F32)
        unknown.append(u)
        chunks.append((near, a, b, farp))
        pairs += [(a, u), (b, u)]
        rows.append([t, j, kind])
    total = sum(len(c[0]) + 2 + len(c[3]) for c in chunks)
    assert total <= s, (total, s)
    known = (_uniform(rng, s, 2.0) + np.array([-40.0, 0, 0], F32)).astype(F32)           # padding: far from every unknown point
    free = list(rng.permutation(s))
    if cut >= 0:
        free = [p for p in free if p not in (cut - 1, cut)]
    for t, (near, a, b, farp) in enumerate(chunks):
        take = [int(free.pop()) for _ in range(len(near) + len(farp) + 2)]
        ia, ib = sorted(take[:2])
        if t == 0 and cut >= 0:
            free += [ia, ib]
            ia, ib = cut - 1, cut
        known[ia], known[ib] = a, b
        for p, v in zip(take[2:], np.concatenate([near, farp])):
            known[p] = v
        rows[t] += [ia, ib]
    # a few unknown points that are not special, one of them a known point itself (distance 0)
    extra = np.concatenate([_uniform(rng, 5, 2.0) + np.array([-40.0, 0, 0], F32), known[3:4]]).astype(F32)
    return dict(unknown=np.concatenate([np.stack(unknown), extra]).astype(F32), known=known, pairs=pairs, rows=[tuple(r) for r in rows])


@functools.lru_cache(maxsize=None)
def nn_plain_case(name: str, n: int, s: int):
    """(unknown (2,n,3), known (2,s,3)) for the tie / scale / non-finite / tiny-s families."""
    rng = _rng("nnplain", name, n, s)
    if name == "ties":
        unknown = np.stack([lattice_points(rng, n, 16), _uniform(rng, n)])
        half = _uniform(rng, (s + 1) // 2)
        known = np.stack([lattice_points(rng, s, 16), np.concatenate([half, half])[:s]])
        return unknown, known.astype(F32)
    unknown, known = np.stack([_uniform(rng, n), _uniform(rng, n)]), np.stack([_uniform(rng, s), _uniform(rng, s)])
    if name == "nonfinite":
        unknown[0, 1] = NAN_POS; unknown[0, 2, 1] = NAN_NEG; unknown[0, 3] = INF; unknown[0, 4] = -INF
        known[0, 0] = NAN_POS
        if s > 1:
            known[0, s // 2, 2] = NAN_NEG
        if s > 4:
            known[0, s - 1] = INF; known[0, 2] = INF; known[0, 3] = -INF
        unknown[0, 5] = known[0, s - 1]                             # inf - inf
        known[1] = NAN_POS                                          # no finite neighbour at all: idx 0, d2 +inf, weights NaN
        if s > 2:
            known[1, s - 2:] = unknown[1, :2]                       # ... but two: fewer than three finite neighbours
    return unknown, known


# ---- the table -------------------------------------------------------------------------------------------------------------------------
FPS_SIZES = (512, 4096, 8192, 16384, 20480)        # <1,8>, <4,16>, pruned, global-memory broadcast (pruned off), pruned with LDS slots
WEIGHT_SIZES = (1, 2, 3, 37, 4096, 4097, 5000)
KNN_KS = (1, 3, 16, 200)


def _runs():
    rows = []
    for n in FPS_SIZES:
        rows += [dict(op="fps", cloud=("knife", n), m=8), dict(op="fps", cloud=("ties", n), m=64),
                 dict(op="fps", cloud=("nonfinite", n), m=12)]
    for n in (512, 4096, 8192):
        rows += [dict(op="fps", cloud=("scaled", n, e), m=16) for e in (0,) + SCALES]
    for n in (512, 4096):
        rows.append(dict(op="fps", cloud=("nan_temp", n), m=12))
    for dev in DEVIATIONS:
        rows += [dict(op="ball", cloud=("knife", dev, n)) for n in (4096, 9000)]
    rows += [dict(op="ball", cloud=("knife", dev, 1500)) for dev in ("fused_b", "le", "r2_double")]    # the grid's range is 1024..4096
    rows += [dict(op="ball", cloud=(name, 4096)) for name in ("ties", "nonfinite", "thin")]
    rows += [dict(op="ball", cloud=("scaled", 4096, e)) for e in (0,) + SCALES]
    for dev in DISTANCE_DEVIATIONS:
        rows.append(dict(op="nn3", cloud=("knife", dev)))
        rows += [dict(op="knn", cloud=("knife", dev), k=k) for k in KNN_KS]
    for name in ("ties", "nonfinite"):
        rows.append(dict(op="nn3", cloud=(name,)))
        rows += [dict(op="knn", cloud=(name,), k=k) for k in KNN_KS]
    rows += [dict(op="nn3", cloud=("scaled", e)) for e in (0,) + SCALES]
    for s in WEIGHT_SIZES:
        rows += [dict(op="weights", cloud=("knife", s)), dict(op="weights", cloud=("nonfinite", s))]
    rows.append(dict(op="weights", cloud=("ties", 512)))
    return rows


RUNS = _runs()


def fps_inputs(cloud):
    """-> (xyz (B,n,3), incoming temp or None, meta)."""
    kind, n = cloud[0], cloud[1]
    if kind == "knife":
        kb = fps_knife_batch(n)
        return kb["xyz"], None, kb["meta"]
    if kind == "ties":
        return tie_clouds(n), None, None
    if kind == "nonfinite":
        return nonfinite_clouds(n)[0], None, None
    if kind == "scaled":
        base = np.stack([_uniform(_rng("fps_scaled", n, b), n) for b in range(2)])
        return scaled(base, cloud[2]), None, None
    if kind == "nan_temp":
        xyz = np.stack([_uniform(_rng("fps_nan_temp", n, b), n) for b in range(2)])
        temp = np.full((2, n), FPS_START, F32)
        temp[0, n // 3] = NAN_POS; temp[1, 7] = NAN_NEG; temp[1, n - 1] = NAN_POS
        return xyz, temp, None
    raise KeyError(cloud)


def ball_inputs(cloud):
    """-> (xyz (B,n,3), centres (B,m,3), [(radius, k)], meta)."""
    kind = cloud[0]
    if kind == "knife":
        dev, n = cloud[1], cloud[2]
        c = ball_knife_cloud(dev, n)
        queries = [(KNIFE_R, 64), (KNIFE_R, c["kth"]), (KNIFE_R_LO, 64), (KNIFE_R_HI, 64), (LATTICE_R, 256), (0.05, 32)]
        return c["xyz"][None], c["centres"][None], queries, c
    n = cloud[1]
    if kind == "ties":
        xyz = tie_clouds(n).copy()
        xyz[0] = lattice_points(_rng("ball_ties", n), n, 64)          # extent 1: balls of 9/64 hold about 48 points
        centres = xyz[:, ::n // 64][:, :64].copy()
        # r = 9/64: r2 = 81 / 4096 exactly, and 81 = 9^2 = 1 + 16 + 64 = 16 + 16 + 49 = 9 + 36 + 36: 102 lattice sites ON the sphere
        return xyz, centres, [(LATTICE_TIE_R, 256), (LATTICE_R, 64), (0.1, 32)], None
    if kind == "nonfinite":
        xyz = nonfinite_clouds(n)[0]
        return xyz, nonfinite_centres(xyz, 64, n), [(0.05, 16), (0.1, 32), (0.3, 64)], None
    if kind == "thin":
        xyz, r = thin_clouds()
        pick = np.unique(np.concatenate([np.arange(0, 4096, 9), [1, 2, 4093, 4094, 4095]]))
        return xyz, xyz[:, pick].copy(), [(float(r), 8)], None
    if kind == "scaled":
        e = cloud[2]
        rng = _rng("ball_scaled", n)
        xyz = np.stack([_uniform(rng, n), _uniform(rng, n)])
        centres = xyz[:, ::n // 64][:, :64].copy()
        return scaled(xyz, e), scaled(centres, e), [(float(F32(r) * F32(2.0 ** e)), k) for r, k in ((0.05, 32), (0.1, 64), (0.2, 128))], None
    raise KeyError(cloud)


def nn_inputs(op: str, cloud, k: int = 3):
    """-> (unknown (B,n,3), known (B,s,3), meta)."""
    kind = cloud[0]
    if op == "weights":
        s = cloud[1]
        if kind == "knife":
            if s < 37:
                u, kn = nn_plain_case("tiny", 300, s)
                return u, kn, None
            # one cloud per deviation; from 4097 points on, a pair straddles the 4096-point tile edge
            cs = [nn_knife_cloud(d, 3, s, cut=4096 if s > 4096 else -1) for d in DISTANCE_DEVIATIONS]
            return np.stack([c["unknown"] for c in cs]), np.stack([c["known"] for c in cs]), cs
        u, kn = nn_plain_case(kind, 300 if s < 4096 else 70, s)
        return u, kn, None
    if kind == "knife":
        c = nn_knife_cloud(cloud[1], k, max(700, 3 * (2 * k + 4) * 2 + 100))
        return c["unknown"][None], c["known"][None], [c]
    if kind == "scaled":
        u, kn = nn_plain_case("scale_base", 300, 257)
        return scaled(u, cloud[1]), scaled(kn, cloud[1]), None
    u, kn = nn_plain_case(kind, 300, 257)
    return u, kn, None


# ---- what the judge expects of a row (computed once, shared by every test that needs it; treat as read-only) ---------------------------
@functools.lru_cache(maxsize=None)
def _expected(key):
    row = dict(key)
    op, cloud = row["op"], row["cloud"]
    if op == "fps":
        xyz, temp, meta = fps_inputs(cloud)
        idx, tout = fps_batch(xyz, row["m"], temp)
        out = dict(xyz=xyz, temp_in=temp, meta=meta, idx=idx, temp=tout)
        if temp is not None:
            out["idx_fminf"], out["temp_fminf"] = fps_batch(xyz, row["m"], temp, tmin="fminf")
        return out
    if op == "ball":
        xyz, centres, queries, meta = ball_inputs(cloud)
        return dict(xyz=xyz, centres=centres, queries=queries, meta=meta,
                    lists=[ball_query_batch(r2_float(r), k, xyz, centres) for r, k in queries])
    unknown, known, meta = nn_inputs(op, cloud, row.get("k", 3))
    d2, idx = knn_batch(row.get("k", 3), unknown, known)
    out = dict(unknown=unknown, known=known, meta=meta, d2=d2, idx=idx)
    if op == "weights":
        out["w32"], out["w64"] = weights_f32(d2), weights_f64(d2)
    return out


def expected(row):
    return _expected(tuple(sorted(row.items())))


def row_id(row):
    return "-".join(str(v) for v in [row["op"], *row["cloud"], *[f"{k}{row[k]}" for k in ("m", "k") if k in row]])
