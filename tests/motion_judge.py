"""The rule of captra_pose_extrapolate (include/captra_hip.h) in numpy float64 on the fp32 inputs as stored, every output rounded to
fp32 once -- the judge of tests/test_motion_gpu.py -- in two formulations of the extrapolating rotation Q: Rodrigues' formula as the
header states it (`form="rodrigues"`, THE judge) and the half-angle quaternion (`form="quaternion"`, other operations in another
order), and the batches of cases the kernel is held to."""
import numpy as np

RAD2DEG = 180.0 / np.pi


def rodrigues(axis, ang):
    """I + sin(ang) K + (1 - cos(ang)) K^2 for the unit vector `axis`, float64."""
    K = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    return np.eye(3) + np.sin(ang) * K + (1.0 - np.cos(ang)) * (K @ K)


def _quat_matrix(axis, ang):
    h = 0.5 * ang
    w = np.cos(h)
    x, y, z = np.sin(h) * axis
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def step_of(rot0, rot1, sym, form="rodrigues"):
    """(v, c) of the step rot0 -> rot1 (float64 3x3 each)."""
    if sym:
        a0, a1 = rot0[:, 1], rot1[:, 1]
        if form == "rodrigues":
            v = np.array([a0[1] * a1[2] - a0[2] * a1[1], a0[2] * a1[0] - a0[0] * a1[2], a0[0] * a1[1] - a0[1] * a1[0]])
            c = (a0[0] * a1[0] + a0[1] * a1[1]) + a0[2] * a1[2]
        else:
            v, c = np.cross(a0, a1), a0 @ a1
        return v, c
    if form == "rodrigues":
        D = np.array([[(rot1[i, 0] * rot0[j, 0] + rot1[i, 1] * rot0[j, 1]) + rot1[i, 2] * rot0[j, 2] for j in range(3)] for i in range(3)])
        c = 0.5 * (((D[0, 0] + D[1, 1]) + D[2, 2]) - 1.0)
    else:
        D = np.einsum("ik,jk->ij", rot1, rot0)
        c = (np.trace(D) - 1.0) / 2.0
    v = 0.5 * np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return v, c


def judge_one(rot0, trans0, rot1, trans1, measured0, verdict, sym, gain, max_angle, max_shift, form="rodrigues"):
    """One (b, p): fp32 arrays (3,3), (3,), (3,3), (3,) as stored, two ints, the launch's settings (gain, max_angle, max_shift: the
    fp32 values the kernel receives) -> dict(rot_next, trans_next fp32; measured1, used int; angle, shift fp32; Q float64 or None)."""
    gain, max_angle, max_shift = float(np.float32(gain)), float(np.float32(max_angle)), float(np.float32(max_shift))
    R0, R1 = rot0.astype(np.float64), rot1.astype(np.float64)
    t0, t1 = trans0.astype(np.float64), trans1.astype(np.float64)
    finite = bool(np.isfinite(R0).all() and np.isfinite(R1).all() and np.isfinite(t0).all() and np.isfinite(t1).all())
    out = dict(rot_next=rot1.astype(np.float32).copy(), trans_next=trans1.astype(np.float32).copy(), Q=None,
               measured1=int(finite and verdict in (0, 3)), used=0, angle=np.float32(0.0), shift=np.float32(0.0),
               angle64=0.0, shift64=0.0)
    if not finite:
        return out
    d = t1 - t0
    shift = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    v, c = step_of(R0, R1, sym, form)
    vn = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    theta = np.arctan2(vn, c)
    angle = theta * RAD2DEG
    out.update(angle=np.float32(angle), shift=np.float32(shift), angle64=float(angle), shift64=float(shift))
    if not (measured0 != 0 and verdict == 0 and angle <= max_angle and shift <= max_shift):
        return out
    out["used"] = 1
    out["trans_next"] = (t1 + gain * d).astype(np.float32)
    if vn == 0.0:
        return out
    Q = (rodrigues if form == "rodrigues" else _quat_matrix)(v / vn, gain * theta)
    out["Q"] = Q
    out["rot_next"] = (Q @ R1).astype(np.float32)
    return out


def judge_batch(case, form="rodrigues"):
    """`judge_one` over a batch of `make_batch` -> dict of (B,P,...) arrays."""
    B, P = case["measured0"].shape
    verdict = case["verdict"] if case["verdict"] is not None else np.zeros((B, P), np.int32)
    res = [[judge_one(case["rot0"][b, p], case["trans0"][b, p], case["rot1"][b, p], case["trans1"][b, p], int(case["measured0"][b, p]),
                      int(verdict[b, p]), case["sym"], case["gain"], case["max_angle"], case["max_shift"], form) for p in range(P)]
           for b in range(B)]
    stack = lambda k, dt: np.array([[r[k] for r in row] for row in res], dtype=dt)      # noqa: E731
    return dict(rot_next=stack("rot_next", np.float32), trans_next=stack("trans_next", np.float32), measured1=stack("measured1", np.int32),
                used=stack("used", np.int32), angle=stack("angle", np.float32), shift=stack("shift", np.float32),
                angle64=stack("angle64", np.float64), shift64=stack("shift64", np.float64))


# ---- the cases -----------------------------------------------------------------------------------------------------------------
MAX_SHIFT = 0.03125          # exactly representable: the case `shift_edge` steps by exactly this much and must be used
NONFINITE = [(t, name) for t in ("rot0", "trans0", "rot1", "trans1") for name in ("nan", "inf", "ninf")]
KINDS = (["equal", "theta_1e-7", "theta_1e-5", "theta_1e-3", "theta_45", "theta_89.9", "theta_120", "theta_180", "shift_edge", "shift_over",
          "unmeasured", "verdict_0", "verdict_1", "verdict_2", "verdict_3"] + [f"{name}_{t}" for t, name in NONFINITE])
_THETA = {"theta_1e-7": 1e-7, "theta_1e-5": 1e-5, "theta_1e-3": 1e-3, "theta_45": np.deg2rad(45.0), "theta_89.9": np.deg2rad(89.9),
          "theta_120": np.deg2rad(120.0), "theta_180": np.pi}


def random_rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    return _quat_matrix(q[1:] / np.linalg.norm(q[1:]), 2.0 * np.arctan2(np.linalg.norm(q[1:]), q[0]))


def kind_of(q, k):
    """The kind of thread q in launch k: with B P = 1 the 4 * len(KINDS) launches meet every kind with every k mod 4."""
    return KINDS[(q + 7 * k) % len(KINDS)]


def make_batch(B, P, sym, gain, k, seed=0):
    """Launch k of a shape: every (b, p) another motion of kind `kind_of(b P + p, k)`; k mod 2 picks max_angle (90 / 30 degrees), k mod
    4 >= 2 hands the verdicts over as NULL.  fp32 / int32 arrays as the kernel reads them."""
    assert np.gcd(len(KINDS), 28) == 1
    rng = np.random.default_rng(1000 * seed + 10 * k + sym)
    case = dict(sym=int(sym), gain=float(gain), max_angle=(90.0, 30.0)[k % 2], max_shift=MAX_SHIFT, kinds=[],
                rot0=np.zeros((B, P, 3, 3), np.float32), trans0=np.zeros((B, P, 3), np.float32), rot1=np.zeros((B, P, 3, 3), np.float32),
                trans1=np.zeros((B, P, 3), np.float32), measured0=np.ones((B, P), np.int32), verdict=np.zeros((B, P), np.int32))
    for b in range(B):
        for p in range(P):
            kind = kind_of(b * P + p, k)
            case["kinds"].append(kind)
            R0 = random_rotation(rng).astype(np.float32)
            theta = _THETA.get(kind, rng.uniform(0.01, 0.4))
            axis = rng.normal(size=3)
            if sym:         # the axis angle of the step IS theta: rotate about an axis perpendicular to the object's y-axis
                axis = np.cross(R0[:, 1].astype(np.float64), axis)
            axis /= np.linalg.norm(axis)
            R1 = R0.copy() if kind == "equal" else (rodrigues(axis, theta) @ R0.astype(np.float64)).astype(np.float32)
            t0 = rng.uniform(-0.5, 0.5, size=3).astype(np.float32)
            step = rng.normal(size=3)
            step *= (0.05 if kind == "shift_over" else rng.uniform(0.002, 0.02)) / np.linalg.norm(step)
            t1 = (t0.astype(np.float64) + step).astype(np.float32)
            if kind == "shift_edge":
                t0, t1 = np.zeros(3, np.float32), np.array([MAX_SHIFT, 0.0, 0.0], np.float32)
            if kind == "unmeasured":
                case["measured0"][b, p] = 0
            if kind.startswith("verdict_"):
                case["verdict"][b, p] = int(kind[-1])
            arrays = dict(rot0=R0, trans0=t0, rot1=R1, trans1=t1)
            for t, name in NONFINITE:
                if kind == f"{name}_{t}":
                    arrays[t].reshape(-1)[int(rng.integers(arrays[t].size))] = dict(nan=np.nan, inf=np.inf, ninf=-np.inf)[name]
            for key, a in arrays.items():
                case[key][b, p] = a
    if k % 4 >= 2:
        case["verdict"] = None
    return case


def check_batch(case, ref):
    """The fixture's precondition: but for `shift_edge`'s shift, which EQUALS max_shift on exactly representable values, every angle
    and shift lies at least 1e-6 (relative) from its threshold -- a case on the knife edge is a broken fixture."""
    ma, ms = float(np.float32(case["max_angle"])), float(np.float32(case["max_shift"]))
    kinds = np.array(case["kinds"]).reshape(ref["angle64"].shape)
    assert (np.abs(ref["angle64"] - ma) >= 1e-6 * ma).all(), "an angle on the knife edge"
    off = kinds != "shift_edge"
    assert (np.abs(ref["shift64"][off] - ms) >= 1e-6 * ms).all(), "a shift on the knife edge"
    assert (ref["shift64"][~off] == ms).all() and (ref["shift"][~off] == np.float32(ms)).all()
