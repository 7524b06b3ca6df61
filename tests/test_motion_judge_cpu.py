"""The motion model's rule on the host: the two formulations of tests/motion_judge.py against each other and against the properties
the issue states, the parser of track_cfg/motion and the layout of its record."""
import numpy as np
import pytest

from tests import motion_judge as MJ

ULP1 = 2.0 ** -23            # one fp32 ulp of a value in [1, 2): a rotation entry is a sum of terms of order one


def _one(R0, R1, t0=(0, 0, 0), t1=(0.01, 0, 0), measured0=1, verdict=0, sym=0, gain=1.0, max_angle=90.0, max_shift=1.0, form="rodrigues"):
    return MJ.judge_one(np.asarray(R0, np.float32), np.asarray(t0, np.float32), np.asarray(R1, np.float32), np.asarray(t1, np.float32),
                        measured0, verdict, sym, gain, max_angle, max_shift, form)


def _pair(rng, theta, sym):
    R0 = MJ.random_rotation(rng).astype(np.float32)
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    return R0, (MJ.rodrigues(axis, theta) @ R0.astype(np.float64)).astype(np.float32)


def test_the_two_formulations_agree():
    """Rodrigues' formula and the half-angle quaternion, theta from 1e-8 rad to 90 degrees: both compute in double and round once, so
    they differ by at most one rounding flip -- the tolerance the kernel gets."""
    rng = np.random.default_rng(0)
    worst = 0.0
    for trial in range(1500):
        theta = 10 ** rng.uniform(-8, np.log10(np.pi / 2))
        for sym in (0, 1):
            R0, R1 = _pair(rng, theta, sym)
            if trial % 50 == 0:
                R1 = R0.copy()
            for gain in (1.0, 0.5):
                a, b = _one(R0, R1, sym=sym, gain=gain), _one(R0, R1, sym=sym, gain=gain, form="quaternion")
                assert a["used"] == b["used"] == 1
                worst = max(worst, float(np.abs(a["rot_next"].astype(np.float64) - b["rot_next"]).max()))
                assert abs(float(a["angle"]) - float(b["angle"])) <= np.spacing(np.float32(abs(a["angle"])))
                if trial % 50 == 0:
                    assert a["Q"] is None and a["rot_next"].tobytes() == R1.tobytes() and float(a["angle"]) == 0.0
    print("largest difference of a rotation entry between the formulations:", worst)
    assert worst <= ULP1


def test_constant_velocity_is_predicted():
    """rot1 = W rot0 with an exact W, sym = 0, gain 1: the prediction is W rot1 within 1e-6 (the inputs' own fp32 rounding gives a few
    1e-7), and Q is orthogonal at rounding level."""
    rng = np.random.default_rng(1)
    for theta in (1e-3, 0.03, 0.3, 1.2):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        W = MJ.rodrigues(axis, theta)
        R0 = MJ.random_rotation(rng)
        R1 = W @ R0
        for form in ("rodrigues", "quaternion"):
            r = _one(R0, R1, t0=(0.1, 0.2, 0.3), t1=(0.11, 0.18, 0.33), form=form)
            assert r["used"] == 1
            assert np.abs(r["rot_next"] - W @ R1).max() <= 1e-6
            assert np.abs(r["Q"].T @ r["Q"] - np.eye(3)).max() <= 1e-15
            t0, t1 = np.float32([0.1, 0.2, 0.3]).astype(np.float64), np.float32([0.11, 0.18, 0.33]).astype(np.float64)
            assert r["trans_next"].tobytes() == (t1 + (t1 - t0)).astype(np.float32).tobytes()
        half = _one(R0, R1, gain=0.5)
        assert np.abs(half["rot_next"] - MJ.rodrigues(axis, 0.5 * theta) @ R1).max() <= 1e-6


def test_symmetric_step_moves_the_axis_only():
    rng = np.random.default_rng(2)
    R0 = MJ.random_rotation(rng)
    spin = R0 @ MJ.rodrigues(np.array([0.0, 1.0, 0.0]), 0.7)          # a turn about the object's own y-axis: no motion of the axis
    r = _one(R0, spin, sym=1)
    assert r["used"] == 1 and float(r["angle"]) < 1e-4
    assert np.abs(r["rot_next"] - spin.astype(np.float32)).max() <= 1e-6
    axis = np.cross(R0[:, 1], rng.normal(size=3))
    axis /= np.linalg.norm(axis)
    W = MJ.rodrigues(axis, 0.2)
    r = _one(R0, W @ R0, sym=1)
    assert abs(float(r["angle"]) - np.rad2deg(0.2)) < 1e-4
    assert np.abs(r["rot_next"][:, 1] - (W @ W @ R0)[:, 1]).max() <= 1e-6


def test_gates_verdicts_and_pass_through():
    rng = np.random.default_rng(3)
    R0, R1 = _pair(rng, np.deg2rad(10.0), 0)
    t0, t1 = np.float32([0, 0, 0]), np.float32([MJ.MAX_SHIFT, 0, 0])

    def passes(r):
        return r["used"] == 0 and r["rot_next"].tobytes() == R1.tobytes() and r["trans_next"].tobytes() == t1.tobytes()

    r = _one(R0, R1, t0, t1, max_shift=MJ.MAX_SHIFT, max_angle=10.5)
    assert r["used"] == 1 and r["measured1"] == 1 and float(r["shift"]) == MJ.MAX_SHIFT          # a step EQUAL to max_shift is used
    assert passes(_one(R0, R1, t0, t1, max_shift=MJ.MAX_SHIFT * (1 - 1e-6)))
    assert passes(_one(R0, R1, t0, t1, max_angle=9.5))
    assert passes(_one(R0, R1, t0, t1, measured0=0)) and _one(R0, R1, t0, t1, measured0=0)["measured1"] == 1
    for verdict, used, measured1 in ((0, 1, 1), (1, 0, 0), (2, 0, 0), (3, 0, 1)):
        r = _one(R0, R1, t0, t1, verdict=verdict)
        assert (r["used"], r["measured1"]) == (used, measured1), verdict
        assert used or passes(r)
    for big in (120.0, 180.0):                      # c < 0: beyond any max_angle
        near, far = _pair(rng, np.deg2rad(big), 0)
        r = _one(near, far)
        assert r["used"] == 0 and abs(float(r["angle"]) - big) < 1e-3 and r["measured1"] == 1
    for which, name in MJ.NONFINITE:
        bad = dict(nan=np.nan, inf=np.inf, ninf=-np.inf)[name]
        arrays = dict(rot0=R0.copy(), trans0=t0.copy(), rot1=R1.copy(), trans1=t1.copy())
        arrays[which].reshape(-1)[1] = bad
        r = MJ.judge_one(arrays["rot0"], arrays["trans0"], arrays["rot1"], arrays["trans1"], 1, 0, 0, 1.0, 90.0, 1.0)
        assert (r["used"], r["measured1"], float(r["angle"]), float(r["shift"])) == (0, 0, 0.0, 0.0), (which, name)
        assert r["rot_next"].tobytes() == arrays["rot1"].tobytes() and r["trans_next"].tobytes() == arrays["trans1"].tobytes()


def test_case_batches_meet_every_kind_and_their_precondition():
    met = set()
    for k in range(4 * len(MJ.KINDS)):
        case = MJ.make_batch(1, 1, k % 2, 1.0, k)
        met.add((case["kinds"][0], k % 4))
    assert met == {(kind, m) for kind in MJ.KINDS for m in range(4)}
    for sym in (0, 1):
        for k in range(4):
            case = MJ.make_batch(3, 4, sym, 0.5, k)
            ref = MJ.judge_batch(case)
            MJ.check_batch(case, ref)
            assert (case["verdict"] is None) == (k >= 2)
            assert len({c.tobytes() for c in case["rot1"].reshape(-1, 9)}) == 12           # every (b, p) another motion


def _cfg(motion, radius=0.6):
    return {"track_cfg": {} if motion is None else {"motion": motion}, "data_radius": radius}


def test_motion_cfg():
    from captra_amd import track_options as O
    assert O.motion_cfg(_cfg(None)) is None
    assert O.motion_cfg(_cfg({"max_angle": 30, "max_shift": 0.2})) is None
    assert O.motion_cfg(_cfg({"predict": False, "max_angle": 30, "max_shift": 0.2})) is None
    got = O.motion_cfg(_cfg({"predict": True, "max_angle": 30, "max_shift": 0.2}))
    assert got == {"max_angle": 30.0, "max_shift": 0.2 * 0.6, "gain": 1.0}
    assert O.motion_cfg(_cfg({"predict": True, "max_angle": 90, "max_shift": 1, "gain": 0.25}, radius=2.0)) == {"max_angle": 90.0, "max_shift": 2.0, "gain": 0.25}
    for bad, path in (({"max_shift": 0.2}, "max_angle"), ({"max_angle": 30}, "max_shift"), ({"max_angle": 0, "max_shift": 0.2}, "max_angle"),
                      ({"max_angle": 90.5, "max_shift": 0.2}, "max_angle"), ({"max_angle": float("nan"), "max_shift": 0.2}, "max_angle"),
                      ({"max_angle": 30, "max_shift": 0}, "max_shift"), ({"max_angle": 30, "max_shift": -1}, "max_shift"),
                      ({"max_angle": 30, "max_shift": float("inf")}, "max_shift"), ({"max_angle": 30, "max_shift": 0.2, "gain": 0}, "gain"),
                      ({"max_angle": 30, "max_shift": 0.2, "gain": 1.5}, "gain")):
        with pytest.raises(ValueError, match=f"track_cfg/motion/{path}"):
            O.motion_cfg(_cfg({"predict": True, **bad}))
    assert O.STEP_RECORDS["motion"] == ("motion_", ("used", "angle", "shift", "rotation", "translation"))


def test_pose_dict_helpers():
    import torch
    from captra_amd import track_options as O
    pose = {"rotation": torch.eye(3).repeat(2, 3, 1, 1), "scale": torch.ones(2, 3), "translation": torch.zeros(2, 3, 3, 1)}
    assert O.start_pose(pose) is pose
    full = O.entering_pose(pose)
    assert set(full) == set(O.POSE_KEYS) | {"next_rotation", "next_translation", "measured"}
    assert full["measured"].dtype == torch.int32 and full["measured"].shape == (2, 3) and not full["measured"].any()
    assert full["next_rotation"] is pose["rotation"] and full["next_translation"] is pose["translation"]
    assert O.entering_pose(full) is full
    full["next_translation"] = full["translation"] + 1
    start = O.start_pose(full)
    assert set(start) == set(O.POSE_KEYS) and start["translation"] is full["next_translation"] and start["scale"] is pose["scale"]


def test_records_to_numpy_lays_out_a_motion_record():
    import torch
    from captra_amd import track_options as O
    B, P = 2, 3
    rec = lambda i: {"used": torch.full((B, P), i, dtype=torch.int32), "angle": torch.full((B, P), 1.5 * i), "shift": torch.zeros(B, P),   # noqa: E731
                     "rotation": torch.eye(3).repeat(B, P, 1, 1), "translation": torch.zeros(B, P, 3, 1)}
    pred = {"poses": [{"scale": torch.ones(B, P)}] * 3, "npcs_pred": [None] * 3, "motion": [None, rec(1), rec(2)]}
    out = O.records_to_numpy(pred)
    assert set(out) == {"motion"} and out["motion"][0] is None and len(out["motion"]) == 3
    for i in (1, 2):
        r = out["motion"][i]
        assert set(r) == {"used", "angle", "shift", "rotation", "translation"} and all(isinstance(v, np.ndarray) for v in r.values())
        assert r["used"].dtype == np.int32 and (r["used"] == i).all() and r["rotation"].shape == (B, P, 3, 3) and r["translation"].shape == (B, P, 3, 1)
    # what a commit does with the step's maps and pose: the record out of the maps, the committed pose back to three keys
    npcs = {"seg": torch.zeros(1), **{"motion_" + k: v for k, v in rec(1).items()}}
    pose = O.entering_pose({"rotation": torch.eye(3).repeat(B, P, 1, 1), "scale": torch.ones(B, P), "translation": torch.zeros(B, P, 3, 1)})
    records = {"motion": {}}
    got_npcs, got_pose = O.commit_with_records(lambda i, result: result, records)(1, (npcs, pose))
    assert set(got_npcs) == {"seg"} and set(got_pose) == set(O.POSE_KEYS) and set(records["motion"][1]) == set(rec(1))


def test_binding_has_the_header_s_argument_list():
    """Every argument of the declaration has its ctypes type, the stream included: an argument without one is converted as a C int,
    which truncates a pointer."""
    import ctypes as C
    import re
    from pathlib import Path
    from captra_amd import _lib
    text = (Path(__file__).resolve().parent.parent / "include" / "captra_hip.h").read_text()
    decl = re.search(r"int captra_pose_extrapolate\(([^;]*)\);", text).group(1)
    args = [a.strip() for a in decl.split(",")]
    types = _lib._SIGNATURES["captra_pose_extrapolate"]
    assert len(args) == len(types) == 19
    for a, t in zip(args, types):
        want = C.c_void_p if "*" in a or "captra_stream_t" in a else C.c_float if a.startswith("float") else C.c_int
        assert t is want, (a, t)
