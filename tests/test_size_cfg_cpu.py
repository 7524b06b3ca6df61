"""track_cfg/size as far as it is plumbing (captra_amd/track_options.py, captra_amd/eval.py, captra_amd/_lib.py), without a GPU:
the parser and its ranges, the records table's row, a track's initial size state, what a commit keeps, the pickle entry and the
eval CLI's table."""
import numpy as np
import pytest
import torch

from captra_amd import track_options as O


def _cfg(size):
    return {"track_cfg": {} if size is None else {"size": size}, "data_radius": 0.6}


def test_size_cfg():
    assert O.size_cfg(_cfg(None)) is None
    assert O.size_cfg(_cfg({"max_ratio": 1.5})) is None
    assert O.size_cfg(_cfg({"hold": False, "max_ratio": 1.5})) is None
    got = O.size_cfg(_cfg({"hold": True, "max_ratio": 1.5}))
    assert got == {"max_ratio": 1.5, "min_frames": 1, "max_frames": None, "reset_after": None, "init_frames": 0}
    got = O.size_cfg(_cfg({"hold": True, "max_ratio": 1.1, "min_frames": 3, "max_frames": 30, "reset_after": 5, "init_frames": 3}))
    assert got == {"max_ratio": float(np.float32(1.1)), "min_frames": 3, "max_frames": 30, "reset_after": 5, "init_frames": 3}
    assert O.size_cfg(_cfg({"hold": True, "max_ratio": 2, "max_frames": None, "reset_after": None}))["max_frames"] is None
    with pytest.raises(ValueError, match="track_cfg/size/max_ratio.*no default"):
        O.size_cfg(_cfg({"hold": True}))
    for bad, path in (({"max_ratio": 1.0}, "max_ratio"), ({"max_ratio": 0.5}, "max_ratio"), ({"max_ratio": float("nan")}, "max_ratio"),
                      ({"max_ratio": float("inf")}, "max_ratio"), ({"max_ratio": 1.0 + 1e-9}, "max_ratio"),      # (1 in fp32, the kernel's type)
                      ({"max_ratio": 2, "min_frames": 0}, "min_frames"), ({"max_ratio": 2, "min_frames": 1.5}, "min_frames"),
                      ({"max_ratio": 2, "max_frames": 0}, "max_frames"), ({"max_ratio": 2, "max_frames": -3}, "max_frames"),
                      ({"max_ratio": 2, "reset_after": 0}, "reset_after"), ({"max_ratio": 2, "init_frames": -1}, "init_frames"),
                      ({"max_ratio": 2, "min_frames": True}, "min_frames"), ({"max_ratio": 2, "max_frames": 2 ** 31}, "max_frames")):
        with pytest.raises(ValueError, match=f"track_cfg/size/{path}"):
            O.size_cfg(_cfg({"hold": True, **bad}))
    assert O.STEP_RECORDS["size"] == ("size_", ("held", "accepted", "free", "n"))
    assert O.SIZE_KEYS == ("size_mean", "size_n", "size_miss")


def test_command_line_flags_reach_the_parser():
    import argparse
    from captra_amd.parse_args import add_args
    ns = vars(add_args(argparse.ArgumentParser()).parse_args([]))
    assert not any(k.startswith("track_cfg/size") for k in ns)                # not given = not in the namespace
    ns = vars(add_args(argparse.ArgumentParser()).parse_args(["--track_cfg/size/hold", "True", "--track_cfg/size/max_ratio", "1.25",
                                                              "--track_cfg/size/init_frames", "2"]))
    size = {k.split("/")[-1]: v for k, v in ns.items() if k.startswith("track_cfg/size")}
    assert size == {"hold": True, "max_ratio": 1.25, "init_frames": 2}
    assert O.size_cfg(_cfg(size))["init_frames"] == 2


def _pose(B=2, P=3):
    return {"rotation": torch.eye(3).repeat(B, P, 1, 1), "scale": torch.full((B, P), 0.25), "translation": torch.zeros(B, P, 3, 1)}


def test_initial_state():
    size = O.size_cfg(_cfg({"hold": True, "max_ratio": 2}))
    pose = _pose()
    pose["scale"][0, 1], pose["scale"][1, 0], pose["scale"][1, 2] = float("nan"), -1.0, float("inf")
    full = O.entering_size(pose, size)
    assert set(full) == set(O.POSE_KEYS) | set(O.SIZE_KEYS) and all(full[k] is pose[k] for k in O.POSE_KEYS)
    assert full["size_mean"].dtype == torch.float32 and full["size_n"].dtype == torch.int32 and full["size_miss"].dtype == torch.int32
    # init_frames = 0: an empty state whatever the start scale is
    assert not full["size_n"].any() and not full["size_miss"].any() and (full["size_mean"] == 0).all()
    assert O.entering_size(full, size) is full
    # init_frames = 3: the start pose's scale counts for three frames where it is finite and > 0
    full = O.entering_size(pose, {**size, "init_frames": 3})
    assert full["size_n"].tolist() == [[3, 0, 3], [0, 3, 0]] and not full["size_miss"].any()
    assert full["size_mean"].tolist() == [[0.25, 0.0, 0.25], [0.0, 0.25, 0.0]]
    # the model-wide helper: both options' keys, in the order the step returns them
    both = O.entering(_pose(), type("M", (), {"motion": {"gain": 1.0}, "size": size}))
    assert list(both) == list(O.POSE_KEYS) + ["next_rotation", "next_translation", "measured"] + list(O.SIZE_KEYS)
    assert O.entering(pose, type("M", (), {"motion": None, "size": None})) is pose and O.entering(pose, object()) is pose
    # the pose a step starts from keeps the state beside the prediction
    both["next_translation"] = both["translation"] + 1
    start = O.start_pose(both)
    assert set(start) == set(O.POSE_KEYS) | set(O.SIZE_KEYS) and start["translation"] is both["next_translation"] and start["size_n"] is both["size_n"]


def _rec(i, B=2, P=3):
    return {"held": torch.full((B, P), int(i > 1), dtype=torch.int32), "accepted": torch.ones(B, P, dtype=torch.int32),
            "free": torch.full((B, P), 0.25 * i), "n": torch.full((B, P), i, dtype=torch.int32)}


def test_commit_strips_the_state_and_keeps_the_record():
    B, P = 2, 3
    size = O.size_cfg(_cfg({"hold": True, "max_ratio": 2}))
    npcs = {"seg": torch.zeros(1), **{"size_" + k: v for k, v in _rec(1).items()}}
    records = {"size": {}}
    got_npcs, got_pose = O.commit_with_records(lambda i, result: result, records)(1, (npcs, O.entering_size(_pose(B, P), size)))
    assert set(got_npcs) == {"seg"} and set(got_pose) == set(O.POSE_KEYS) and set(records["size"][1]) == {"held", "accepted", "free", "n"}
    # without the option a commit is the batch form's own
    plain = lambda i, result: result           # noqa: E731
    assert O.commit_with_records(plain, {}) is plain


def test_records_to_numpy_lays_out_a_size_record():
    B, P = 2, 3
    pred = {"poses": [{"scale": torch.ones(B, P)}] * 3, "npcs_pred": [None] * 3, "size": [None, _rec(1), _rec(2)]}
    out = O.records_to_numpy(pred)
    assert set(out) == {"size"} and out["size"][0] is None and len(out["size"]) == 3
    for i in (1, 2):
        r = out["size"][i]
        assert set(r) == {"held", "accepted", "free", "n"} and all(isinstance(v, np.ndarray) and v.shape == (B, P) for v in r.values())
        assert r["held"].dtype == np.int32 and r["n"].dtype == np.int32 and r["free"].dtype == np.float32 and (r["n"] == i).all()
    assert "size" not in O.records_to_numpy({"poses": pred["poses"], "npcs_pred": pred["npcs_pred"]})


def test_size_table():
    from captra_amd import eval as E
    assert any(key == "size" and table is E.size_table for key, table, _ in E.RECORD_TABLES)
    arr = lambda *v: np.array([list(v)])           # noqa: E731  one trajectory, two parts
    # part 0: empty state; accepted 0.5 (n 1), accepted 1.0 (n 2: mean 0.75), gated 4.0, restart at 4.0 (n 1).  part 1: three frames
    # counted for frame 0's scale 2.0; accepted 1.0 (n 4: mean 1.75), an invalid frame, accepted 2.75 (n 5: mean 1.95), accepted 1.95
    data = {"pred": {"poses": [{"scale": arr(9.0, 2.0)}]},
            "size": [None,
                     {"held": arr(0, 1), "accepted": arr(1, 1), "free": arr(0.5, 1.0), "n": arr(1, 4)},
                     {"held": arr(1, 1), "accepted": arr(1, 0), "free": arr(1.0, 7.0), "n": arr(2, 4)},
                     {"held": arr(1, 1), "accepted": arr(0, 1), "free": arr(4.0, 2.75), "n": arr(2, 5)},
                     {"held": arr(0, 1), "accepted": arr(1, 1), "free": arr(4.0, 1.95), "n": arr(1, 6)}],
            "st_fit": [None] + [{"valid": arr(1, int(i != 2)), "inliers": arr(9, 9)} for i in range(1, 5)]}
    lines = E.size_table("inst_0", data)
    assert lines == [
        "inst_0 part 0: held 2; accepted 3; gated or invalid 1; restarted 1 (of 4 frames); final mean 4.00000 over 1 frames; free scale min 0.50000 max 4.00000",
        "inst_0 part 1: held 4; accepted 3; gated or invalid 1; restarted 0 (of 4 frames); final mean 1.95000 over 6 frames; free scale min 1.00000 max 2.75000"]
    # without the robust fit's record the free scale spans every frame
    del data["st_fit"]
    assert E.size_table("inst_0", data)[1].endswith("free scale min 1.00000 max 7.00000")
    assert E.size_table("x", {"pred": data["pred"], "size": [None]}) == []


def test_binding_has_the_header_s_argument_list():
    """Every argument of the declaration has its ctypes type, the stream included."""
    import ctypes as C
    import re
    from pathlib import Path
    from captra_amd import _lib
    text = (Path(__file__).resolve().parent.parent / "include" / "captra_hip.h").read_text()
    decl = re.search(r"int captra_part_fit_st_size\(([^;]*)\);", text).group(1)
    args = [" ".join(a.split()) for a in decl.split(",")]
    types = _lib._SIGNATURES["captra_part_fit_st_size"]
    assert len(args) == len(types) == 43
    for a, t in zip(args, types):
        want = (C.c_void_p if "*" in a or "captra_stream_t" in a else C.c_float if a.startswith("float") else
                C.c_ulonglong if a.startswith("unsigned long long") else C.c_int)
        assert t is want, (a, t)
