"""track_cfg/box as far as it is plumbing (captra_amd/track_options.py, pose_utils/bbox_utils.py, captra_amd/eval.py, captra_amd/_lib.py),
without a GPU: the parser and its ranges, the records table's row, a track's initial histograms, what a commit keeps, the corner
helper in numpy and torch, the pickle entry, the eval CLI's table and the command-line flags."""
import numpy as np
import pytest
import torch

from captra_amd import track_options as O


def _cfg(box, sym=False):
    return {"track_cfg": {} if box is None else {"box": box}, "data_radius": 0.6, "obj_sym": sym, "obj_category": "1" if sym else "6"}


def test_box_cfg():
    assert O.box_cfg(_cfg(None)) is None
    assert O.box_cfg(_cfg({"quantile": 0.95})) is None
    assert O.box_cfg(_cfg({"hold": False, "quantile": 0.95})) is None
    assert O.box_cfg(_cfg({"hold": True, "quantile": 0.95})) == {"quantile_permille": 950, "bins": 128, "min_points": 16, "radial": False}
    got = O.box_cfg(_cfg({"hold": True, "quantile": 0.999, "bins": 512, "min_points": 1, "radial": True}, sym=True))
    assert got == {"quantile_permille": 999, "bins": 512, "min_points": 1, "radial": True}
    assert O.box_cfg(_cfg({"hold": True, "quantile": 0.5}))["quantile_permille"] == 500
    assert O.box_cfg(_cfg({"hold": True, "quantile": 1}))["quantile_permille"] == 1000
    assert O.box_cfg(_cfg({"hold": True, "quantile": 0.9, "bins": None, "min_points": None}))["bins"] == 128
    # every thousandth in range is taken as written, whatever its binary neighbour is
    assert [O.box_cfg(_cfg({"hold": True, "quantile": k / 1000}))["quantile_permille"] for k in range(500, 1001)] == list(range(500, 1001))
    with pytest.raises(ValueError, match="track_cfg/box/quantile.*no default"):
        O.box_cfg(_cfg({"hold": True}))
    for bad, path in (({"quantile": 0.499}, "quantile"), ({"quantile": 1.001}, "quantile"), ({"quantile": float("nan")}, "quantile"),
                      ({"quantile": 0.9505}, "quantile.*thousandths"), ({"quantile": "0.9"}, "quantile"), ({"quantile": True}, "quantile"),
                      ({"quantile": 0.9, "bins": 100}, "bins"), ({"quantile": 0.9, "bins": 1024}, "bins"), ({"quantile": 0.9, "bins": 32}, "bins"),
                      ({"quantile": 0.9, "bins": 128.5}, "bins"), ({"quantile": 0.9, "min_points": 0}, "min_points"),
                      ({"quantile": 0.9, "min_points": 1.5}, "min_points"), ({"quantile": 0.9, "min_points": 2 ** 31}, "min_points"),
                      ({"quantile": 0.9, "min_points": True}, "min_points")):
        with pytest.raises(ValueError, match=f"track_cfg/box/{path}"):
            O.box_cfg(_cfg({"hold": True, **bad}))
    # radial is for the symmetric categories, as yaxis_only is
    with pytest.raises(ValueError, match="track_cfg/box/radial.*symmetric"):
        O.box_cfg(_cfg({"hold": True, "quantile": 0.9, "radial": True}, sym=False))
    assert O.box_cfg(_cfg({"hold": True, "quantile": 0.9, "radial": False}, sym=False))["radial"] is False
    assert O.STEP_RECORDS["box"] == ("box_", ("extent", "frame", "added", "total"))
    assert O.BOX_KEY == "box_hist"


def test_command_line_flags_reach_the_parser():
    import argparse
    from captra_amd.parse_args import add_args
    ns = vars(add_args(argparse.ArgumentParser()).parse_args([]))
    assert not any(k.startswith("track_cfg/box") for k in ns)                 # not given = not in the namespace
    ns = vars(add_args(argparse.ArgumentParser()).parse_args(["--track_cfg/box/hold", "True", "--track_cfg/box/quantile", "0.95",
                                                              "--track_cfg/box/bins", "256", "--track_cfg/box/min_points", "32",
                                                              "--track_cfg/box/radial", "True"]))
    box = {k.split("/")[-1]: v for k, v in ns.items() if k.startswith("track_cfg/box")}
    assert box == {"hold": True, "quantile": 0.95, "bins": 256, "min_points": 32, "radial": True}
    assert O.box_cfg(_cfg(box, sym=True)) == {"quantile_permille": 950, "bins": 256, "min_points": 32, "radial": True}


def _pose(B=2, P=3):
    return {"rotation": torch.eye(3).repeat(B, P, 1, 1), "scale": torch.full((B, P), 0.25), "translation": torch.zeros(B, P, 3, 1)}


def test_initial_state_and_the_travelling_dict():
    box = O.box_cfg(_cfg({"hold": True, "quantile": 0.9, "bins": 64}))
    pose = _pose()
    full = O.entering_box(pose, box)
    assert set(full) == set(O.POSE_KEYS) | {"box_hist"} and all(full[k] is pose[k] for k in O.POSE_KEYS)
    assert full["box_hist"].shape == (2, 3, 3, 64) and full["box_hist"].dtype == torch.int32 and not full["box_hist"].any()
    assert O.entering_box(full, box) is full
    size = {"max_ratio": 2.0, "min_frames": 1, "max_frames": None, "reset_after": None, "init_frames": 0}
    every = O.entering(_pose(), type("M", (), {"motion": {"gain": 1.0}, "size": size, "box": box}))
    assert list(every) == list(O.POSE_KEYS) + ["next_rotation", "next_translation", "measured"] + list(O.SIZE_KEYS) + ["box_hist"]
    only = O.entering(pose, type("M", (), {"motion": None, "size": None, "box": box}))
    assert set(only) == set(O.POSE_KEYS) | {"box_hist"}
    assert O.entering(pose, type("M", (), {"motion": None, "size": None, "box": None})) is pose and O.entering(pose, object()) is pose
    # the pose a step starts from keeps the histograms beside the prediction; without a prediction the dict itself
    every["next_translation"] = every["translation"] + 1
    start = O.start_pose(every)
    assert set(start) == set(O.POSE_KEYS) | set(O.SIZE_KEYS) | {"box_hist"}
    assert start["translation"] is every["next_translation"] and start["box_hist"] is every["box_hist"]
    assert O.start_pose(only) is only


def _rec(i, B=2, P=3):
    return {"extent": torch.full((B, P, 3), 0.125 * i), "frame": torch.full((B, P, 3), 0.25), "added": torch.full((B, P), 100, dtype=torch.int32),
            "total": torch.full((B, P), 100 * i, dtype=torch.int32)}


def test_commit_strips_the_state_and_keeps_the_record():
    box = O.box_cfg(_cfg({"hold": True, "quantile": 0.9}))
    npcs = {"seg": torch.zeros(1), **{"box_" + k: v for k, v in _rec(1).items()}}
    records = {"box": {}}
    got_npcs, got_pose = O.commit_with_records(lambda i, result: result, records)(1, (npcs, O.entering_box(_pose(), box)))
    assert set(got_npcs) == {"seg"} and set(got_pose) == set(O.POSE_KEYS) and set(records["box"][1]) == {"extent", "frame", "added", "total"}


def test_records_to_numpy_lays_out_a_box_record():
    B, P = 2, 3
    pred = {"poses": [{"scale": torch.ones(B, P)}] * 3, "npcs_pred": [None] * 3, "box": [None, _rec(1), _rec(2)]}
    out = O.records_to_numpy(pred)
    assert set(out) == {"box"} and out["box"][0] is None and len(out["box"]) == 3
    for i in (1, 2):
        r = out["box"][i]
        assert set(r) == {"extent", "frame", "added", "total"} and r["extent"].shape == (B, P, 3) and r["added"].shape == (B, P)
        assert r["extent"].dtype == np.float32 and r["total"].dtype == np.int32 and (r["total"] == 100 * i).all()
    assert "box" not in O.records_to_numpy({"poses": pred["poses"], "npcs_pred": pred["npcs_pred"]})


def test_held_box_corners():
    from captra_amd.pose_utils.bbox_utils import held_box_corners
    rng = np.random.default_rng(3)
    size = rng.uniform(0.1, 0.5, size=(4, 2, 3, 3))                        # (frames, B, P, 3)
    ref = np.stack([-size, size], axis=-2)                                 # (frames, B, P, 2, 3)
    extent = rng.uniform(0.1, 0.5, size=(4, 2, 3, 3)).astype(np.float32)
    extent[0] = 0.0                          # nothing established
    extent[1, 0, 1, 2] = 0.0                 # one axis short: the whole part keeps the reference's box
    extent[2, 1, 0] = (0.25, 0.0, 0.25)
    got = held_box_corners(ref, extent)
    assert got.shape == ref.shape and got.dtype == ref.dtype
    est = (extent > 0).all(-1)
    assert est.sum() == 24 - 6 - 1 - 1
    e = extent.astype(np.float64)
    np.testing.assert_array_equal(got[est], np.stack([-e, e], axis=-2)[est])
    np.testing.assert_array_equal(got[~est], ref[~est])
    # one frame (B,P,2,3), and torch gives the same values in the corners' dtype
    np.testing.assert_array_equal(held_box_corners(ref[3], extent[3]), got[3])
    t = held_box_corners(torch.from_numpy(ref).float(), torch.from_numpy(extent))
    assert isinstance(t, torch.Tensor) and t.dtype == torch.float32
    np.testing.assert_array_equal(t.numpy(), held_box_corners(ref.astype(np.float32), extent))
    np.testing.assert_array_equal(t.numpy()[est], np.stack([-extent, extent], axis=-2)[est])


def test_box_table():
    from captra_amd import eval as E
    assert any(key == "box" and table is E.box_table for key, table, _ in E.RECORD_TABLES)
    ext = lambda a, b: np.array([a, b], np.float32)            # noqa: E731  one trajectory, two parts
    cnt = lambda a, b: np.array([a, b], np.int32)              # noqa: E731
    # part 0: established after frame 1, frame 3 skipped on the guard's verdict (members, no growth); part 1: too few values until frame 3
    data = {"box": [None,
                    {"extent": ext([0.25, 0.5, 0.25], [0, 0, 0]), "frame": ext([0.25, 0.5, 0.25], [0, 0, 0]), "added": cnt(100, 5), "total": cnt(100, 5)},
                    {"extent": ext([0.25, 0.5, 0.25], [0, 0, 0]), "frame": ext([0.375, 0.5, 0.125], [0, 0, 0]), "added": cnt(100, 5), "total": cnt(200, 10)},
                    {"extent": ext([0.25, 0.5, 0.25], [0.125, 0.125, 0.25]), "frame": ext([0.5, 0.5, 0.5], [0.125, 0.125, 0.25]), "added": cnt(100, 20),
                     "total": cnt(200, 30)},
                    {"extent": ext([0.375, 0.5, 0.25], [0.125, 0.25, 0.25]), "frame": ext([0.375, 0.5, 0.25], [0, 0, 0]), "added": cnt(100, 0),
                     "total": cnt(300, 30)}]}
    lines = E.box_table("inst_0", data)
    assert lines == [
        "inst_0 part 0: half-extents 0.3750 0.5000 0.2500; established at frame 1; skipped on the guard's verdict 1 (of 4 frames); 300 values held; "
        "x frame 0.2500-0.5000 held 0.2500-0.3750; y frame 0.5000-0.5000 held 0.5000-0.5000; z frame 0.1250-0.5000 held 0.2500-0.2500",
        "inst_0 part 1: half-extents 0.1250 0.2500 0.2500; established at frame 3; skipped on the guard's verdict 0 (of 4 frames); 30 values held; "
        "x frame 0.0000-0.1250 held 0.1250-0.1250; y frame 0.0000-0.1250 held 0.1250-0.2500; z frame 0.0000-0.2500 held 0.2500-0.2500"]
    assert E.box_table("x", {"box": [None]}) == []


def test_binding_has_the_header_s_argument_list():
    """Every argument of the declaration has its ctypes type, the stream included; the A/B knob is declared and bound too."""
    import ctypes as C
    import re
    from pathlib import Path
    from captra_amd import _lib
    text = (Path(__file__).resolve().parent.parent / "include" / "captra_hip.h").read_text()
    decl = re.search(r"int captra_part_box_hist\(([^;]*)\);", text).group(1)
    args = [" ".join(a.split()) for a in decl.split(",")]
    types = _lib._SIGNATURES["captra_part_box_hist"]
    assert len(args) == len(types) == 17
    for a, t in zip(args, types):
        assert t is (C.c_void_p if "*" in a or "captra_stream_t" in a else C.c_int), (a, t)
    assert "captra_part_box_set_subhists" in _lib._AUX_SIGNATURES and "void captra_part_box_set_subhists(int sub);" in text
    from captra_amd.pose_utils import pose_fit
    assert pose_fit.BOX_BINS == (64, 128, 256, 512) and callable(pose_fit.part_box_hist)
