"""The configuration surface of the camera model: the `camera` section and its flags (track_options.camera_cfg), every error it raises
and the key it names, the precedence frame 0's camera > the configuration's > none (track_options.trajectory_cameras, the model's
set_data), a camera that changes between frames, several image sizes in one batch, the `.npz` keys through save / load / stack /
concat with a mixed stack, synthetic's `cameras` (default = the shipped frames, byte for byte), the table of captra_amd.eval and the
binding rows."""
import argparse

import numpy as np
import pytest
import torch

from tests.test_image_fit_cfg_cpu import SHIPPED_DIGEST, _digest

REAL = np.array([[591.0125, 0.0, 322.525], [0.0, 590.16775, 244.11084], [0.0, 0.0, 1.0]])
CAMERA25 = np.array([[577.5, 0.0, 319.5], [0.0, 577.5, 239.5], [0.0, 0.0, 1.0]])


def _cfg(otf=True, **section):
    from captra_amd.configs import make_config
    return make_config("1", nocs_otf=otf, **{f"camera/{k}": v for k, v in section.items()})


def test_absent_means_none():
    from captra_amd import track_options as O
    from captra_amd.configs import make_config
    assert "camera" not in make_config("1") and O.camera_cfg(make_config("1")) is None
    assert O.camera_cfg(make_config("1", nocs_otf=True)) is None
    assert O.trajectory_cameras(None, None, 3) is None


def test_presets_and_explicit_keys_parse_to_the_same_tables():
    from captra_amd import nocs_otf, track_options as O
    for preset, K in (("nocs_real", REAL), ("nocs_camera", CAMERA25)):
        a = O.camera_cfg(_cfg(preset=preset))
        b = O.camera_cfg(_cfg(fx=K[0, 0], fy=K[1, 1], cx=K[0, 2], cy=K[1, 2]))                # skew and depth_unit default to 0 and 0.001
        c = O.camera_cfg(_cfg(fx=K[0, 0], fy=K[1, 1], cx=K[0, 2], cy=K[1, 2], skew=0, depth_unit=0.001))
        assert a["K"].tobytes() == K.tobytes() == b["K"].tobytes() == c["K"].tobytes() and a["depth_unit"] == b["depth_unit"] == c["depth_unit"] == 0.001
        tabs = [nocs_otf.camera_rows(x["K"][None], [x["depth_unit"]]) for x in (a, b, c)]
        assert all(t[0].tobytes() == tabs[0][0].tobytes() and t[1].tolist() == [0] for t in tabs)
        assert tabs[0][0][0, 9:18].tobytes() == nocs_otf._kinv(K).tobytes() and tabs[0][0].shape == (1, 19)
    assert nocs_otf.NOCS_REAL_INTRINSICS.tobytes() == REAL.tobytes()
    skewed = O.camera_cfg(_cfg(fx=500, fy=510.5, cx=300, cy=200, skew=0.25, depth_unit=0.0005))
    assert skewed["K"].tolist() == [[500.0, 0.25, 300.0], [0.0, 510.5, 200.0], [0.0, 0.0, 1.0]] and skewed["depth_unit"] == 0.0005


def test_parse_args_builds_the_section():
    from captra_amd.configs import make_config
    from captra_amd.parse_args import add_args
    argv = ["--camera/fx", "577.5", "--camera/fy", "577.5", "--camera/cx", "319.5", "--camera/cy", "239.5", "--camera/skew", "0", "--camera/depth_unit", "0.001"]
    over = {k: v for k, v in vars(add_args(argparse.ArgumentParser()).parse_args(argv)).items() if k.startswith("camera/")}
    assert over == {"camera/fx": 577.5, "camera/fy": 577.5, "camera/cx": 319.5, "camera/cy": 239.5, "camera/skew": 0.0, "camera/depth_unit": 0.001}
    from captra_amd import track_options as O
    assert O.camera_cfg(make_config("1", nocs_otf=True, **over))["K"].tobytes() == CAMERA25.tobytes()
    over = {k: v for k, v in vars(add_args(argparse.ArgumentParser()).parse_args(["--camera/preset", "nocs_camera"])).items() if k.startswith("camera/")}
    assert over == {"camera/preset": "nocs_camera"}
    assert not any(k.startswith("camera/") for k in vars(add_args(argparse.ArgumentParser()).parse_args([])))     # not given: no section


GOOD = dict(fx=500.0, fy=500.0, cx=320.0, cy=240.0)


@pytest.mark.parametrize("section,word", [
    ({k: v for k, v in GOOD.items() if k != "fx"}, "camera/fx"), ({k: v for k, v in GOOD.items() if k != "fy"}, "camera/fy"),
    ({k: v for k, v in GOOD.items() if k != "cx"}, "camera/cx"), ({k: v for k, v in GOOD.items() if k != "cy"}, "camera/cy"),
    ({**GOOD, "fx": 0.0}, "camera/fx"), ({**GOOD, "fx": -3.0}, "camera/fx"), ({**GOOD, "fy": 0.0}, "camera/fy"),
    ({**GOOD, "fx": float("nan")}, "camera/fx"), ({**GOOD, "fy": float("inf")}, "camera/fy"), ({**GOOD, "cx": float("inf")}, "camera/cx"),
    ({**GOOD, "cy": float("nan")}, "camera/cy"), ({**GOOD, "skew": float("nan")}, "camera/skew"),
    ({**GOOD, "depth_unit": 0.0}, "camera/depth_unit"), ({**GOOD, "depth_unit": -0.001}, "camera/depth_unit"),
    ({**GOOD, "depth_unit": float("inf")}, "camera/depth_unit"), ({**GOOD, "depth_unit": float("nan")}, "camera/depth_unit"),
    ({**GOOD, "fx": "wide"}, "camera/fx"), ({**GOOD, "fx": True}, "camera/fx"),
    (dict(preset="kinect"), "camera/preset"), (dict(preset="nocs_real", fx=500.0), "camera/preset"), ({**GOOD, "k1": 0.1}, "k1"),
])
def test_errors_name_the_key(section, word):
    from captra_amd import track_options as O
    with pytest.raises(ValueError, match=word):
        O.camera_cfg(_cfg(**section))


def test_last_row_and_shapes_of_a_carried_camera():
    from captra_amd import nocs_otf, track_options as O
    bad = REAL.copy()
    bad[2] = (0.0, 1e-9, 1.0)
    with pytest.raises(ValueError, match="last row"):
        nocs_otf.check_camera(bad, 0.001)
    with pytest.raises(ValueError, match="trajectory 1.*last row"):
        O.trajectory_cameras({"K": np.stack([REAL, bad]), "depth_unit": np.array([0.001, 0.001])}, None, 2)
    with pytest.raises(ValueError, match="trajectory 0.*depth_unit"):
        O.trajectory_cameras({"K": np.stack([REAL, REAL]), "depth_unit": np.array([0.0, 0.001])}, None, 2)
    with pytest.raises(ValueError, match="B = 3"):
        O.trajectory_cameras({"K": np.stack([REAL, REAL]), "depth_unit": np.array([0.001, 0.001])}, None, 3)
    with pytest.raises(ValueError, match="depth_unit"):
        O.trajectory_cameras({"K": REAL[None]}, None, 1)
    low = REAL.copy()
    low[1, 0] = 0.5
    with pytest.raises(ValueError, match=r"K\[1\]\[0\]"):
        nocs_otf.check_camera(low, 0.001)


def test_camera_without_a_depth_image_is_refused():
    from captra_amd import track_options as O
    from captra_amd.configs import make_config
    with pytest.raises(ValueError, match="nocs_otf"):
        O.camera_cfg(_cfg(otf=False, preset="nocs_real"))
    assert O.camera_cfg(make_config("1", **{"camera/preset": "nocs_camera", "init_frame/image_fit": True})) is not None


def test_precedence():
    from captra_amd import track_options as O
    cfg_cam = O.camera_cfg(_cfg(preset="nocs_camera"))
    own = {"K": torch.from_numpy(np.stack([REAL, CAMERA25 * np.array([[2.0], [2.0], [1.0]])])), "depth_unit": torch.tensor([0.001, 0.0005], dtype=torch.float64)}
    got = O.trajectory_cameras(own, cfg_cam, 2)                                      # frame 0's own first
    assert got["K"].tobytes() == own["K"].numpy().tobytes() and got["depth_unit"].tolist() == [0.001, 0.0005]
    got = O.trajectory_cameras(None, cfg_cam, 2)                                     # then the configuration's, for every trajectory
    assert got["K"].shape == (2, 3, 3) and (got["K"] == CAMERA25).all() and got["depth_unit"].tolist() == [0.001, 0.001]
    assert O.trajectory_cameras(None, None, 2) is None                               # then none


def _model(**section):
    from captra_amd.trainer import Trainer
    cfg = _cfg(**section)
    cfg["device"] = "cpu"
    return Trainer(cfg).model


def test_the_model_keeps_the_cameras_and_refuses_a_change():
    from captra_amd import synthetic as S
    m = _model()
    assert m.camera_cfg is None
    m.set_data(S.make_otf_trajectory(2, 2, seed=1))
    assert m.camera is None and m._camera_host is None                              # option absent: no tensor
    cams = [(None, 0.001, 1), (CAMERA25, 0.0005, 2)]
    m.set_data(S.make_otf_trajectory(2, 2, seed=1, cameras=cams))
    table, cam_of = m.camera
    assert table.dtype == torch.float64 and tuple(table.shape) == (2, 19) and cam_of.dtype == torch.int32 and cam_of.tolist() == [0, 1]
    assert table[1, :9].numpy().tobytes() == CAMERA25.tobytes() and table[:, 18].tolist() == [0.001, 0.0005]
    assert m._camera_host["K"].shape == (2, 3, 3) and m._camera_host["depth_unit"].tolist() == [0.001, 0.0005]
    m2 = _model(preset="nocs_camera")
    m2.set_data(S.make_otf_trajectory(3, 2, seed=1))                                 # the configuration's: one row, three trajectories
    assert tuple(m2.camera[0].shape) == (1, 19) and m2.camera[1].tolist() == [0, 0, 0] and m2.camera[0][0, :9].numpy().tobytes() == CAMERA25.tobytes()
    m2.set_data(S.make_otf_trajectory(2, 2, seed=1, cameras=cams))                   # frame 0's own wins
    assert tuple(m2.camera[0].shape) == (2, 19)
    data = S.make_otf_trajectory(2, 3, seed=1, cameras=cams)
    data[2]["meta"]["pre_fetched"]["camera"] = {"K": data[2]["meta"]["pre_fetched"]["camera"]["K"].clone(), "depth_unit": torch.tensor([0.001, 0.001], dtype=torch.float64)}
    with pytest.raises(ValueError, match="frame 2.*differs from frame 0"):
        m.set_data(data)
    data = S.make_otf_trajectory(2, 3, seed=1)
    data[1]["meta"]["pre_fetched"]["camera"] = {"K": torch.from_numpy(np.stack([REAL, REAL])), "depth_unit": torch.tensor([0.001, 0.001], dtype=torch.float64)}
    with pytest.raises(ValueError, match="frame 1.*differs from frame 0"):
        m.set_data(data)
    del data[1]["meta"]["pre_fetched"]["camera"]
    m.set_data(data)
    assert m.camera is None


def test_several_image_sizes_in_one_batch_raise(tmp_path):
    from captra_amd import synthetic as S
    from captra_amd.trajectory_io import concat_frame_batches, load_trajectory_npz, save_trajectory_npz, stack_trajectories
    data = S.make_otf_trajectory(2, 2, seed=1)
    small = [dict(f, meta=dict(f["meta"], pre_fetched={k: v[:, :240, :320] for k, v in f["meta"]["pre_fetched"].items()})) for f in data]
    save_trajectory_npz(str(tmp_path / "a.npz"), data, 0)
    save_trajectory_npz(str(tmp_path / "b.npz"), small, 1)
    trajs = [load_trajectory_npz(str(tmp_path / n)) for n in ("a.npz", "b.npz")]
    with pytest.raises(ValueError, match=r"share their size H x W.*\(240, 320\).*\(480, 640\)"):
        stack_trajectories(trajs)
    with pytest.raises(ValueError, match="share their size H x W"):
        concat_frame_batches([stack_trajectories(trajs[:1]), stack_trajectories(trajs[1:])])
    ragged = [dict(f, meta=dict(f["meta"], pre_fetched={"depth": [f["meta"]["pre_fetched"]["depth"][0], f["meta"]["pre_fetched"]["depth"][1][:240, :320]],
                                                         "mask": [f["meta"]["pre_fetched"]["mask"][0], f["meta"]["pre_fetched"]["mask"][1][:240, :320]]})) for f in data]
    with pytest.raises(ValueError, match="several image sizes"):
        _model().set_data(ragged)


def test_npz_round_trip_and_the_mixed_stack(tmp_path):
    from captra_amd import synthetic as S, track_options as O
    from captra_amd.trajectory_io import concat_frame_batches, load_trajectory_npz, save_trajectory_npz, stack_trajectories
    cams = [(CAMERA25, 0.0005, 2), (None, 0.001, 1)]
    with_c, without = S.make_otf_trajectory(2, 2, seed=4, cameras=cams), S.make_otf_trajectory(2, 2, seed=4)
    for b in range(2):
        save_trajectory_npz(str(tmp_path / f"c{b}.npz"), with_c, b)
        save_trajectory_npz(str(tmp_path / f"p{b}.npz"), without, b)
    tc = [load_trajectory_npz(str(tmp_path / f"c{b}.npz")) for b in range(2)]
    tp = [load_trajectory_npz(str(tmp_path / f"p{b}.npz")) for b in range(2)]
    assert tc[0]["camera_K"].dtype == np.float64 and tc[0]["camera_K"].tobytes() == CAMERA25.tobytes() and float(tc[0]["camera_depth_unit"]) == 0.0005
    assert tc[1]["camera_K"].tobytes() == REAL.tobytes() and all("camera_K" not in t and "camera_depth_unit" not in t for t in tp)
    fc, fp = stack_trajectories(tc), stack_trajectories(tp)
    assert all("camera" not in f["meta"]["pre_fetched"] for f in fp)                   # files without it load as before
    for f, g in zip(fc, with_c):
        cam = f["meta"]["pre_fetched"]["camera"]
        assert cam["K"].dtype == torch.float64 and cam["K"].numpy().tobytes() == g["meta"]["pre_fetched"]["camera"]["K"].numpy().tobytes()
        assert cam["depth_unit"].tolist() == [0.0005, 0.001]
        assert np.array_equal(f["meta"]["pre_fetched"]["depth"].numpy(), g["meta"]["pre_fetched"]["depth"].numpy())
    # a mixed stack: the trajectory without a camera gets the configuration's, or NOCS REAL
    mixed = stack_trajectories([tc[0], tp[1]])
    assert mixed[0]["meta"]["pre_fetched"]["camera"]["K"][1].numpy().tobytes() == REAL.tobytes()
    assert mixed[0]["meta"]["pre_fetched"]["camera"]["depth_unit"].tolist() == [0.0005, 0.001]
    cfg_cam = O.camera_cfg(_cfg(fx=400.0, fy=410.0, cx=300.0, cy=200.0, depth_unit=0.002))
    mixed = stack_trajectories([tp[0], tc[0]], default_camera=cfg_cam)
    cam = mixed[1]["meta"]["pre_fetched"]["camera"]
    assert cam["K"][0].numpy().tobytes() == cfg_cam["K"].tobytes() and cam["K"][1].numpy().tobytes() == CAMERA25.tobytes()
    assert cam["depth_unit"].tolist() == [0.002, 0.0005]
    both = concat_frame_batches([stack_trajectories(tc[:1]), stack_trajectories(tc[1:])])
    assert both[1]["meta"]["pre_fetched"]["camera"]["K"].numpy().tobytes() == fc[1]["meta"]["pre_fetched"]["camera"]["K"].numpy().tobytes()
    both = concat_frame_batches([stack_trajectories(tp[:1]), stack_trajectories(tc[:1])], default_camera=cfg_cam)
    assert both[0]["meta"]["pre_fetched"]["camera"]["depth_unit"].tolist() == [0.002, 0.0005]
    both = concat_frame_batches([stack_trajectories(tp[:1]), stack_trajectories(tc[:1])])
    assert both[0]["meta"]["pre_fetched"]["camera"]["K"][0].numpy().tobytes() == REAL.tobytes()
    assert all("camera" not in f["meta"]["pre_fetched"] for f in concat_frame_batches([stack_trajectories(tp[:1]), stack_trajectories(tp[1:])]))
    # a file with half a camera is refused
    with np.load(str(tmp_path / "c0.npz")) as z:
        half = {k: z[k] for k in z.files if k != "camera_depth_unit"}
    np.savez(str(tmp_path / "half.npz"), **half)
    with pytest.raises(ValueError, match="camera_K"):
        load_trajectory_npz(str(tmp_path / "half.npz"))


def test_synthetic_defaults_are_the_shipped_frames_and_a_scaled_sensor_is_exact():
    from captra_amd import synthetic as S
    assert _digest(S.make_otf_trajectory(2, 2, seed=1)) == SHIPPED_DIGEST
    assert _digest(S.make_otf_trajectory(2, 2, seed=1, cameras=None)) == SHIPPED_DIGEST
    a, b = S.make_frame(3), S.make_frame(3, intrinsics=None, depth_scale=1)
    assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a[:3], b[:3]))
    two = S.make_frame(3, depth_scale=2)
    assert two[0].dtype == np.uint16 and (two[0] == 2 * a[0].astype(np.int64)).all() and two[2].tobytes() == a[2].tobytes()
    frames = S.make_otf_trajectory(2, 2, seed=1, cameras=[(None, 0.001, 1), (None, 0.0005, 2)], coord=True)
    plain = S.make_otf_trajectory(2, 2, seed=1, coord=True)
    for f, g in zip(frames, plain):
        d, e = f["meta"]["pre_fetched"]["depth"], g["meta"]["pre_fetched"]["depth"]
        assert (d[0] == e[0]).all() and (d[1] == 2 * e[1]).all()
        assert f["meta"]["pre_fetched"]["camera"]["depth_unit"].tolist() == [0.001, 0.0005]
    assert (frames[0]["meta"]["pre_fetched"]["coord"] == plain[0]["meta"]["pre_fetched"]["coord"]).all()     # the same 3D blob
    for f in frames:
        del f["meta"]["pre_fetched"]["camera"]
        f["meta"]["pre_fetched"]["depth"][1] //= 2
    assert _digest([dict(f, meta=dict(f["meta"], pre_fetched={k: v for k, v in f["meta"]["pre_fetched"].items() if k != "coord"})) for f in frames]) == SHIPPED_DIGEST
    other = S.make_frame(3, intrinsics=CAMERA25)
    assert other[0].tobytes() == a[0].tobytes() and not np.array_equal(other[2], a[2])     # the same pixels, seen through another K
    with pytest.raises(ValueError, match="uint16"):
        S.make_frame(3, depth_scale=64)


def test_records_and_eval_list_the_camera():
    from captra_amd import track_options as O
    from captra_amd.eval import RECORD_TABLES, camera_table
    from captra_amd.utils import get_ith_from_batch
    assert O.records_to_numpy({"poses": []}) == {}
    K = np.stack([REAL, np.array([[500.0, 0.25, 300.0], [0.0, 510.5, 200.0], [0.0, 0.0, 1.0]])])
    rec = O.records_to_numpy({"poses": [], "camera": {"K": K, "depth_unit": np.array([0.001, 0.0005])}})
    assert set(rec) == {"camera"} and rec["camera"]["K"].dtype == np.float64
    one = get_ith_from_batch(rec, 1, to_single=False)
    assert camera_table("inst1_track0", one) == ["inst1_track0: fx 500; fy 510.5; cx 300; cy 200; skew 0.25; depth unit 0.0005 m"]
    assert camera_table("x", get_ith_from_batch(rec, 0, to_single=False)) == ["x: fx 591.013; fy 590.168; cx 322.525; cy 244.111; depth unit 0.001 m"]
    assert any(key == "camera" and table is camera_table for key, table, _ in RECORD_TABLES)


def test_binding_rows_match_the_header():
    """Argument count and pointer places of the five rows against their declarations (stream included), and against their plain
    counterparts: the single matrix replaced by (int ncam, cams, cam_of)."""
    import re
    from pathlib import Path
    from captra_amd import _lib
    text = (Path(__file__).resolve().parent.parent / "include" / "captra_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for plain in ("captra_crop_box", "captra_crop_box_det", "captra_crop_ball", "captra_crop_ball_det", "captra_image_members"):
        name = plain + "_cam"
        params = [p.strip() for p in re.search(rf"\b{name}\s*\(([^;]*?)\)\s*;", text, flags=re.S).group(1).split(",")]
        base = [p.strip() for p in re.search(rf"\b{plain}\s*\(([^;]*?)\)\s*;", text, flags=re.S).group(1).split(",")]
        sig = _lib._SIGNATURES[name]
        assert len(sig) == len(params) == len(base) + 2, name
        for p, t in zip(params, sig):
            assert ("*" in p or "captra_stream_t" in p) == (t is _lib._P), (name, p)
        at = next(i for i, p in enumerate(base) if p.split()[-1].lstrip("*") in ("kmat", "kinv"))
        assert [p.split()[-1].lstrip("*") for p in params[at:at + 3]] == ["ncam", "cams", "cam_of"], name
        assert [re.sub(r"\s+", " ", p) for p in params[:at] + params[at + 3:]] == [re.sub(r"\s+", " ", p) for p in base[:at] + base[at + 1:]], name


def test_wrappers_refuse_bad_camera_tensors():
    from captra_amd import nocs_otf
    tab, cam_of = nocs_otf.camera_table(np.stack([REAL, CAMERA25, REAL]), [0.001, 0.001, 0.001], "cpu")
    assert tuple(tab.shape) == (2, 19) and tab.dtype == torch.float64 and cam_of.dtype == torch.int32 and cam_of.tolist() == [0, 1, 0]      # by bytes
    assert nocs_otf.camera_table(np.stack([REAL, REAL]), [0.001, 0.0005], "cpu")[1].tolist() == [0, 1]                                   # the unit is part of a camera
    dev = torch.device("cpu")
    for bad, word in (((tab.float(), cam_of), "float64"), ((tab[:, :18].contiguous(), cam_of), "19"), ((tab, cam_of.long()), "int32"),
                      ((tab, cam_of[:2]), "B = 3"), ((tab[:0], cam_of), "C >= 1")):
        with pytest.raises(ValueError, match=word):
            nocs_otf._check_cameras(bad, 3, dev)
    d, m = torch.zeros(3, 4, 4, dtype=torch.int32), torch.ones(3, 4, 4, dtype=torch.bool)
    with pytest.raises(ValueError, match="on the device"):
        nocs_otf.full_data_batch_arrays(d, m, np.zeros((3, 3)), np.ones(3), None, 4, cameras=(tab, cam_of))
