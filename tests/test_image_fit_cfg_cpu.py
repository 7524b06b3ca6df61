"""The configuration surface of init_frame/image_fit (the first pose fitted from frame 0's depth, mask and NOCS coordinate image):
the flags, track_options.image_fit_cfg and every error it raises, the error of a frame 0 without its images, the optional `coord`
array of the trajectory files, synthetic's `coord` (default = the shipped frames, byte for byte), the table of captra_amd.eval and the
binding row."""
import argparse
import hashlib

import numpy as np
import pytest

# sha256 over every array and name of make_otf_trajectory(2, 2, seed=1) as it was before `coord` existed (_digest below)
SHIPPED_DIGEST = "4d3514eb3c15be57bee96bb9e141e12b303ee9d91486407d88fd7120cb9b64b5"


def _cfg(**section):
    from captra_amd.configs import make_config
    return make_config("1", nocs_otf=True, **{f"init_frame/{k}": v for k, v in section.items()})


def _digest(frames) -> str:
    h = hashlib.sha256()
    for f in frames:
        for k in ("points", "labels", "nocs"):
            h.update(f[k].numpy().tobytes())
        m = f["meta"]
        h.update(repr(sorted(m)).encode())
        h.update(repr(sorted(m["pre_fetched"])).encode())
        for k in sorted(m["pre_fetched"]):
            h.update(np.asarray(m["pre_fetched"][k]).tobytes())
        h.update(m["points_mean"].numpy().tobytes())
        h.update(m["nocs_corners"].numpy().tobytes())
        h.update(repr(m["path"] + m["ori_path"]).encode())
        for p in m["nocs2camera"]:
            for k in ("rotation", "translation", "scale"):
                h.update(p[k].numpy().tobytes())
    return h.hexdigest()


def test_parse_args_builds_the_option():
    from captra_amd.configs import make_config
    from captra_amd.parse_args import add_args
    argv = ["--init_frame/image_fit", "True", "--init_frame/border", "2", "--init_frame/cap", "4096", "--init_frame/coord_negate_z", "True"]
    args = add_args(argparse.ArgumentParser()).parse_args(argv)
    over = {k: v for k, v in vars(args).items() if k in ("init_frame/image_fit", "init_frame/border", "init_frame/cap", "init_frame/coord_negate_z")}
    assert over == {"init_frame/image_fit": True, "init_frame/border": 2, "init_frame/cap": 4096, "init_frame/coord_negate_z": True}
    init = make_config("1", **over)["init_frame"]
    assert (init["image_fit"], init["border"], init["cap"], init["coord_negate_z"]) == (True, 2, 4096, True)
    none = vars(add_args(argparse.ArgumentParser()).parse_args([]))
    assert not any(k in none for k in over)                                           # not given: not in the namespace at all
    assert not any(k in make_config("1")["init_frame"] for k in ("image_fit", "border", "cap", "coord_negate_z"))   # shipped: absent


def test_absent_option_is_none_and_defaults():
    from captra_amd.configs import make_config
    from captra_amd import track_options
    assert track_options.image_fit_cfg(make_config("1")) is None
    assert track_options.image_fit_cfg(_cfg(image_fit=False, border=9)) is None     # off: nothing is looked at
    assert track_options.image_fit_cfg(_cfg(image_fit=True)) == {"cap": 16384, "border": 0, "negate_z": False}
    assert track_options.image_fit_cfg(_cfg(image_fit=True, border=3, cap=3, coord_negate_z=True)) == {"cap": 3, "border": 3, "negate_z": True}


@pytest.mark.parametrize("section,word", [
    (dict(fit=True), "init_frame/fit"),
    (dict(cap=2), "init_frame/cap"), (dict(cap=16385), "init_frame/cap"), (dict(cap=0), "init_frame/cap"), (dict(cap=100.5), "init_frame/cap"),
    (dict(border=-1), "init_frame/border"), (dict(border=4), "init_frame/border"), (dict(border=1.5), "init_frame/border"),
])
def test_errors_of_the_option(section, word):
    from captra_amd import track_options
    with pytest.raises(ValueError, match=word):
        track_options.image_fit_cfg(_cfg(image_fit=True, **section))


def test_an_articulated_object_is_refused():
    from captra_amd.configs import make_config
    from captra_amd import track_options
    from captra_amd.synthetic import PHYSICAL_SETUPS
    cat, objcfg = PHYSICAL_SETUPS["drawers"][:2]
    cfg = make_config(cat, objcfg, **{"init_frame/image_fit": True})
    assert int(cfg["num_parts"]) > 1
    with pytest.raises(ValueError, match="num_parts"):
        track_options.image_fit_cfg(cfg)


def test_the_model_parses_the_option_and_asks_for_frame_0s_images():
    """The errors are the constructor's; a frame 0 without depth, mask or coordinate image is refused before anything is launched."""
    from captra_amd import synthetic as S
    from captra_amd.trainer import Trainer
    cfg = _cfg(image_fit=True, border=7)
    cfg["device"] = "cpu"
    with pytest.raises(ValueError, match="init_frame/border"):
        Trainer(cfg)
    cfg = _cfg(image_fit=True, border=2)
    cfg["device"] = "cpu"
    model = Trainer(cfg).model
    assert model.image_fit == {"cap": 16384, "border": 2, "negate_z": False} and not model.fit_init
    model.set_data(S.make_otf_trajectory(1, 1, seed=1))
    with pytest.raises(KeyError, match="coord"):
        model._initial_pose()
    model.set_data(S.make_trajectory("nocs", 1, 1, seed=1))
    with pytest.raises(KeyError, match="depth.*mask.*coord"):
        model._initial_pose()
    cfg = _cfg()
    cfg["device"] = "cpu"
    assert Trainer(cfg).model.image_fit is None


def test_trajectory_files_with_and_without_coord(tmp_path):
    from captra_amd import synthetic as S
    from captra_amd.trajectory_io import concat_frame_batches, load_trajectory_npz, save_trajectory_npz, stack_trajectories
    with_c, without = S.make_otf_trajectory(2, 2, seed=4, coord=True), S.make_otf_trajectory(2, 2, seed=4)
    for b in range(2):
        save_trajectory_npz(str(tmp_path / f"c{b}.npz"), with_c, b)
        save_trajectory_npz(str(tmp_path / f"p{b}.npz"), without, b)
    tc = [load_trajectory_npz(str(tmp_path / f"c{b}.npz")) for b in range(2)]
    tp = [load_trajectory_npz(str(tmp_path / f"p{b}.npz")) for b in range(2)]
    assert all("coord" in t and t["coord"].dtype == np.uint8 and t["coord"].shape == (480, 640, 3) for t in tc)
    assert all("coord" not in t for t in tp)
    fc, fp = stack_trajectories(tc), stack_trajectories(tp)
    assert set(fc[0]["meta"]["pre_fetched"]) == {"depth", "mask", "coord"} and set(fc[1]["meta"]["pre_fetched"]) == {"depth", "mask"}
    assert np.array_equal(fc[0]["meta"]["pre_fetched"]["coord"].numpy(), with_c[0]["meta"]["pre_fetched"]["coord"].numpy())
    assert all(set(f["meta"]["pre_fetched"]) == {"depth", "mask"} for f in fp)         # files without it load as before
    for a, b in zip(fc, fp):
        assert all(np.array_equal(a["meta"]["pre_fetched"][k].numpy(), b["meta"]["pre_fetched"][k].numpy()) for k in ("depth", "mask"))
    mixed = stack_trajectories([tc[0], tp[1]])                                          # one trajectory without it: the batch has none
    assert "coord" not in mixed[0]["meta"]["pre_fetched"]
    both = concat_frame_batches([stack_trajectories(tc[:1]), stack_trajectories(tc[1:])])
    assert np.array_equal(both[0]["meta"]["pre_fetched"]["coord"].numpy(), fc[0]["meta"]["pre_fetched"]["coord"].numpy())
    assert "coord" not in both[1]["meta"]["pre_fetched"]


def test_coord_default_is_the_shipped_trajectory():
    from captra_amd import synthetic as S
    assert _digest(S.make_otf_trajectory(2, 2, seed=1)) == SHIPPED_DIGEST
    assert _digest(S.make_otf_trajectory(2, 2, seed=1, coord=False)) == SHIPPED_DIGEST
    frames = S.make_otf_trajectory(2, 2, seed=1, coord=True)
    coord = frames[0]["meta"]["pre_fetched"].pop("coord")
    assert "coord" not in frames[1]["meta"]["pre_fetched"]                             # frame 0 alone carries it
    assert _digest(frames) == SHIPPED_DIGEST                                            # ... and nothing else moved
    coord = coord.numpy()
    mask = frames[0]["meta"]["pre_fetched"]["mask"].numpy()
    assert coord.dtype == np.uint8 and coord.shape == (2, 480, 640, 3)
    assert not coord[~mask].any() and coord[mask].any()


def test_rendered_coord_image_decodes_to_the_pose():
    """render_coord_image against its definition on a few pixels: NOCS = R^T (p - t) / s, round((nocs + 0.5) 255)."""
    from captra_amd import synthetic as S
    from tests import image_fit_judge as IJ
    depth, mask, _, pose = S.make_frame(5)
    img = S.render_coord_image(depth, mask, pose)
    rows, cols = np.nonzero(mask & (depth > 0))
    sel = np.arange(0, len(rows), 97)
    p = IJ.backproject(rows[sel], cols[sel], depth[rows[sel], cols[sel]].astype(np.int64), depth.shape[0], IJ.kinv_of(IJ.NOCS_INTRINSICS["real"]))
    nocs = (p - pose["translation"].reshape(3)) @ pose["rotation"] / float(pose["scale"])
    want = np.clip(np.round((nocs + 0.5) * 255.0), 0, 255)
    assert np.abs(img[rows[sel], cols[sel]].astype(np.float64) - want).max() <= 1       # (a value at .5 may round either way)
    inner = (want > 0) & (want < 255)                                                   # (not clipped)
    assert (np.abs(IJ.decode(img[rows[sel], cols[sel]]) - nocs)[inner] <= 0.5 / 255 + 1e-12).all() and inner.mean() > 0.9


def test_eval_lists_the_image_fit():
    from captra_amd.eval import image_fit_table
    data = {"image_fit": {"members": np.int32(24950), "used": np.int32(12475), "holes": np.int32(301), "inliers": np.int32(12475), "valid": np.int32(1)}}
    assert image_fit_table("inst1_track0", data) == ["inst1_track0: members 24950; used 12475; holes 301; inliers 12475; valid yes"]
    data["image_fit"]["valid"] = np.int32(0)
    assert image_fit_table("x", data)[0].endswith("valid no")


def test_binding_row_matches_the_header():
    """Argument count and pointer places of the row against the declaration (stream included)."""
    import re
    from pathlib import Path
    from captra_amd import _lib
    text = (Path(__file__).resolve().parent.parent / "include" / "captra_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"\bcaptra_image_members\s*\(([^;]*?)\)\s*;", text, flags=re.S).group(1)
    params = [p.strip() for p in decl.split(",")]
    sig = _lib._SIGNATURES["captra_image_members"]
    assert len(sig) == len(params) == 16
    for p, t in zip(params, sig):
        assert ("*" in p or "captra_stream_t" in p) == (t is _lib._P), p


def test_wrapper_refuses_cpu_tensors_and_bad_arguments():
    import torch
    from captra_amd.nocs_otf import check_image_fit_params, image_members
    d, m, c = torch.zeros(2, 4, 4, dtype=torch.int32), torch.ones(2, 4, 4, dtype=torch.bool), torch.zeros(2, 4, 4, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        image_members(d, m, c)
    assert check_image_fit_params(16384, 3) == (16384, 3) and check_image_fit_params(3, 0) == (3, 0)
    for cap, border, word in ((2, 0, "cap"), (16385, 0, "cap"), (64, 4, "border"), (64, -1, "border"), (True, 0, "cap")):
        with pytest.raises(ValueError, match=word):
            check_image_fit_params(cap, border)
