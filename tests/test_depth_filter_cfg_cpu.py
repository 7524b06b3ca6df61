"""The configuration surface of track_cfg/depth_filter (flying depth pixels removed from every uploaded depth image): the flags,
track_options.depth_filter_cfg and every error it raises, the table of captra_amd.eval, the binding row, and synthetic's `flying`
(default = the shipped frames)."""
import argparse

import numpy as np
import pytest

KEYS = ("window", "abs_mm", "rel_permille", "min_support")


def _cfg(nocs_otf=True, **section):
    from captra_amd.configs import make_config
    return make_config("1", nocs_otf=nocs_otf, **{f"track_cfg/depth_filter/{k}": v for k, v in section.items()})


def test_parse_args_builds_the_depth_filter_cfg():
    from captra_amd.configs import make_config
    from captra_amd.parse_args import add_args
    argv = ["--track_cfg/depth_filter/window", "3", "--track_cfg/depth_filter/abs_mm", "10", "--track_cfg/depth_filter/rel_permille", "5",
            "--track_cfg/depth_filter/min_support", "12"]
    args = add_args(argparse.ArgumentParser()).parse_args(argv)
    over = {k: v for k, v in vars(args).items() if k.startswith("track_cfg/depth_filter/")}
    assert over == {"track_cfg/depth_filter/window": 3, "track_cfg/depth_filter/abs_mm": 10, "track_cfg/depth_filter/rel_permille": 5,
                    "track_cfg/depth_filter/min_support": 12}
    assert make_config("1", **over)["track_cfg"]["depth_filter"] == {"window": 3, "abs_mm": 10, "rel_permille": 5, "min_support": 12}
    none = add_args(argparse.ArgumentParser()).parse_args([])
    assert all(v is None for k, v in vars(none).items() if k.startswith("track_cfg/depth_filter/"))
    assert "depth_filter" not in make_config("1")["track_cfg"]                         # shipped: absent


def test_absent_option_is_none():
    from captra_amd.configs import make_config
    from captra_amd import track_options
    assert track_options.depth_filter_cfg(make_config("1")) is None
    assert track_options.depth_filter_cfg(make_config("1", nocs_otf=True)) is None
    cfg = make_config("1", nocs_otf=True)
    cfg["track_cfg"]["depth_filter"] = None
    assert track_options.depth_filter_cfg(cfg) is None


def test_defaults_and_parsed_values():
    from captra_amd import track_options
    assert track_options.depth_filter_cfg(_cfg(abs_mm=10, min_support=6)) == {"window": 2, "abs_mm": 10, "rel_permille": 0, "min_support": 6}
    assert track_options.depth_filter_cfg(_cfg(window=3, abs_mm=0, rel_permille=1000, min_support=48)) == {
        "window": 3, "abs_mm": 0, "rel_permille": 1000, "min_support": 48}
    assert tuple(track_options.depth_filter_cfg(_cfg(abs_mm=10, min_support=6))) == KEYS       # the wrapper's keyword order


@pytest.mark.parametrize("section,word", [
    (dict(min_support=6), "abs_mm"),                                   # no default
    (dict(abs_mm=10), "min_support"),                                  # no default
    (dict(window=2), "abs_mm"),
    (dict(window=0, abs_mm=10, min_support=1), "window"),
    (dict(window=4, abs_mm=10, min_support=1), "window"),
    (dict(abs_mm=-1, min_support=1), "abs_mm"),
    (dict(abs_mm=10, rel_permille=-1, min_support=1), "rel_permille"),
    (dict(abs_mm=10, rel_permille=1001, min_support=1), "rel_permille"),
    (dict(abs_mm=10, min_support=0), "min_support"),
    (dict(window=1, abs_mm=10, min_support=9), "min_support"),
    (dict(window=2, abs_mm=10, min_support=25), "min_support"),
    (dict(window=3, abs_mm=10, min_support=49), "min_support"),
    (dict(abs_mm=10.5, min_support=6), "abs_mm"),
])
def test_values_outside_the_kernels_ranges_raise_at_construction(section, word):
    from captra_amd import track_options
    with pytest.raises(ValueError, match="track_cfg/depth_filter.*" + word):
        track_options.depth_filter_cfg(_cfg(**section))


def test_the_option_needs_the_on_the_fly_re_crop():
    from captra_amd import track_options
    with pytest.raises(ValueError, match="nocs_otf"):
        track_options.depth_filter_cfg(_cfg(nocs_otf=False, abs_mm=10, min_support=6))


def test_the_model_parses_the_option_when_it_is_built():
    """The errors are the constructor's, and the parsed option is the model's attribute."""
    from captra_amd.trainer import Trainer
    cfg = _cfg(abs_mm=10)
    cfg["device"] = "cpu"
    with pytest.raises(ValueError, match="min_support"):
        Trainer(cfg)
    cfg = _cfg(window=3, abs_mm=10, min_support=12)
    cfg["device"] = "cpu"
    assert Trainer(cfg).model.depth_filter == {"window": 3, "abs_mm": 10, "rel_permille": 0, "min_support": 12}
    cfg = _cfg()
    cfg["device"] = "cpu"
    assert Trainer(cfg).model.depth_filter is None


def test_eval_lists_the_pixels_removed():
    from captra_amd.eval import depth_filter_table
    data = {"depth_filter": [{"removed": np.int32(r)} for r in (640, 0, 700)] + [None]}
    assert depth_filter_table("inst1_track0", data) == ["inst1_track0: removed 1340 pixels in 3 frames (mean 446.7, max 700 per frame)"]
    assert depth_filter_table("x", {"depth_filter": [None, None]}) == ["x: removed 0 pixels in 0 frames"]


def test_binding_row_matches_the_header():
    """Argument count and pointer places of the row against the declaration (stream included)."""
    import re
    from pathlib import Path
    from captra_amd import _lib
    text = (Path(__file__).resolve().parent.parent / "include" / "captra_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"\bcaptra_depth_support_filter\s*\(([^;]*?)\)\s*;", text, flags=re.S).group(1)
    params = [p.strip() for p in decl.split(",")]
    sig = _lib._SIGNATURES["captra_depth_support_filter"]
    assert len(sig) == len(params) == 11
    for p, t in zip(params, sig):
        assert ("*" in p or "captra_stream_t" in p) == (t is _lib._P), p


def test_wrapper_refuses_cpu_tensors_and_bad_arguments():
    import torch
    from captra_amd.nocs_otf import check_depth_filter_params, depth_support_filter
    with pytest.raises(RuntimeError):
        depth_support_filter(torch.zeros(2, 4, 4, dtype=torch.int32), 1, 0, 0, 1)
    assert check_depth_filter_params(2, 10, 0, 24) == (2, 10, 0, 24)
    with pytest.raises(ValueError, match="min_support"):
        check_depth_filter_params(2, 10, 0, 25)


def test_flying_default_is_the_shipped_frame():
    from captra_amd.synthetic import make_frame, make_otf_trajectory
    a, b = make_frame(3, dr=4.0, dc=9.0, blob_px=90), make_frame(3, dr=4.0, dc=9.0, blob_px=90, flying=0.0)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert a[2].tobytes() == b[2].tobytes() and all(np.array_equal(a[3][k], b[3][k]) for k in a[3]) and len(b) == 4
    c = make_frame(3, dr=4.0, dc=9.0, blob_px=90, flying=0.0, return_flying=True)
    assert len(c) == 5 and c[0].tobytes() == a[0].tobytes() and c[4].dtype == bool and not c[4].any()
    f = make_frame(3, dr=4.0, dc=9.0, blob_px=90, flying=0.5, return_flying=True)
    assert f[1].tobytes() == a[1].tobytes() and f[2].tobytes() == a[2].tobytes()      # the frame's own stream did not move
    changed = f[0] != a[0]
    assert changed.any() and not (changed & ~f[4]).any()                               # only injected pixels differ
    assert f[0][f[4]].min() >= 975 and f[0][f[4]].max() <= 1130 and (a[0][f[4]] > 0).all()
    plain, fly = make_otf_trajectory(2, 2, seed=1), make_otf_trajectory(2, 2, seed=1, flying=0.5)
    assert set(plain[1]["meta"]["pre_fetched"]) == {"depth", "mask"} and set(fly[1]["meta"]["pre_fetched"]) == {"depth", "mask", "flying"}
    same = make_otf_trajectory(2, 2, seed=1, flying=0.0)
    assert all(np.array_equal(p["meta"]["pre_fetched"][k], s["meta"]["pre_fetched"][k]) for p, s in zip(plain, same) for k in ("depth", "mask"))
    inj = fly[1]["meta"]["pre_fetched"]["flying"]
    assert inj.dtype == np.bool_ or str(inj.dtype) == "torch.bool"
    assert tuple(inj.shape) == (2, 480, 640) and int(inj.sum()) > 800
