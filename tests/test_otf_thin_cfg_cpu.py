"""The configuration surface of track_cfg/otf_thin (the re-crop's lists thinned on the device): the flags, the shipped default,
track_options.otf_thin_cfg, the table of captra_amd.eval, the binding rows, and synthetic's blob_px (default = the shipped frames)."""
import argparse

import numpy as np
import pytest


def test_parse_args_builds_the_otf_thin_cfg():
    from captra_amd.configs import make_config
    from captra_amd.parse_args import add_args
    args = add_args(argparse.ArgumentParser()).parse_args(["--track_cfg/otf_thin/device", "True", "--track_cfg/otf_thin/seed", "11"])
    over = {k: v for k, v in vars(args).items() if k.startswith("track_cfg/otf_thin/")}
    assert over == {"track_cfg/otf_thin/device": True, "track_cfg/otf_thin/seed": 11}
    assert make_config("1", **over)["track_cfg"]["otf_thin"] == {"device": True, "seed": 11}
    none = add_args(argparse.ArgumentParser()).parse_args([])
    assert all(v is None for k, v in vars(none).items() if k.startswith("track_cfg/otf_thin/"))
    assert make_config("1")["track_cfg"]["otf_thin"] == {"device": False, "seed": 0}          # shipped: off


def test_otf_thin_cfg_defaults_and_errors():
    from captra_amd.configs import make_config
    from captra_amd import track_options
    assert track_options.otf_thin_cfg(make_config("1")) is None
    assert track_options.otf_thin_cfg(make_config("1", **{"track_cfg/otf_thin/seed": 5})) is None
    assert track_options.otf_thin_cfg(make_config("1", **{"track_cfg/otf_thin/device": True})) == {"seed": 0}
    assert track_options.otf_thin_cfg(make_config("1", **{"track_cfg/otf_thin/device": True, "track_cfg/otf_thin/seed": 5})) == {"seed": 5}
    cfg = make_config("1")
    del cfg["track_cfg"]["otf_thin"]
    assert track_options.otf_thin_cfg(cfg) is None
    with pytest.raises(ValueError, match="seed"):
        track_options.otf_thin_cfg(make_config("1", **{"track_cfg/otf_thin/device": True, "track_cfg/otf_thin/seed": -1}))


def test_eval_lists_the_frames_thinned():
    from captra_amd.eval import otf_thin_table
    data = {"otf_thin": [None] + [{"thinned": np.array([t], np.int32)} for t in (1, 0, 1, 1)]}
    assert otf_thin_table("inst1_track0", data) == ["inst1_track0: thinned 3 / 4 frames"]
    assert otf_thin_table("x", {"otf_thin": [None]}) == ["x: thinned 0 / 0 frames"]


def test_binding_rows_match_the_header():
    """Argument counts of the three rows against the declarations (stream included)."""
    import re
    from pathlib import Path
    from captra_amd import _lib
    text = (Path(__file__).resolve().parent.parent / "include" / "captra_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("captra_otf_thin", "captra_otf_candidates_thin", "captra_otf_finish_thin"):
        decl = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S).group(1)
        params = [p.strip() for p in decl.split(",")]
        sig = _lib._SIGNATURES[name]
        assert len(sig) == len(params), name
        for p, t in zip(params, sig):
            assert ("*" in p or "captra_stream_t" in p) == (t is _lib._P), (name, p)


def test_blob_px_default_is_the_shipped_frame():
    from captra_amd.synthetic import make_frame
    a, b, c = make_frame(3, dr=4.0, dc=9.0), make_frame(3, dr=4.0, dc=9.0, blob_px=70), make_frame(3, dr=4.0, dc=9.0, blob_px=90)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert int(c[1].sum()) > int(a[1].sum()) * 1.5
