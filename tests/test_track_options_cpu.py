"""The track loop's opt-in features as the configuration sees them: what each parser returns -- key order included -- or raises for a
table of configs (the literals below were recorded from the parsers as they stood as static methods of EvalTrackModel), the model
attributes they fill, the layout of the records in the result pickles, and the one wrapper that takes the per-step records out of
CoordinateNet's maps."""
import numpy as np
import pytest
import torch

from captra_amd import track_options as _M

PARSERS = {"guard": _M.guard_cfg, "st_fit": _M.st_fit_cfg, "rot_pool": _M.rot_pool_cfg, "otf_thin": _M.otf_thin_cfg,
           "depth_filter": _M.depth_filter_cfg, "image_fit": _M.image_fit_cfg,
           "init_yaxis": lambda cfg: _M.yaxis_only(cfg, cfg["init_frame"], "init_frame/yaxis_only")}

G, S, R, T, D, I = "track_cfg/guard/", "track_cfg/st_fit/", "track_cfg/rot_pool/", "track_cfg/otf_thin/", "track_cfg/depth_filter/", "init_frame/"
INIT = {"init_frame/num_hyps": 48, "init_frame/seed": 9}
S_ON, R_ON, T_ON = {S + "ransac": True}, {R + "consensus": True, R + "angle_th": 15.0}, {T + "device": True}
D_ON, I_ON = {"nocs_otf": True, D + "abs_mm": 10, D + "min_support": 6}, {"nocs_otf": True, I + "image_fit": True}
NAN = float("nan")


def _d(base, **section):
    """`base` with the depth filter's keys replaced by `section` (nocs_otf stays)."""
    return {"nocs_otf": base["nocs_otf"], **{D + k: v for k, v in section.items()}}


# (parser, case, overrides for make_config ["cat" / "obj_config": the object], values put into the finished cfg by path -- an explicit None
# cannot come through make_config)
CASES = [
    ("guard", "absent", {}, {}),
    ("guard", "section_none", {}, {("track_cfg", "guard"): None}),
    ("guard", "no_lost_below", {G + "refit": True, G + "num_hyps": 32}, {}),
    ("guard", "lost_below_none", {G + "refit": True}, {("track_cfg", "guard", "lost_below"): None}),
    ("guard", "defaults", {G + "lost_below": 0.5}, {}),
    ("guard", "every_key", {G + "refit": True, G + "lost_below": 0.25, G + "inlier_th": 0.01, G + "min_members": 6, G + "num_hyps": 32,
                            G + "seed": 3, G + "yaxis_only": True}, {}),
    ("guard", "init_frames_draws", {G + "lost_below": 0.5, **INIT}, {}),
    ("guard", "own_draws_over_init_frames", {G + "lost_below": 0.5, G + "num_hyps": 16, G + "seed": 2, **INIT}, {}),
    ("guard", "num_hyps_0", {G + "lost_below": 0.5, G + "num_hyps": 0}, {}),                # (no range check on the guard's draws)
    ("guard", "num_hyps_257", {G + "lost_below": 0.5, G + "num_hyps": 257}, {}),
    ("guard", "seed_negative", {G + "lost_below": 0.5, G + "seed": -1}, {}),
    ("guard", "num_hyps_none", {G + "lost_below": 0.5}, {("track_cfg", "guard", "num_hyps"): None}),
    ("guard", "lost_below_above_1", {G + "lost_below": 1.5}, {}),
    ("guard", "lost_below_negative", {G + "lost_below": -0.1}, {}),
    ("guard", "yaxis_only_false", {G + "lost_below": 0.5, G + "yaxis_only": False}, {}),
    ("guard", "yaxis_only_not_symmetric", {"cat": "6", G + "lost_below": 0.5, G + "yaxis_only": True}, {}),
    ("st_fit", "absent", {}, {}),
    ("st_fit", "section_none", {}, {("track_cfg", "st_fit"): None}),
    ("st_fit", "off_with_keys", {S + "ransac": False, S + "num_hyps": 0, S + "inlier_th": -1.0, S + "seed": -1}, {}),
    ("st_fit", "no_switch_with_keys", {S + "num_hyps": 0}, {}),
    ("st_fit", "defaults", S_ON, {}),
    ("st_fit", "every_key", {**S_ON, S + "inlier_th": 0.01, S + "num_hyps": 32, S + "seed": 3}, {}),
    ("st_fit", "init_frames_draws", {**S_ON, **INIT}, {}),
    ("st_fit", "own_draws_over_init_frames", {**S_ON, S + "num_hyps": 16, S + "seed": 2, **INIT}, {}),
    ("st_fit", "keys_none", S_ON, {("track_cfg", "st_fit", k): None for k in ("inlier_th", "num_hyps", "seed")}),
    ("st_fit", "inlier_th_0", {**S_ON, S + "inlier_th": 0.0}, {}),
    ("st_fit", "inlier_th_negative", {**S_ON, S + "inlier_th": -0.01}, {}),
    ("st_fit", "inlier_th_nan", {**S_ON, S + "inlier_th": NAN}, {}),
    ("st_fit", "num_hyps_0", {**S_ON, S + "num_hyps": 0}, {}),
    ("st_fit", "num_hyps_negative", {**S_ON, S + "num_hyps": -4}, {}),
    ("st_fit", "num_hyps_257", {**S_ON, S + "num_hyps": 257}, {}),
    ("st_fit", "num_hyps_256", {**S_ON, S + "num_hyps": 256}, {}),
    ("st_fit", "seed_negative", {**S_ON, S + "seed": -1}, {}),
    ("st_fit", "init_frames_num_hyps_0", {**S_ON, "init_frame/num_hyps": 0}, {}),
    ("rot_pool", "absent", {}, {}),
    ("rot_pool", "section_none", {}, {("track_cfg", "rot_pool"): None}),
    ("rot_pool", "off_with_keys", {R + "consensus": False, R + "num_hyps": 0, R + "angle_th": 500.0}, {}),
    ("rot_pool", "no_switch_with_keys", {R + "angle_th": 15.0}, {}),
    ("rot_pool", "no_angle_th", {R + "consensus": True, R + "num_hyps": 0}, {}),
    ("rot_pool", "defaults", R_ON, {}),
    ("rot_pool", "every_key", {**R_ON, R + "angle_th": 20, R + "num_hyps": 32, R + "seed": 3}, {}),
    ("rot_pool", "init_frames_draws", {**R_ON, **INIT}, {}),
    ("rot_pool", "own_draws_over_init_frames", {**R_ON, R + "num_hyps": 16, R + "seed": 2, **INIT}, {}),
    ("rot_pool", "draws_none", R_ON, {("track_cfg", "rot_pool", k): None for k in ("num_hyps", "seed")}),
    ("rot_pool", "angle_th_0", {**R_ON, R + "angle_th": 0.0}, {}),
    ("rot_pool", "angle_th_negative", {**R_ON, R + "angle_th": -5.0}, {}),
    ("rot_pool", "angle_th_180", {**R_ON, R + "angle_th": 180.0}, {}),
    ("rot_pool", "angle_th_nan", {**R_ON, R + "angle_th": NAN}, {}),
    ("rot_pool", "num_hyps_0", {**R_ON, R + "num_hyps": 0}, {}),
    ("rot_pool", "num_hyps_257", {**R_ON, R + "num_hyps": 257}, {}),
    ("rot_pool", "seed_negative", {**R_ON, R + "seed": -1}, {}),
    ("rot_pool", "angle_before_draws", {**R_ON, R + "angle_th": 0.0, R + "num_hyps": 0, R + "seed": -1}, {}),
    ("otf_thin", "shipped", {}, {}),
    ("otf_thin", "absent", {}, {("track_cfg",): {"gt_label": False, "nocs2d_label": False}}),
    ("otf_thin", "section_none", {}, {("track_cfg", "otf_thin"): None}),
    ("otf_thin", "off_with_seed", {T + "device": False, T + "seed": -5}, {}),
    ("otf_thin", "no_switch_with_seed", {}, {("track_cfg", "otf_thin"): {"seed": 5}}),
    ("otf_thin", "defaults", T_ON, {}),
    ("otf_thin", "every_key", {**T_ON, T + "seed": 5}, {}),
    ("otf_thin", "no_seed_key", {}, {("track_cfg", "otf_thin"): {"device": True}}),
    ("otf_thin", "seed_none", T_ON, {("track_cfg", "otf_thin", "seed"): None}),
    ("otf_thin", "not_init_frames_seed", {}, {("track_cfg", "otf_thin"): {"device": True}, ("init_frame", "seed"): 9}),
    ("otf_thin", "seed_negative", {**T_ON, T + "seed": -1}, {}),
    ("depth_filter", "absent", {}, {}),
    ("depth_filter", "absent_with_otf", {"nocs_otf": True}, {}),
    ("depth_filter", "section_none", {"nocs_otf": True}, {("track_cfg", "depth_filter"): None}),
    ("depth_filter", "defaults", D_ON, {}),
    ("depth_filter", "every_key", _d(D_ON, window=3, abs_mm=0, rel_permille=1000, min_support=48), {}),
    ("depth_filter", "keys_none", D_ON, {("track_cfg", "depth_filter", k): None for k in ("window", "rel_permille")}),
    ("depth_filter", "without_otf", {**D_ON, "nocs_otf": False}, {}),
    ("depth_filter", "no_abs_mm", _d(D_ON, min_support=6), {}),
    ("depth_filter", "no_min_support", _d(D_ON, abs_mm=10), {}),
    ("depth_filter", "neither", _d(D_ON, window=2), {}),
    ("depth_filter", "window_0", _d(D_ON, window=0, abs_mm=10, min_support=1), {}),
    ("depth_filter", "window_4", _d(D_ON, window=4, abs_mm=10, min_support=1), {}),
    ("depth_filter", "abs_mm_negative", _d(D_ON, abs_mm=-1, min_support=1), {}),
    ("depth_filter", "rel_negative", _d(D_ON, abs_mm=10, rel_permille=-1, min_support=1), {}),
    ("depth_filter", "rel_1001", _d(D_ON, abs_mm=10, rel_permille=1001, min_support=1), {}),
    ("depth_filter", "min_support_0", _d(D_ON, abs_mm=10, min_support=0), {}),
    ("depth_filter", "min_support_window_1", _d(D_ON, window=1, abs_mm=10, min_support=9), {}),
    ("depth_filter", "min_support_window_2", _d(D_ON, window=2, abs_mm=10, min_support=25), {}),
    ("depth_filter", "min_support_window_3", _d(D_ON, window=3, abs_mm=10, min_support=49), {}),
    ("depth_filter", "abs_mm_fraction", _d(D_ON, abs_mm=10.5, min_support=6), {}),
    ("image_fit", "absent", {}, {}),
    ("image_fit", "off_with_keys", {"nocs_otf": True, I + "image_fit": False, I + "border": 9, I + "cap": 0, I + "fit": True}, {}),
    ("image_fit", "defaults", I_ON, {}),
    ("image_fit", "every_key", {**I_ON, I + "border": 3, I + "cap": 3, I + "coord_negate_z": True}, {}),
    ("image_fit", "keys_none", I_ON, {("init_frame", k): None for k in ("cap", "border")}),
    ("image_fit", "with_fit", {**I_ON, I + "fit": True}, {}),
    ("image_fit", "articulated", {"cat": "drawers", "obj_config": "obj_info_sapien.yml", I + "image_fit": True}, {}),
    ("image_fit", "cap_2", {**I_ON, I + "cap": 2}, {}),
    ("image_fit", "cap_16385", {**I_ON, I + "cap": 16385}, {}),
    ("image_fit", "cap_0", {**I_ON, I + "cap": 0}, {}),
    ("image_fit", "cap_fraction", {**I_ON, I + "cap": 100.5}, {}),
    ("image_fit", "border_negative", {**I_ON, I + "border": -1}, {}),
    ("image_fit", "border_4", {**I_ON, I + "border": 4}, {}),
    ("image_fit", "border_fraction", {**I_ON, I + "border": 1.5}, {}),
    ("init_yaxis", "absent", {}, {}),
    ("init_yaxis", "on", {I + "yaxis_only": True}, {}),
    ("init_yaxis", "off", {I + "yaxis_only": False}, {}),
    ("init_yaxis", "not_symmetric", {"cat": "6", I + "yaxis_only": True}, {}),
    ("init_yaxis", "off_not_symmetric", {"cat": "6", I + "yaxis_only": False}, {}),
]

EXPECTED = {
    "guard/absent": None,
    "guard/section_none": None,
    "guard/no_lost_below": ("ValueError", "track_cfg/guard needs lost_below (the inlier fraction below which a part counts as lost): it has no default"),
    "guard/lost_below_none": ("ValueError", "track_cfg/guard needs lost_below (the inlier fraction below which a part counts as lost): it has no default"),
    "guard/defaults": [("refit", False), ("lost_below", (1, 2)), ("inlier_th", 0.003), ("min_members", 4), ("num_hyps", 64), ("seed", 0)],
    "guard/every_key": [("refit", True), ("lost_below", (1, 4)), ("inlier_th", 0.006), ("min_members", 6), ("num_hyps", 32), ("seed", 3),
                        ("yaxis_only", True)],
    "guard/init_frames_draws": [("refit", False), ("lost_below", (1, 2)), ("inlier_th", 0.003), ("min_members", 4), ("num_hyps", 48), ("seed", 9)],
    "guard/own_draws_over_init_frames": [("refit", False), ("lost_below", (1, 2)), ("inlier_th", 0.003), ("min_members", 4), ("num_hyps", 16),
                                         ("seed", 2)],
    "guard/num_hyps_0": [("refit", False), ("lost_below", (1, 2)), ("inlier_th", 0.003), ("min_members", 4), ("num_hyps", 0), ("seed", 0)],
    "guard/num_hyps_257": [("refit", False), ("lost_below", (1, 2)), ("inlier_th", 0.003), ("min_members", 4), ("num_hyps", 257), ("seed", 0)],
    "guard/seed_negative": [("refit", False), ("lost_below", (1, 2)), ("inlier_th", 0.003), ("min_members", 4), ("num_hyps", 64), ("seed", -1)],
    "guard/num_hyps_none": ("TypeError", None),
    "guard/lost_below_above_1": ("ValueError", "lost_below must be a fraction in [0, 1], got 1.5"),
    "guard/lost_below_negative": ("ValueError", "lost_below must be a fraction in [0, 1], got -0.1"),
    "guard/yaxis_only_false": [("refit", False), ("lost_below", (1, 2)), ("inlier_th", 0.003), ("min_members", 4), ("num_hyps", 64), ("seed", 0)],
    "guard/yaxis_only_not_symmetric": ("ValueError", "track_cfg/guard/yaxis_only: the axis-only inlier test is for symmetric categories (obj_sym), "
                                                     "category 6 is not one: its in-plane angle is part of the pose"),
    "st_fit/absent": None,
    "st_fit/section_none": None,
    "st_fit/off_with_keys": None,
    "st_fit/no_switch_with_keys": None,
    "st_fit/defaults": [("inlier_th", 0.003), ("num_hyps", 64), ("seed", 0)],
    "st_fit/every_key": [("inlier_th", 0.006), ("num_hyps", 32), ("seed", 3)],
    "st_fit/init_frames_draws": [("inlier_th", 0.003), ("num_hyps", 48), ("seed", 9)],
    "st_fit/own_draws_over_init_frames": [("inlier_th", 0.003), ("num_hyps", 16), ("seed", 2)],
    "st_fit/keys_none": [("inlier_th", 0.003), ("num_hyps", 64), ("seed", 0)],
    "st_fit/inlier_th_0": ("ValueError", "track_cfg/st_fit/inlier_th must be a positive fraction of data_radius, got 0.0"),
    "st_fit/inlier_th_negative": ("ValueError", "track_cfg/st_fit/inlier_th must be a positive fraction of data_radius, got -0.01"),
    "st_fit/inlier_th_nan": ("ValueError", "track_cfg/st_fit/inlier_th must be a positive fraction of data_radius, got nan"),
    "st_fit/num_hyps_0": ("ValueError", "track_cfg/st_fit/num_hyps must be in [1, 256] (the kernel's limit), got 0"),
    "st_fit/num_hyps_negative": ("ValueError", "track_cfg/st_fit/num_hyps must be in [1, 256] (the kernel's limit), got -4"),
    "st_fit/num_hyps_257": ("ValueError", "track_cfg/st_fit/num_hyps must be in [1, 256] (the kernel's limit), got 257"),
    "st_fit/num_hyps_256": [("inlier_th", 0.003), ("num_hyps", 256), ("seed", 0)],
    "st_fit/seed_negative": ("ValueError", "track_cfg/st_fit/seed must not be negative, got -1"),
    "st_fit/init_frames_num_hyps_0": ("ValueError", "track_cfg/st_fit/num_hyps must be in [1, 256] (the kernel's limit), got 0"),
    "rot_pool/absent": None,
    "rot_pool/section_none": None,
    "rot_pool/off_with_keys": None,
    "rot_pool/no_switch_with_keys": None,
    "rot_pool/no_angle_th": ("ValueError", "track_cfg/rot_pool/consensus needs track_cfg/rot_pool/angle_th (degrees, inside (0, 180)): it has no default"),
    "rot_pool/defaults": [("angle_th", 15.0), ("num_hyps", 64), ("seed", 0)],
    "rot_pool/every_key": [("angle_th", 20.0), ("num_hyps", 32), ("seed", 3)],
    "rot_pool/init_frames_draws": [("angle_th", 15.0), ("num_hyps", 48), ("seed", 9)],
    "rot_pool/own_draws_over_init_frames": [("angle_th", 15.0), ("num_hyps", 16), ("seed", 2)],
    "rot_pool/draws_none": [("angle_th", 15.0), ("num_hyps", 64), ("seed", 0)],
    "rot_pool/angle_th_0": ("ValueError", "track_cfg/rot_pool/angle_th must be an angle in degrees inside (0, 180), got 0.0"),
    "rot_pool/angle_th_negative": ("ValueError", "track_cfg/rot_pool/angle_th must be an angle in degrees inside (0, 180), got -5.0"),
    "rot_pool/angle_th_180": ("ValueError", "track_cfg/rot_pool/angle_th must be an angle in degrees inside (0, 180), got 180.0"),
    "rot_pool/angle_th_nan": ("ValueError", "track_cfg/rot_pool/angle_th must be an angle in degrees inside (0, 180), got nan"),
    "rot_pool/num_hyps_0": ("ValueError", "track_cfg/rot_pool/num_hyps must be in [1, 256] (the kernel's limit), got 0"),
    "rot_pool/num_hyps_257": ("ValueError", "track_cfg/rot_pool/num_hyps must be in [1, 256] (the kernel's limit), got 257"),
    "rot_pool/seed_negative": ("ValueError", "track_cfg/rot_pool/seed must not be negative, got -1"),
    "rot_pool/angle_before_draws": ("ValueError", "track_cfg/rot_pool/angle_th must be an angle in degrees inside (0, 180), got 0.0"),
    "otf_thin/shipped": None,
    "otf_thin/absent": None,
    "otf_thin/section_none": None,
    "otf_thin/off_with_seed": None,
    "otf_thin/no_switch_with_seed": None,
    "otf_thin/defaults": [("seed", 0)],
    "otf_thin/every_key": [("seed", 5)],
    "otf_thin/no_seed_key": [("seed", 0)],
    "otf_thin/seed_none": [("seed", 0)],
    "otf_thin/not_init_frames_seed": [("seed", 0)],
    "otf_thin/seed_negative": ("ValueError", "track_cfg/otf_thin/seed must not be negative, got -1"),
    "depth_filter/absent": None,
    "depth_filter/absent_with_otf": None,
    "depth_filter/section_none": None,
    "depth_filter/defaults": [("window", 2), ("abs_mm", 10), ("rel_permille", 0), ("min_support", 6)],
    "depth_filter/every_key": [("window", 3), ("abs_mm", 0), ("rel_permille", 1000), ("min_support", 48)],
    "depth_filter/keys_none": [("window", 2), ("abs_mm", 10), ("rel_permille", 0), ("min_support", 6)],
    "depth_filter/without_otf": ("ValueError", "track_cfg/depth_filter filters the depth images the on-the-fly re-crop reads: it needs nocs_otf: True "
                                               "(without it there is no depth image)"),
    "depth_filter/no_abs_mm": ("ValueError", "track_cfg/depth_filter needs track_cfg/depth_filter/abs_mm: it has no default"),
    "depth_filter/no_min_support": ("ValueError", "track_cfg/depth_filter needs track_cfg/depth_filter/min_support: it has no default"),
    "depth_filter/neither": ("ValueError", "track_cfg/depth_filter needs track_cfg/depth_filter/abs_mm: it has no default"),
    "depth_filter/window_0": ("ValueError", "track_cfg/depth_filter/window must be 1, 2 or 3 (a square of 3, 5 or 7 pixels), got 0"),
    "depth_filter/window_4": ("ValueError", "track_cfg/depth_filter/window must be 1, 2 or 3 (a square of 3, 5 or 7 pixels), got 4"),
    "depth_filter/abs_mm_negative": ("ValueError", "track_cfg/depth_filter/abs_mm (millimetres) must be in [0, 2^31 - 1], got -1"),
    "depth_filter/rel_negative": ("ValueError", "track_cfg/depth_filter/rel_permille must be in [0, 1000], got -1"),
    "depth_filter/rel_1001": ("ValueError", "track_cfg/depth_filter/rel_permille must be in [0, 1000], got 1001"),
    "depth_filter/min_support_0": ("ValueError", "track_cfg/depth_filter/min_support must be in [1, 24] (the other pixels of a window of 2), got 0"),
    "depth_filter/min_support_window_1": ("ValueError", "track_cfg/depth_filter/min_support must be in [1, 8] (the other pixels of a window of 1), got 9"),
    "depth_filter/min_support_window_2": ("ValueError", "track_cfg/depth_filter/min_support must be in [1, 24] (the other pixels of a window of 2), got 25"),
    "depth_filter/min_support_window_3": ("ValueError", "track_cfg/depth_filter/min_support must be in [1, 48] (the other pixels of a window of 3), got 49"),
    "depth_filter/abs_mm_fraction": ("ValueError", "track_cfg/depth_filter/abs_mm must be an integer, got 10.5"),
    "image_fit/absent": None,
    "image_fit/off_with_keys": None,
    "image_fit/defaults": [("cap", 16384), ("border", 0), ("negate_z", False)],
    "image_fit/every_key": [("cap", 3), ("border", 3), ("negate_z", True)],
    "image_fit/keys_none": [("cap", 16384), ("border", 0), ("negate_z", False)],
    "image_fit/with_fit": ("ValueError", "init_frame/image_fit and init_frame/fit both fit the first pose, one from frame 0's images and one from its "
                                         "pre-cropped cloud: set one of them"),
    "image_fit/articulated": ("ValueError", "init_frame/image_fit fits one rigid object (a coordinate image describes one), this object has "
                                            "num_parts = 4"),
    "image_fit/cap_2": ("ValueError", "init_frame/cap must be in [3, 16384] (a fit needs three members, the fit kernel takes 16384), got 2"),
    "image_fit/cap_16385": ("ValueError", "init_frame/cap must be in [3, 16384] (a fit needs three members, the fit kernel takes 16384), got 16385"),
    "image_fit/cap_0": ("ValueError", "init_frame/cap must be in [3, 16384] (a fit needs three members, the fit kernel takes 16384), got 0"),
    "image_fit/cap_fraction": ("ValueError", "init_frame/cap must be an integer, got 100.5"),
    "image_fit/border_negative": ("ValueError", "init_frame/border must be in [0, 3] (pixels eroded from the mask), got -1"),
    "image_fit/border_4": ("ValueError", "init_frame/border must be in [0, 3] (pixels eroded from the mask), got 4"),
    "image_fit/border_fraction": ("ValueError", "init_frame/border must be an integer, got 1.5"),
    "init_yaxis/absent": False,
    "init_yaxis/on": True,
    "init_yaxis/off": False,
    "init_yaxis/not_symmetric": ("ValueError", "init_frame/yaxis_only: the axis-only inlier test is for symmetric categories (obj_sym), category 6 "
                                               "is not one: its in-plane angle is part of the pose"),
    "init_yaxis/off_not_symmetric": False,
}


def _make(over, put):
    from captra_amd.configs import make_config
    over = dict(over)
    args = [over.pop("cat", "1")] + ([over.pop("obj_config")] if "obj_config" in over else [])
    cfg = make_config(*args, **over)
    for path, value in put.items():
        at = cfg
        for key in path[:-1]:
            at = at[key]
        at[path[-1]] = value
    return cfg


def observe(parser, over, put):
    """What the parser does with the config: None, the returned dict as its (key, value) pairs in order, a plain value, or
    (exception type, message) -- the message None for a TypeError, whose text is the interpreter's."""
    cfg = _make(over, put)
    try:
        out = PARSERS[parser](cfg)
    except TypeError:
        return ("TypeError", None)
    except (ValueError, KeyError) as e:
        return (type(e).__name__, str(e))
    return list(out.items()) if isinstance(out, dict) else out


def test_the_table_is_whole():
    names = [f"{p}/{c}" for p, c, _, _ in CASES]
    assert len(set(names)) == len(names) and set(names) == set(EXPECTED)


@pytest.mark.parametrize("parser,case,over,put", CASES, ids=[f"{p}-{c}" for p, c, _, _ in CASES])
def test_parser_returns_or_raises_what_it_did(parser, case, over, put):
    got, want = observe(parser, over, put), EXPECTED[f"{parser}/{case}"]
    assert got == want
    if isinstance(want, list):
        assert [type(v) for _, v in got] == [type(v) for _, v in want]         # (True == 1 and 15 == 15.0 would pass the line above)


# what the model object carries of all this: (overrides, {attribute: value})
MODEL_CASES = [
    ({},
     {"gt_init": False, "fit_init": False, "fit_init_cfg": [("inlier_th", 0.003), ("num_hyps", 64), ("seed", 0)], "fit_init_yaxis": False,
      "image_fit": None, "guard": None, "st_fit": None, "rot_pool": None, "otf_thin": None, "depth_filter": None}),
    ({"nocs_otf": True, G + "lost_below": 0.5, G + "yaxis_only": True, **S_ON, **R_ON, **T_ON, T + "seed": 5, **D_ON, I + "fit": True,
      I + "inlier_th": 0.01, I + "num_hyps": 48, I + "seed": 9, I + "yaxis_only": True, I + "gt": True},
     {"gt_init": True, "fit_init": True, "fit_init_cfg": [("inlier_th", 0.006), ("num_hyps", 48), ("seed", 9)], "fit_init_yaxis": True,
      "image_fit": None,
      "guard": [("refit", False), ("lost_below", (1, 2)), ("inlier_th", 0.003), ("min_members", 4), ("num_hyps", 48), ("seed", 9),
                ("yaxis_only", True)],
      "st_fit": [("inlier_th", 0.003), ("num_hyps", 48), ("seed", 9)], "rot_pool": [("angle_th", 15.0), ("num_hyps", 48), ("seed", 9)],
      "otf_thin": [("seed", 5)], "depth_filter": [("window", 2), ("abs_mm", 10), ("rel_permille", 0), ("min_support", 6)]}),
    ({**I_ON, I + "border": 2, G + "lost_below": 0.25, G + "seed": 4},
     {"gt_init": False, "fit_init": False, "fit_init_cfg": [("inlier_th", 0.003), ("num_hyps", 64), ("seed", 0)], "fit_init_yaxis": False,
      "image_fit": [("cap", 16384), ("border", 2), ("negate_z", False)],
      "guard": [("refit", False), ("lost_below", (1, 4)), ("inlier_th", 0.003), ("min_members", 4), ("num_hyps", 64), ("seed", 4)],
      "st_fit": None, "rot_pool": None, "otf_thin": None, "depth_filter": None}),
]


@pytest.mark.parametrize("over,want", MODEL_CASES, ids=[str(i) for i in range(len(MODEL_CASES))])
def test_the_model_keeps_its_attributes(over, want):
    assert model_attributes(over) == want


ATTRIBUTES = ("gt_init", "fit_init", "fit_init_cfg", "fit_init_yaxis", "image_fit", "guard", "st_fit", "rot_pool", "otf_thin", "depth_filter")


def model_attributes(over):
    from captra_amd.trainer import Trainer
    cfg = _make({"experiment_dir": "/tmp/captra_test_exp", **over}, {("device",): "cpu"})
    model = Trainer(cfg).model
    assert model.net.st_fit is model.st_fit and model.net.rot_pool is model.rot_pool
    return {k: (list(v.items()) if isinstance(v, dict) else v) for k, v in ((k, getattr(model, k)) for k in ATTRIBUTES)}


# ---- the records: the pickle's layout and the one commit wrapper ---------------------------------------------------------------
def _same(got, want, where="record"):
    """Equal in structure, key order, None places, dtype, shape and value."""
    assert type(got) is type(want), (where, type(got), type(want))
    if isinstance(want, dict):
        assert list(got) == list(want), where
        for k in want:
            _same(got[k], want[k], f"{where}[{k!r}]")
    elif isinstance(want, list):
        assert len(got) == len(want), where
        for i, (g, w) in enumerate(zip(got, want)):
            _same(g, w, f"{where}[{i}]")
    elif isinstance(want, np.ndarray):
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), where
    else:
        assert want is None and got is None, where


def _pred_dict():
    """Three frames of B = 2 trajectories with P = 2 parts, every record present, as `forward` leaves them (CPU tensors)."""
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    pose = {"rotation": torch.eye(3).repeat(2, 2, 1, 1), "translation": torch.zeros(2, 2, 3, 1), "scale": torch.ones(2, 2)}
    return {"poses": [pose, pose, pose], "npcs_pred": [None, {}, {}],
            "guard": [None,
                      {"count": i32([10, 11], [12, 13]), "inliers": i32([9, 8], [7, 6]), "rms": torch.tensor([[0.5, 0.25], [0.125, 2.0]]),
                       "verdict": i32([0, 1], [2, 3])},
                      {"count": i32([20, 21], [22, 23]), "inliers": i32([19, 18], [17, 16]), "rms": torch.tensor([[1.5, 1.25], [1.125, 3.0]]),
                       "verdict": i32([3, 2], [1, 0])}],
            "st_fit": [None, {"inliers": i32([5, 6], [7, 8]), "valid": i32([1, 0], [1, 1])}, {"inliers": i32([1, 2], [3, 4]), "valid": i32([0, 0], [1, 0])}],
            "rot_pool": [None, {"inliers": i32([50, 60], [70, 80]), "count": i32([100, 0], [90, 95])},
                         {"inliers": i32([51, 61], [71, 81]), "count": i32([101, 1], [91, 96])}],
            "otf_thin": [None, i32(1, 0), i32(0, 0)],
            "depth_filter": [i32(640, 0), None, i32(7, 700)],                      # (frame 1 came without a depth image)
            "image_fit": {"members": i32(24950, 3), "used": i32(12475, 3), "holes": i32(301, 0), "inliers": i32(12000, 2), "valid": i32(1, 0)}}


def test_the_pickles_record_layout():
    a32, f32 = (lambda *v: np.array(v, np.int32)), (lambda *v: np.array(v, np.float32))
    want = {
        "guard": [None,
                  {"count": a32([10, 11], [12, 13]), "inliers": a32([9, 8], [7, 6]), "rms": f32([0.5, 0.25], [0.125, 2.0]), "verdict": a32([0, 1], [2, 3])},
                  {"count": a32([20, 21], [22, 23]), "inliers": a32([19, 18], [17, 16]), "rms": f32([1.5, 1.25], [1.125, 3.0]), "verdict": a32([3, 2], [1, 0])}],
        "st_fit": [None, {"inliers": a32([5, 6], [7, 8]), "valid": a32([1, 0], [1, 1])}, {"inliers": a32([1, 2], [3, 4]), "valid": a32([0, 0], [1, 0])}],
        "rot_pool": [None, {"inliers": a32([50, 60], [70, 80]), "count": a32([100, 0], [90, 95])},
                     {"inliers": a32([51, 61], [71, 81]), "count": a32([101, 1], [91, 96])}],
        "otf_thin": [None, {"thinned": a32(1, 0)}, {"thinned": a32(0, 0)}],
        "depth_filter": [{"removed": a32(640, 0)}, None, {"removed": a32(7, 700)}],
        "image_fit": {"members": a32(24950, 3), "used": a32(12475, 3), "holes": a32(301, 0), "inliers": a32(12000, 2), "valid": a32(1, 0)},
    }
    _same(_M.records_to_numpy(_pred_dict()), want)
    _same(_M.records_to_numpy(_pred_dict(), guard_yaxis_only=False), want)
    want["guard"][0] = {"yaxis_only": np.array([True, True])}                      # the head: one boolean per trajectory, only when on
    _same(_M.records_to_numpy(_pred_dict(), guard_yaxis_only=True), want)
    # what get_ith_from_batch makes of it is the per-trajectory pickle: every array indexed by the trajectory
    from captra_amd.utils import get_ith_from_batch
    one = get_ith_from_batch(_M.records_to_numpy(_pred_dict(), guard_yaxis_only=True), 1, to_single=False)
    assert one["guard"][0]["yaxis_only"] == np.bool_(True) and one["guard"][2]["verdict"].tolist() == [1, 0] and one["depth_filter"][1] is None
    assert one["otf_thin"][1]["thinned"] == np.int32(0) and one["image_fit"]["valid"] == np.int32(0) and one["depth_filter"][2]["removed"] == 700


def test_no_option_adds_no_key():
    plain = {k: v for k, v in _pred_dict().items() if k in ("poses", "npcs_pred")}
    assert _M.records_to_numpy(plain) == {} and _M.records_to_numpy(plain, guard_yaxis_only=True) == {}
    some = {k: v for k, v in _pred_dict().items() if k in ("poses", "npcs_pred", "st_fit", "depth_filter")}
    assert list(_M.records_to_numpy(some, guard_yaxis_only=True)) == ["st_fit", "depth_filter"]
    assert list(_M.records_to_numpy(_pred_dict())) == ["guard", "st_fit", "rot_pool", "otf_thin", "depth_filter", "image_fit"]


@pytest.mark.parametrize("active", [("guard", "st_fit", "rot_pool"), ("guard",), ("st_fit",), ("rot_pool",), ("guard", "rot_pool"),
                                    ("st_fit", "rot_pool"), ("guard", "st_fit"), ()])
def test_one_commit_wrapper_takes_every_active_record_out(active):
    """The maps a batch form's `commit` returns, in the order the step fills them: CoordinateNet's own, then st_*, rot_*, guard_* of
    the options that are on.  What stays -- and its order, which the lanes' concatenation and copy batching go by -- is what three
    nested one-record wrappers left: CoordinateNet's own maps, in their order."""
    values = {"st_fit": {"inliers": 1, "valid": 2}, "rot_pool": {"inliers": 3, "count": 4},
              "guard": {"count": 5, "inliers": 6, "rms": 7, "verdict": 8}}
    calls = []

    def commit(i, result):
        calls.append((i, result))
        npcs = {"seg": "seg%d" % i, "nocs": "nocs%d" % i, "points": "points%d" % i}
        for name in ("st_fit", "rot_pool", "guard"):                # (_step_post's order)
            if name in active:
                _M.put_record(npcs, name, {k: 10 * i + v for k, v in values[name].items()})
        return npcs, {"scale": i}

    filled = {"st_fit": ["seg", "nocs", "points", "st_inliers", "st_valid"], "rot_pool": ["seg", "nocs", "points", "rot_inliers", "rot_count"],
              "guard": ["seg", "nocs", "points", "guard_count", "guard_inliers", "guard_rms", "guard_verdict"]}
    if len(active) == 1:
        assert list(commit(0, None)[0]) == filled[active[0]]
    if len(active) == 3:
        assert list(commit(0, None)[0]) == ["seg", "nocs", "points", "st_inliers", "st_valid", "rot_inliers", "rot_count", "guard_count",
                                            "guard_inliers", "guard_rms", "guard_verdict"]
    calls.clear()
    records = {name: {} for name in _M.STEP_RECORDS if name in active}
    assert list(records) == [n for n in ("guard", "st_fit", "rot_pool") if n in active]
    wrapped = _M.commit_with_records(commit, records)
    if not active:
        assert wrapped is commit                                    # nothing on: the batch form's own commit, no call in between
    for i in (1, 2):
        npcs, pose = wrapped(i, "result%d" % i)
        assert list(npcs.items()) == [("seg", "seg%d" % i), ("nocs", "nocs%d" % i), ("points", "points%d" % i)] and pose == {"scale": i}
    assert calls == [(1, "result1"), (2, "result2")]
    want = {"guard": {1: [("count", 15), ("inliers", 16), ("rms", 17), ("verdict", 18)], 2: [("count", 25), ("inliers", 26), ("rms", 27), ("verdict", 28)]},
            "st_fit": {1: [("inliers", 11), ("valid", 12)], 2: [("inliers", 21), ("valid", 22)]},
            "rot_pool": {1: [("inliers", 13), ("count", 14)], 2: [("inliers", 23), ("count", 24)]}}
    assert {n: {i: list(r.items()) for i, r in f.items()} for n, f in records.items()} == {n: want[n] for n in records}
    wrapped(1, "again")                                             # a replayed frame's record takes the first run's place
    assert all(list(f) == [1, 2] for f in records.values())
