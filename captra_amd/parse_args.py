"""The command-line surface shared by the harnesses: every flag of the reference's network/parse_args.py:5-69, same
names, types and defaults (a flag named `a/b` overrides cfg['a']['b'], None = keep the YAML value).  Declared as a table
so that `track`, `train` and `eval` register exactly the same set; flags whose subsystem is outside this build
(`--num_workers`, `--dataset_length`, `--eval_train`: DataLoader options) are accepted and ignored.
"""
from __future__ import annotations

import argparse


def boolean_string(s: str) -> bool:
    if s not in ("True", "False"):
        raise ValueError("Not a valid boolean string")
    return s == "True"


_FLAGS = [  # (name, type, default)
    ("obj_config", str, None), ("obj_category", str, None), ("experiment_dir", str, None), ("resume_epoch", int, -1),
    ("coord_exp/dir", str, None), ("coord_exp/resume_epoch", int, None),
    ("batch_size", int, None), ("cuda_id", int, None), ("num_points", int, None), ("data_radius", float, None),
    ("num_workers", int, 0), ("dataset_length", int, None), ("pointnet_cfg/camera", str, None),
    ("network/type", str, None), ("network/nocs_head_dims", int, None), ("network/backbone_out_dim", int, None),
    ("network/pwm_num", int, None),
    ("init_frame/gt", boolean_string, None), ("init_frame/fit", boolean_string, None), ("nocs_otf", boolean_string, None),
    ("track_cfg/gt_label", boolean_string, None), ("track_cfg/nocs2d_label", boolean_string, None), ("track_cfg/nocs2d_path", str, None),
    # track health (track_options.py: guard_cfg); lost_below has no default
    ("track_cfg/guard/refit", boolean_string, None), ("track_cfg/guard/lost_below", float, None), ("track_cfg/guard/inlier_th", float, None),
    ("track_cfg/guard/min_members", int, None), ("track_cfg/guard/num_hyps", int, None), ("track_cfg/guard/seed", int, None),
    # the axis-only inlier test of the symmetric categories, in the guard and in the first-pose fit (init_frame/fit).  Not given = not
    # in the namespace at all (argparse.SUPPRESS): the key reaches the configuration only when it was written
    ("track_cfg/guard/yaxis_only", boolean_string, argparse.SUPPRESS), ("init_frame/yaxis_only", boolean_string, argparse.SUPPRESS),
    # the first pose fitted from frame 0's depth, mask and NOCS coordinate image (track_options.py: image_fit_cfg); off unless image_fit
    # is True.  Not given = not in the namespace at all, like yaxis_only
    ("init_frame/image_fit", boolean_string, argparse.SUPPRESS), ("init_frame/border", int, argparse.SUPPRESS),
    ("init_frame/cap", int, argparse.SUPPRESS), ("init_frame/coord_negate_z", boolean_string, argparse.SUPPRESS),
    # the robust scale / translation fit of every step (track_options.py: st_fit_cfg); off unless ransac is True
    ("track_cfg/st_fit/ransac", boolean_string, None), ("track_cfg/st_fit/inlier_th", float, None), ("track_cfg/st_fit/num_hyps", int, None),
    ("track_cfg/st_fit/seed", int, None),
    # the consensus rotation read-out of every step (track_options.py: rot_pool_cfg); off unless consensus is True, and then angle_th
    # (degrees) is required
    ("track_cfg/rot_pool/consensus", boolean_string, None), ("track_cfg/rot_pool/angle_th", float, None),
    ("track_cfg/rot_pool/num_hyps", int, None), ("track_cfg/rot_pool/seed", int, None),
    # the re-crop's over-long candidate lists thinned on the device (track_options.py: otf_thin_cfg); off unless device is True
    ("track_cfg/otf_thin/device", boolean_string, None), ("track_cfg/otf_thin/seed", int, None),
    # flying depth pixels removed from every uploaded depth image (track_options.py: depth_filter_cfg); on when any of the four is
    # given, and then abs_mm (depth counts: millimetres for a millimetre sensor) and min_support are required
    ("track_cfg/depth_filter/window", int, None), ("track_cfg/depth_filter/abs_mm", int, None),
    ("track_cfg/depth_filter/rel_permille", int, None), ("track_cfg/depth_filter/min_support", int, None),
    # the camera of the depth images (track_options.py: camera_cfg): a preset, or fx / fy / cx / cy (required then), skew and depth_unit
    # (metres per depth count).  Not given = not in the namespace at all, like yaxis_only: no `camera` section appears
    ("camera/preset", str, argparse.SUPPRESS), ("camera/fx", float, argparse.SUPPRESS), ("camera/fy", float, argparse.SUPPRESS),
    ("camera/cx", float, argparse.SUPPRESS), ("camera/cy", float, argparse.SUPPRESS), ("camera/skew", float, argparse.SUPPRESS),
    ("camera/depth_unit", float, argparse.SUPPRESS),
    # every step starts from a constant-velocity prediction (track_options.py: motion_cfg); off unless predict is True, and then max_angle
    # (degrees) and max_shift (a fraction of data_radius) are required
    ("track_cfg/motion/predict", boolean_string, None), ("track_cfg/motion/max_angle", float, None),
    ("track_cfg/motion/max_shift", float, None), ("track_cfg/motion/gain", float, None),
    # every step holds the part's running scale (track_options.py: size_cfg); off unless hold is True, and then max_ratio is required.
    # Not given = not in the namespace at all, like yaxis_only
    ("track_cfg/size/hold", boolean_string, argparse.SUPPRESS), ("track_cfg/size/max_ratio", float, argparse.SUPPRESS),
    ("track_cfg/size/min_frames", int, argparse.SUPPRESS), ("track_cfg/size/max_frames", int, argparse.SUPPRESS),
    ("track_cfg/size/reset_after", int, argparse.SUPPRESS), ("track_cfg/size/init_frames", int, argparse.SUPPRESS),
    # every step holds the part's box: a histogram of the predicted NOCS coordinates over the track (track_options.py: box_cfg); off
    # unless hold is True, and then quantile is required.  Not given = not in the namespace at all, like the size flags
    ("track_cfg/box/hold", boolean_string, argparse.SUPPRESS), ("track_cfg/box/quantile", float, argparse.SUPPRESS),
    ("track_cfg/box/bins", int, argparse.SUPPRESS), ("track_cfg/box/min_points", int, argparse.SUPPRESS),
    ("track_cfg/box/radial", boolean_string, argparse.SUPPRESS),
    # optimisation
    ("total_epoch", int, None), ("optimizer", str, None), ("weight_decay", float, None), ("learning_rate", float, None),
    ("lr_policy", str, None), ("lr_gamma", float, None), ("lr_step_size", int, None), ("lr_clip", float, None), ("freq/save", int, None),
]
_FLAGS += [(f"loss_weight/{k}", float, None) for k in ("rloss", "tloss", "sloss", "corner_loss", "nocs_loss", "nocs_dist_loss",
                                                        "nocs_pwm_loss", "seg_loss")]
_FLAGS += [(f"pose_loss_type/{k}", str, None) for k in ("r", "s", "t", "point")]
_FLAGS += [("pose_perturb/type", str, None)] + [(f"pose_perturb/{k}", float, None) for k in ("r", "s", "t")]
_SWITCHES = ("save", "eval_train", "no_eval")
HARNESS_ONLY = ("num_workers", "dataset_length", "eval_train", "save", "no_eval")     # not configuration overrides


def add_args(parser: argparse.ArgumentParser, default_config: str = "config.yml") -> argparse.ArgumentParser:
    parser.add_argument("--config", type=str, default=default_config)
    for name, typ, default in _FLAGS:
        parser.add_argument(f"--{name}", type=typ, default=default)
    for name in _SWITCHES:
        parser.add_argument(f"--{name}", action="store_true", default=False)
    return parser
