"""The track loop's opt-in features, as far as they are plumbing: each option's section of the configuration parsed once into the
dict `EvalTrackModel` keeps (None = off: no launch, no tensor, no pickle entry), and ONE description of the records the options
leave per frame: how they travel inside CoordinateNet's maps, are listed in `pred_dict` and laid out in the result pickle."""
import numpy as np

# init_frame/fit: the inlier distance of the first-pose fit as a fraction of data_radius -- 3 mm at the NOCS crops' 0.6 m: the
# reference's preprocessing uses 1 mm on rendered (exact) maps (align_pose.py:49), sensor depth at 1 m is noisy at the millimetre
INIT_FIT_INLIER_TH = 0.005


# ---- the parsers: cfg -> None (off) or the option's dict --------------------------------------------------------------------
def _draws(cfg, section, check=None):
    """(num_hyps, seed) of a RANSAC option: the section's own, else init_frame's, else (64, 0); check = the section's name: in range too."""
    num_hyps, seed = section.get("num_hyps"), section.get("seed")
    num_hyps = int(cfg["init_frame"].get("num_hyps", 64) if num_hyps is None else num_hyps)
    seed = int(cfg["init_frame"].get("seed", 0) if seed is None else seed)
    if check is not None and not 1 <= num_hyps <= 256:
        raise ValueError(f"{check}/num_hyps must be in [1, 256] (the kernel's limit), got {num_hyps}")
    if check is not None and seed < 0:
        raise ValueError(f"{check}/seed must not be negative, got {seed}")
    return num_hyps, seed


def yaxis_only(cfg, section, name) -> bool:
    """init_frame: {yaxis_only: True} / track_cfg: {guard: {yaxis_only: True}}: the AXIS-ONLY inlier test (include/captra_hip.h,
    captra_part_fit_guard_sym) for a symmetric category, whose tracked in-plane angle carries no information.  Absent / False:
    today's launches and records; True on a category that is not symmetric is an error."""
    on = bool(section.get("yaxis_only", False))
    if on and not cfg["obj_sym"]:
        raise ValueError(f"{name}: the axis-only inlier test is for symmetric categories (obj_sym), category "
                         f"{cfg['obj_category']} is not one: its in-plane angle is part of the pose")
    return on


def init_fit_cfg(cfg):
    """init_frame: {fit: True}: the first pose is FITTED to frame 0's own NOCS map, labels and points (RANSAC similarity fit,
    csrc/pose_ransac.hip) -- no pose annotation is needed to start a track.  inlier_th is a fraction of data_radius (default
    INIT_FIT_INLIER_TH); num_hyps hypotheses drawn in the kernel from `seed`.  (Parsed always: init_frame/image_fit reads them too.)"""
    num_hyps, seed = _draws(cfg, {})
    return {"inlier_th": float(cfg["init_frame"].get("inlier_th", INIT_FIT_INLIER_TH)) * float(cfg["data_radius"]), "num_hyps": num_hyps, "seed": seed}


def image_fit_cfg(cfg):
    """init_frame: {image_fit: True, border: 0, cap: 16384, coord_negate_z: False}: the first pose is fitted to frame 0's IMAGES -- the
    depth image, the instance mask and the NOCS coordinate image of meta['pre_fetched'], the three outputs of a NOCS-style
    detector (csrc/image_fit.hip turns them into correspondences, the same RANSAC fit as init_frame/fit reads them with its
    inlier_th, num_hyps, seed and yaxis_only) -- so a track starts from images alone.  The fit is recorded (pred_dict / pickle
    'image_fit').  None when absent or not set, else {'cap', 'border', 'negate_z'} inside the kernels' ranges."""
    from .nocs_otf import IMAGE_FIT_CAP, check_image_fit_params
    f = cfg["init_frame"]
    if not f.get("image_fit", False):
        return None
    if f.get("fit", False):
        raise ValueError("init_frame/image_fit and init_frame/fit both fit the first pose, one from frame 0's images and one from its "
                         "pre-cropped cloud: set one of them")
    if int(cfg["num_parts"]) != 1:
        raise ValueError(f"init_frame/image_fit fits one rigid object (a coordinate image describes one), this object has num_parts = "
                         f"{cfg['num_parts']}")
    cap, border = f.get("cap"), f.get("border")
    cap, border = check_image_fit_params(IMAGE_FIT_CAP if cap is None else cap, 0 if border is None else border, prefix="init_frame/")
    return {"cap": cap, "border": border, "negate_z": bool(f.get("coord_negate_z", False))}


def guard_cfg(cfg):
    """track_cfg: {guard: {...}}: every step checks the pose it produced against the frame's own NOCS map, labels and points
    (csrc/pose_guard.hip, one launch behind the pose fit, captured with the step) and, with refit, re-fits a part found lost
    by the first-pose estimator.  None when absent; lost_below has no default; inlier_th is a fraction of data_radius; num_hyps
    and seed default to init_frame's and are NOT held to the kernel's ranges here."""
    g = cfg["track_cfg"].get("guard")
    if g is None:
        return None
    if g.get("lost_below") is None:
        raise ValueError("track_cfg/guard needs lost_below (the inlier fraction below which a part counts as lost): it has no default")
    from .pose_utils.pose_fit import lost_ratio
    num_hyps, seed = _draws(cfg, {})
    # lost_below as the two ints the kernel compares with, converted once (raises on a value outside [0, 1]); the draws by
    # g.get(key, default), not through _draws: an explicit null is a TypeError here, as it always was
    out = {"refit": bool(g.get("refit", False)), "lost_below": lost_ratio(g["lost_below"]),
           "inlier_th": float(g.get("inlier_th", INIT_FIT_INLIER_TH)) * float(cfg["data_radius"]),
           "min_members": int(g.get("min_members", 4)), "num_hyps": int(g.get("num_hyps", num_hyps)), "seed": int(g.get("seed", seed))}
    if yaxis_only(cfg, g, "track_cfg/guard/yaxis_only"):
        out["yaxis_only"] = True            # (carried only when on)
    return out


def st_fit_cfg(cfg):
    """track_cfg: {st_fit: {ransac: True, ...}}: every step's scale / translation by RANSAC with RotationNet's rotation given
    (csrc/pose_st_ransac.hip, in place of the one-pass fit's launch, captured with the step); the inlier test is the axis-only
    one for a symmetric category.  The guard, when on, judges the pose this fit produced.  None when absent or ransac is not set;
    inlier_th is a fraction of data_radius (the guard's default), num_hyps and seed default to init_frame's."""
    s = cfg["track_cfg"].get("st_fit")
    if s is None or not s.get("ransac", False):
        return None
    frac = s.get("inlier_th")
    frac = INIT_FIT_INLIER_TH if frac is None else float(frac)
    if not (frac > 0.0 and np.isfinite(frac)):
        raise ValueError(f"track_cfg/st_fit/inlier_th must be a positive fraction of data_radius, got {s.get('inlier_th')!r}")
    num_hyps, seed = _draws(cfg, s, check="track_cfg/st_fit")
    return {"inlier_th": frac * float(cfg["data_radius"]), "num_hyps": num_hyps, "seed": seed}


def rot_pool_cfg(cfg):
    """track_cfg: {rot_pool: {consensus: True, angle_th: <degrees>, ...}}: every step's rotation from the consensus of RotationNet's
    per-point votes (csrc/rot_consensus.hip, in place of the plain read-out's launch, captured with the step); the scale /
    translation fit and the guard consume that rotation unchanged.  None when absent or consensus is not set; angle_th has no
    default -- the right value depends on the trained network's vote scatter --, num_hyps and seed default to init_frame's."""
    s = cfg["track_cfg"].get("rot_pool")
    if s is None or not s.get("consensus", False):
        return None
    angle = s.get("angle_th")
    if angle is None:
        raise ValueError("track_cfg/rot_pool/consensus needs track_cfg/rot_pool/angle_th (degrees, inside (0, 180)): it has no default")
    angle = float(angle)
    if not 0.0 < angle < 180.0:
        raise ValueError(f"track_cfg/rot_pool/angle_th must be an angle in degrees inside (0, 180), got {s.get('angle_th')!r}")
    num_hyps, seed = _draws(cfg, s, check="track_cfg/rot_pool")
    return {"angle_th": angle, "num_hyps": num_hyps, "seed": seed}


def otf_thin_cfg(cfg):
    """track_cfg: {otf_thin: {device: True, seed: <int>}}: the re-crop thins a candidate list of more than 5 N ball members ON THE
    DEVICE (csrc/otf_thin.hip: a counter-based draw keyed by seed, trajectory and frame, the kept members in pixel order -- not
    numpy's permutation, see include/captra_hip.h) instead of on the host, so a close-up crop is no rare-path instance of the
    sync-free loop; the frames' thinned instances are recorded (pred_dict / pickle 'otf_thin').  None when absent or device is not
    set (numpy's generator is consumed as before), else {'seed'}."""
    t = cfg["track_cfg"].get("otf_thin")
    if t is None or not t.get("device", False):
        return None
    seed = int(t.get("seed", 0) or 0)       # its own default, not init_frame's: the seed keys the thinning draw, not a RANSAC
    if seed < 0:
        raise ValueError(f"track_cfg/otf_thin/seed must not be negative, got {seed}")
    return {"seed": seed}


def depth_filter_cfg(cfg):
    """track_cfg: {depth_filter: {window: 2, abs_mm: <int>, rel_permille: 0, min_support: <int>}}: every uploaded depth image loses
    its flying pixels -- those that fewer than min_support of their image neighbours support in depth (csrc/depth_filter.hip,
    include/captra_hip.h: captra_depth_support_filter) -- ONCE, when the frame is put on the device (set_data): one launch per
    frame over all trajectories, outside the step, the lanes and the replay of a flagged frame, which all read the filtered
    image.  The removed pixels are recorded per frame and trajectory (pred_dict / pickle 'depth_filter').  None when absent (the
    upload is used as it is), else the four inside the kernel's ranges; abs_mm and min_support have no default: the right values
    depend on the sensor and on the window.  abs_mm is in DEPTH COUNTS -- millimetres for a millimetre sensor, hence the name; under
    a `camera` whose depth_unit is not 0.001 it is abs_mm x depth_unit metres (the kernel compares counts and knows no unit)."""
    from .nocs_otf import check_depth_filter_params
    f = cfg["track_cfg"].get("depth_filter")
    if f is None:
        return None
    if not cfg.get("nocs_otf", False):
        raise ValueError("track_cfg/depth_filter filters the depth images the on-the-fly re-crop reads: it needs nocs_otf: True "
                         "(without it there is no depth image)")
    for key in ("abs_mm", "min_support"):
        if f.get(key) is None:
            raise ValueError(f"track_cfg/depth_filter needs track_cfg/depth_filter/{key}: it has no default")
    window, rel = f.get("window"), f.get("rel_permille")
    vals = check_depth_filter_params(2 if window is None else window, f["abs_mm"], 0 if rel is None else rel, f["min_support"],
                                     prefix="track_cfg/depth_filter/")
    return dict(zip(("window", "abs_mm", "rel_permille", "min_support"), vals))


CAMERA_KEYS = ("fx", "fy", "cx", "cy", "skew", "depth_unit")


def camera_cfg(cfg):
    """camera: {preset: nocs_real | nocs_camera} or camera: {fx, fy, cx, cy, skew: 0, depth_unit: 0.001}: the camera of every trajectory
    that does not carry its own (meta['pre_fetched']['camera']) -- the intrinsics the re-crop projects and back-projects with and the
    depth unit, metres per depth count (csrc/crop.hip, csrc/image_fit.hip: the *_cam entry points, include/captra_hip.h).  The pixel
    and frame convention stays the reference's: ray = K^-1 (col, h - row, 1), p_z negated.  nocs_real is the camera everything was wired
    to (591.0125, 590.16775, 322.525, 244.11084); nocs_camera the CAMERA25 images' (577.5, 577.5, 319.5, 239.5); both count millimetres.
    None when absent (the plain entry points are called and no camera tensor exists), else {'K' (3,3) float64, 'depth_unit' float}; a
    camera that is not valid is a ValueError that names the key."""
    from .nocs_otf import CAMERA_PRESETS, check_camera
    c = cfg.get("camera")
    if c is None:
        return None
    if not isinstance(c, dict):
        raise ValueError(f"camera must be a section (preset, or fx / fy / cx / cy / skew / depth_unit), got {c!r}")
    unknown = [k for k in c if k != "preset" and k not in CAMERA_KEYS]
    if unknown:
        raise ValueError(f"camera: unknown keys {unknown} (preset, or {', '.join(CAMERA_KEYS)})")
    if not cfg.get("nocs_otf", False) and not cfg["init_frame"].get("image_fit", False):
        raise ValueError("camera is the camera of the depth images the on-the-fly re-crop and the first-pose image fit read: it needs "
                         "nocs_otf: True or init_frame/image_fit: True (without them there is no depth image)")
    given = [k for k in CAMERA_KEYS if c.get(k) is not None]
    if c.get("preset") is not None:
        if given:
            raise ValueError(f"camera/preset and camera/{given[0]} both describe the camera: set the preset or the explicit keys")
        if c["preset"] not in CAMERA_PRESETS:
            raise ValueError(f"camera/preset must be one of {sorted(CAMERA_PRESETS)}, got {c['preset']!r}")
        K, unit = CAMERA_PRESETS[c["preset"]]
    else:
        vals = {}
        for key, default in (("fx", None), ("fy", None), ("cx", None), ("cy", None), ("skew", 0.0), ("depth_unit", 0.001)):
            v = c.get(key)
            v = default if v is None else v
            if v is None:
                raise ValueError(f"camera needs camera/{key}: it has no default (or set camera/preset)")
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
                raise ValueError(f"camera/{key} must be a number, got {v!r}")
            vals[key] = float(v)
        K = np.array([[vals["fx"], vals["skew"], vals["cx"]], [0.0, vals["fy"], vals["cy"]], [0.0, 0.0, 1.0]])
        unit = vals["depth_unit"]
    K, unit = check_camera(K, unit, prefix="camera/")
    return {"K": K.copy(), "depth_unit": unit}


def trajectory_cameras(frame_camera, cfg_camera, batch: int):
    """The cameras of a batch's trajectories, by precedence: frame 0's own (meta['pre_fetched']['camera'] = {'K' (B,3,3), 'depth_unit'
    (B,)}), then the configuration's (camera_cfg) for all of them, then None.  -> None or {'K' (B,3,3), 'depth_unit' (B,)} float64 host
    arrays, each camera checked (a ValueError names the entry)."""
    from .nocs_otf import check_camera
    if frame_camera is not None:
        missing = [k for k in ("K", "depth_unit") if k not in frame_camera]
        if missing:
            raise ValueError(f"meta['pre_fetched']['camera'] needs {missing}: it is {{'K': (B,3,3), 'depth_unit': (B,)}}")
        to_np = lambda v: np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, np.float64)
        K, unit = to_np(frame_camera["K"]), to_np(frame_camera["depth_unit"]).reshape(-1)
        if K.shape != (batch, 3, 3) or unit.shape != (batch,):
            raise ValueError(f"meta['pre_fetched']['camera']: K (B,3,3) and depth_unit (B,) with B = {batch} trajectories, got {K.shape} and {unit.shape}")
        for b in range(batch):
            check_camera(K[b], unit[b], prefix=f"meta['pre_fetched']['camera'] of trajectory {b}: ")
        return {"K": K.copy(), "depth_unit": unit.copy()}
    if cfg_camera is not None:
        return {"K": np.broadcast_to(cfg_camera["K"], (batch, 3, 3)).copy(), "depth_unit": np.full(batch, cfg_camera["depth_unit"], np.float64)}
    return None


def motion_cfg(cfg):
    """track_cfg: {motion: {predict: True, max_angle: <degrees>, max_shift: <fraction of data_radius>, gain: 1.0}}: every step STARTS
    from a constant-velocity prediction instead of the pose the step before produced (csrc/pose_motion.hip, include/captra_hip.h:
    captra_pose_extrapolate -- one launch behind the fit and the guard, captured with the step): the re-crop's centre, both networks'
    canonicalisation, R_prev of the read-out and what an invalid fit keeps.  The prediction travels in the pose dict (next_rotation,
    next_translation, measured) and is recorded per frame (pred_dict / pickle 'motion').  None when absent or predict is not set;
    max_angle and max_shift have no default -- they depend on the frame rate and on how fast the objects move: a step larger than
    either is a glitch in the history, not a velocity --, max_shift is a fraction of data_radius, gain defaults to 1."""
    m = cfg["track_cfg"].get("motion")
    if m is None or not m.get("predict", False):
        return None
    vals = {}
    for key, lo_open, hi, what in (("max_angle", 0.0, 90.0, "an angle in degrees inside (0, 90]"),
                                   ("max_shift", 0.0, np.inf, "a positive fraction of data_radius"), ("gain", 0.0, 1.0, "inside (0, 1]")):
        v = m.get(key)
        if v is None and key == "gain":
            v = 1.0
        if v is None:
            raise ValueError(f"track_cfg/motion/predict needs track_cfg/motion/{key} ({what}): it has no default")
        v = float(v)
        if not (lo_open < v <= hi and np.isfinite(v)):
            raise ValueError(f"track_cfg/motion/{key} must be {what}, got {m.get(key)!r}")
        vals[key] = v
    vals["max_shift"] *= float(cfg["data_radius"])
    return vals


def size_cfg(cfg):
    """track_cfg: {size: {hold: True, max_ratio: <ratio>, min_frames: 1, max_frames: None, reset_after: None, init_frames: 0}}: every
    step keeps the running mean of each part's scale -- a rigid part's NOCS scale is a constant of the instance -- and, once min_frames
    frames are in it, HOLDS the pose's scale at that mean and fits the translation with the scale given (csrc/pose_size.hip,
    include/captra_hip.h: captra_part_fit_st_size -- in place of the robust fit's launch, or one launch behind the one-pass fit's,
    captured with the step).  A frame whose own (free) scale is more than max_ratio away from an established mean is gated out of the
    mean; reset_after such frames in a row restart it; max_frames caps the averaging window.  The state travels in the pose dict
    (size_mean, size_n, size_miss) and is recorded per frame (pred_dict / pickle 'size').  None when absent or hold is not set;
    max_ratio has no default -- it depends on the trained network's scale scatter --; init_frames: how many frames the track's first
    pose counts for (>= min_frames: its size is held from frame 1 on and then averaged in)."""
    s = cfg["track_cfg"].get("size")
    if s is None or not s.get("hold", False):
        return None
    ratio = s.get("max_ratio")
    if ratio is None:
        raise ValueError("track_cfg/size/hold needs track_cfg/size/max_ratio (the largest ratio between a frame's scale and the running "
                         "mean, > 1): it has no default")
    ratio = float(np.float32(ratio))        # (the kernel's argument is fp32)
    if not (ratio > 1.0 and np.isfinite(ratio)):
        raise ValueError(f"track_cfg/size/max_ratio must be a finite ratio > 1, got {s.get('max_ratio')!r}")
    out = {"max_ratio": ratio}
    for key, default, lo in (("min_frames", 1, 1), ("max_frames", None, 1), ("reset_after", None, 1), ("init_frames", 0, 0)):
        v = s.get(key)
        v = default if v is None else v
        if v is not None:
            if isinstance(v, bool) or int(v) != v or not lo <= int(v) < 2 ** 31:
                raise ValueError(f"track_cfg/size/{key} must be an integer >= {lo}, got {s.get(key)!r}")
            v = int(v)
        out[key] = v
    return out


def box_cfg(cfg):
    """track_cfg: {box: {hold: True, quantile: <q>, bins: 128, min_points: 16, radial: False}}: every step adds the frame's predicted NOCS
    coordinates to a per-part histogram of |x|, |y|, |z| kept over the track -- a part's box is a constant of the instance -- and reads
    the box's half-extents out of it as the `quantile` of each axis, rounded up to the bin's edge (csrc/pose_box.hip,
    include/captra_hip.h: captra_part_box_hist -- one launch behind the guard, captured with the step); a frame the guard found lost or
    too thin stays out.  The histograms travel in the pose dict (box_hist) and the frame's read-out is recorded (pred_dict / pickle
    'box'); where a part's box is established it replaces the per-frame maximum in pred['corners'] and in the box IoUs.  None when
    absent or hold is not set; quantile has no default -- it depends on the trained network's outlier rate --, lies in [0.5, 1] and is
    a whole number of thousandths; radial: the x and z extents of a symmetric category from the radius sqrt(x^2 + z^2), which does
    not depend on the arbitrary in-plane angle (an error on any other category).
    -> {'quantile_permille', 'bins', 'min_points', 'radial'}."""
    s = cfg["track_cfg"].get("box")
    if s is None or not s.get("hold", False):
        return None
    q = s.get("quantile")
    if q is None:
        raise ValueError("track_cfg/box/hold needs track_cfg/box/quantile (the share of a part's points inside the box per axis, in "
                         "[0.5, 1]): it has no default")
    if isinstance(q, bool) or not isinstance(q, (int, float, np.integer, np.floating)) or not np.isfinite(q) or not 0.5 <= float(q) <= 1.0:
        raise ValueError(f"track_cfg/box/quantile must be a number in [0.5, 1], got {q!r}")
    permille = int(round(float(q) * 1000.0))
    if abs(float(q) * 1000.0 - permille) > 1e-6:
        raise ValueError(f"track_cfg/box/quantile must be a whole number of thousandths (the kernel's quantile is an integer per mille), got {q!r}")
    from .pose_utils.pose_fit import BOX_BINS
    bins, min_points = s.get("bins"), s.get("min_points")
    bins, min_points = 128 if bins is None else bins, 16 if min_points is None else min_points
    if isinstance(bins, bool) or int(bins) != bins or int(bins) not in BOX_BINS:
        raise ValueError(f"track_cfg/box/bins must be one of {BOX_BINS}, got {s.get('bins')!r}")
    if isinstance(min_points, bool) or int(min_points) != min_points or not 1 <= int(min_points) < 2 ** 31:
        raise ValueError(f"track_cfg/box/min_points must be an integer >= 1, got {s.get('min_points')!r}")
    radial = bool(s.get("radial", False))
    if radial and not cfg["obj_sym"]:
        raise ValueError(f"track_cfg/box/radial: the radial extent is for symmetric categories (obj_sym), category "
                         f"{cfg['obj_category']} is not one: its in-plane angle is part of the pose")
    return {"quantile_permille": permille, "bins": int(bins), "min_points": int(min_points), "radial": radial}


# The pose dict that travels from frame to frame: these three, with track_cfg/motion three more -- the pose the next step starts
# from and whether the dict's own pose is a measured result (a track's start is not) --, with track_cfg/size the three words of
# the size state and with track_cfg/box the box histograms.  The dict is the loop's whole state.
POSE_KEYS = ("rotation", "scale", "translation")
SIZE_KEYS = ("size_mean", "size_n", "size_miss")
BOX_KEY = "box_hist"


def entering_box(pose, box):
    """track_cfg/box: a dict without the histograms is a track's START -- empty ones, (B,P,3,bins) int32 zeros.  A dict that carries
    them passes through."""
    if BOX_KEY in pose:
        return pose
    import torch
    scale = pose["scale"]
    return {**pose, BOX_KEY: torch.zeros(tuple(scale.shape) + (3, box["bins"]), dtype=torch.int32, device=scale.device)}


def entering_size(pose, size):
    """track_cfg/size: a dict without the size state is a track's START -- the state is the start pose's scale counted as init_frames
    frames where it is finite and > 0, else empty (n = 0, mean = 0).  A dict that carries its state passes through."""
    if "size_mean" in pose:
        return pose
    import torch
    scale = pose["scale"].float()
    ok = torch.isfinite(scale) & (scale > 0)
    if size["init_frames"] == 0:
        ok = torch.zeros_like(ok)
    n = torch.where(ok, torch.full_like(scale, size["init_frames"], dtype=torch.int32), torch.zeros_like(scale, dtype=torch.int32))
    return {**pose, "size_mean": torch.where(ok, scale, torch.zeros_like(scale)), "size_n": n, "size_miss": torch.zeros_like(n)}


def entering_pose(pose):
    """track_cfg/motion: a dict with only the three keys is a track's START -- the prediction is the pose itself and nothing is
    measured yet, so frame 1 never extrapolates.  A dict that carries its prediction passes through."""
    if "next_rotation" in pose:
        return pose
    import torch
    return {**pose, "next_rotation": pose["rotation"], "next_translation": pose["translation"],
            "measured": torch.zeros(pose["scale"].shape, dtype=torch.int32, device=pose["scale"].device)}


def entering(pose, model):
    """The travelling dict of `model`'s options (its `motion` / `size` / `box` attributes; absent or None: off) for a pose entering a step."""
    if getattr(model, "motion", None) is not None:
        pose = entering_pose(pose)
    if getattr(model, "size", None) is not None:
        pose = entering_size(pose, model.size)
    if getattr(model, "box", None) is not None:
        pose = entering_box(pose, model.box)
    return pose


def start_pose(pose):
    """The pose a step starts from: the prediction where the dict carries one (scale has no velocity), else the dict itself."""
    if "next_rotation" not in pose:
        return pose
    start = {"rotation": pose["next_rotation"], "scale": pose["scale"], "translation": pose["next_translation"]}
    # (track_cfg/size, track_cfg/box: the state stays with the pose it belongs to)
    start.update((k, pose[k]) for k in SIZE_KEYS + (BOX_KEY,) if k in pose)
    return start


# ---- the records: name in pred_dict and the pickle (and of the model attribute that switches the option on) -> ... ---------------
# A step's records, (B,P) tensors per frame -> (the prefix its keys travel under inside CoordinateNet's maps, the keys)
STEP_RECORDS = {"guard": ("guard_", ("count", "inliers", "rms", "verdict")),     # pose_utils/pose_fit.py
                "st_fit": ("st_", ("inliers", "valid")),                         # int32
                "rot_pool": ("rot_", ("inliers", "count")),                      # int32
                # used int32, angle (degrees) / shift float32, and the predicted pose itself: (B,P,3,3), (B,P,3,1)
                "motion": ("motion_", ("used", "angle", "shift", "rotation", "translation")),
                # held / accepted int32, free = the frame's own scale float32, n = the frames in the mean after this one int32
                "size": ("size_", ("held", "accepted", "free", "n")),
                # extent = the held half-extents after the frame (0: not established), frame = the frame's own: (B,P,3) float32;
                # added = the frame's members, total = the values held per axis: int32
                "box": ("box_", ("extent", "frame", "added", "total"))}
# The host loop's records, ONE (B,) int32 tensor per frame (None: a frame without) -> the key that wraps it in the pickle.
# otf_thin: which trajectories' lists were thinned (its sum: the frame's thinned instances); depth_filter: the pixels set to 0
LOOP_RECORDS = {"otf_thin": "thinned", "depth_filter": "removed"}
# (and frame 0's one-off "image_fit": a flat dict of (B,) int32 tensors -- members, used, holes, inliers, valid;
#  and the trajectories' "camera": {'K' (B,3,3), 'depth_unit' (B,)} float64, present when a camera is in use)


def put_record(npcs_pred, name, values):
    """A step record's values into CoordinateNet's maps, under the record's prefix."""
    prefix, keys = STEP_RECORDS[name]
    npcs_pred.update((prefix + k, values[k]) for k in keys)


def commit_with_records(commit, records):
    """`commit` of a batch form, with the frame's step records taken out of CoordinateNet's maps: records = {name: {}} of the
    options that are on, filled as records[name][frame] = {key: tensor}."""
    def wrapped(i, result):
        npcs, pose = commit(i, result)
        for name, frames in records.items():
            prefix, keys = STEP_RECORDS[name]
            frames[i] = {k: npcs.pop(prefix + k) for k in keys}
        if "motion" in records or "size" in records or "box" in records:
            # a committed frame keeps the three keys; the prediction is in its record, the size state and the box histograms only
            # in the travelling dict
            pose = {k: pose[k] for k in POSE_KEYS}
        return npcs, pose
    return wrapped if records else commit


def records_to_numpy(pred_dict, guard_yaxis_only=False):
    """The result pickle's entries for the records `pred_dict` carries (none: {}), as numpy: a step record as [None, {key: (B,P)}, ...],
    a loop record as [None or {'thinned' / 'removed': (B,)}, ...], image_fit as a flat dict.  guard_yaxis_only: which test counted the
    guard's inliers -- one boolean per trajectory in the slot of frame 0 (None otherwise), so the frames' records keep their four keys."""
    to_np = lambda t: t.detach().cpu().numpy()
    out = {name: [None if r is None else {k: to_np(v) for k, v in r.items()} for r in pred_dict[name]] for name in STEP_RECORDS if name in pred_dict}
    if guard_yaxis_only and "guard" in out:
        out["guard"][0] = {"yaxis_only": np.ones(len(pred_dict["poses"][0]["scale"]), bool)}
    out.update({name: [None if r is None else {key: to_np(r)} for r in pred_dict[name]] for name, key in LOOP_RECORDS.items() if name in pred_dict})
    if "image_fit" in pred_dict:
        out["image_fit"] = {k: to_np(v) for k, v in pred_dict["image_fit"].items()}
    if "camera" in pred_dict:           # (host arrays already: K (B,3,3), depth_unit (B,))
        out["camera"] = {k: np.asarray(v, np.float64) for k, v in pred_dict["camera"].items()}
    return out
