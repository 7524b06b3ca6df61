"""On-the-fly ball crop + resample of a depth frame, on the device.

Real NOCS tracking (`--nocs_otf True` in every scripts/track/nocs/*.sh of the reference) re-crops every frame around the
pose predicted for the previous one: project the ball's bounding box into the image, back-project the depth pixels inside
it, keep the points within `radius` of the predicted centre, duplicate-pad / randomly thin to at most 5 x num_points,
furthest-point-sample num_points of them, and derive labels and ground-truth NOCS (reference
datasets/nocs_data/nocs_data_process.py:92-109, 121-163, 43-50, 227-236; nocs_utils.py:5-43; data_utils.py:138-157;
called from network/models/model.py:425-452).  The reference does this in numpy on the host with a GPU round trip for the
FPS; here the frame's depth and mask stay on the device, the arithmetic is torch float64 exactly as numpy's, the
furthest-point sampling is captra_fps_gather, and the host only sees three scalars (pixel / point counts).

Ordering contract (it decides which point FPS starts from): candidate pixels in row-major image order, ball members in
that order, duplication by whole-list doubling, the > 5 x num_points thinning by `numpy.random.permutation` (drawn on the
host from numpy's global generator, as the reference does, so that seeded runs agree) -- or, opt-in, on the device by a rule
of this build's own (full_data_batch_arrays' `thin`, include/captra_hip.h: captra_otf_thin).
"""
from __future__ import annotations

import numpy as np
import torch

def to_host(t: torch.Tensor) -> np.ndarray:
    """Device -> host through pinned memory and an event on the CURRENT stream.  A plain `.cpu()` lands in pageable memory,
    which the runtime serves with a staged copy that waits for the whole device — with two lanes of trajectories on two
    streams that wait is what kept one lane's sampler from running under the other lane's networks."""
    if not t.is_cuda:
        return t.numpy()
    buf = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    buf.copy_(t, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(t.device))
    ev.synchronize()
    return buf.numpy()


def to_device(a, dev, dtype=None) -> torch.Tensor:
    """Host array -> device through pinned memory, asynchronously on the current stream (same reason as to_host)."""
    t = torch.as_tensor(np.ascontiguousarray(a)) if not isinstance(a, torch.Tensor) else a
    if dtype is not None:
        t = t.to(dtype)
    if torch.device(dev).type != "cuda":
        return t.to(dev)
    return t.pin_memory().to(dev, non_blocking=True)


NOCS_REAL_INTRINSICS = np.array([[591.0125, 0.0, 322.525], [0.0, 590.16775, 244.11084], [0.0, 0.0, 1.0]])   # nocs_data_process.py:20


NOCS_CAMERA_INTRINSICS = np.array([[577.5, 0.0, 319.5], [0.0, 577.5, 239.5], [0.0, 0.0, 1.0]])             # get_gt_poses.py:100-102 (CAMERA25)
CAMERA_PRESETS = {"nocs_real": (NOCS_REAL_INTRINSICS, 0.001), "nocs_camera": (NOCS_CAMERA_INTRINSICS, 0.001)}
CAM_ROW = 19              # doubles per row of a camera table: K row-major (9), K^-1 row-major (9), depth_unit (1)


def check_camera(K, depth_unit, prefix: str = "camera/") -> tuple:
    """A camera as (K (3,3) float64, depth_unit float), or a ValueError that names the entry outside the model (`prefix`: where the
    caller read it): K finite with last row 0 0 1 and fx, fy > 0; depth_unit = metres per depth count, finite and > 0."""
    K = np.asarray(K, np.float64)
    if K.shape != (3, 3):
        raise ValueError(f"{prefix}K must be a 3x3 matrix, got shape {K.shape}")
    for key, (r, c) in (("fx", (0, 0)), ("skew", (0, 1)), ("cx", (0, 2)), ("fy", (1, 1)), ("cy", (1, 2))):
        if not np.isfinite(K[r, c]):
            raise ValueError(f"{prefix}{key} must be finite, got {K[r, c]!r}")
    for key, v in (("fx", K[0, 0]), ("fy", K[1, 1])):
        if not v > 0:
            raise ValueError(f"{prefix}{key} must be > 0, got {v!r}")
    if not np.isfinite(K[1, 0]) or K[1, 0] != 0.0:
        raise ValueError(f"{prefix}K[1][0] must be 0 (the model has one skew term, K[0][1]), got {K[1, 0]!r}")
    if not np.array_equal(K[2], [0.0, 0.0, 1.0]):
        raise ValueError(f"{prefix}K's last row must be 0 0 1, got {K[2].tolist()}")
    try:
        unit = float(depth_unit)
    except (TypeError, ValueError):
        raise ValueError(f"{prefix}depth_unit must be a number (metres per depth count), got {depth_unit!r}") from None
    if not (np.isfinite(unit) and unit > 0):
        raise ValueError(f"{prefix}depth_unit must be finite and > 0 (metres per depth count), got {depth_unit!r}")
    return K, unit


def camera_rows(K, depth_unit, prefix: str = "camera/") -> tuple:
    """Per-trajectory cameras K (B,3,3), depth_unit (B,) -> (table (C,19) float64, cam_of (B,) int32) on the HOST: the cameras
    de-duplicated by their bytes (K and unit), in order of first appearance; row = K, K^-1 (by _kinv), depth_unit."""
    K = np.asarray(K, np.float64)
    if K.ndim != 3 or K.shape[1:] != (3, 3):
        raise ValueError(f"{prefix}K must be (B,3,3), one matrix per trajectory, got shape {K.shape}")
    unit = np.asarray(depth_unit, np.float64).reshape(-1)
    if unit.shape[0] != K.shape[0]:
        raise ValueError(f"{prefix}depth_unit must be (B,) with B = {K.shape[0]} as K, got shape {np.shape(depth_unit)}")
    rows, index, cam_of = [], {}, np.empty(K.shape[0], np.int32)
    for b in range(K.shape[0]):
        Kb, ub = check_camera(K[b], unit[b], prefix)
        key = Kb.tobytes() + np.float64(ub).tobytes()
        if key not in index:
            index[key] = len(rows)
            rows.append(np.concatenate([Kb.reshape(9), _kinv(Kb), [ub]]))
        cam_of[b] = index[key]
    table = np.stack(rows) if rows else np.zeros((0, CAM_ROW), np.float64)
    return np.ascontiguousarray(table, np.float64), cam_of


def camera_table(K, depth_unit, dev, prefix: str = "camera/") -> tuple:
    """The `cameras` argument of full_data_batch_arrays / image_members from per-trajectory K (B,3,3) and depth_unit (B,): camera_rows'
    table and cam_of as device tensors, in ONE upload (the int32 indices ride behind the doubles)."""
    table, cam_of = camera_rows(K, depth_unit, prefix)
    C, B = table.shape[0], cam_of.shape[0]
    blob = np.empty(8 * CAM_ROW * C + 4 * B, np.uint8)
    blob[:8 * CAM_ROW * C].view(np.float64)[:] = table.reshape(-1)
    blob[8 * CAM_ROW * C:].view(np.int32)[:] = cam_of
    d = to_device(blob, dev)
    return d[:8 * CAM_ROW * C].view(torch.float64).view(C, CAM_ROW), d[8 * CAM_ROW * C:].view(torch.int32)


def _check_cameras(cameras, B: int, dev) -> tuple:
    """(table, cam_of) as the *_cam entry points read them, or a ValueError."""
    table, cam_of = cameras
    if (not torch.is_tensor(table) or table.dtype != torch.float64 or table.dim() != 2 or table.shape[1] != CAM_ROW or table.shape[0] < 1
            or not table.is_contiguous()):
        raise ValueError(f"cameras: the table is a contiguous float64 tensor (C,{CAM_ROW}) with C >= 1 (camera_table builds it), got "
                         f"{getattr(table, 'dtype', type(table))} {tuple(getattr(table, 'shape', ()))}")
    if not torch.is_tensor(cam_of) or cam_of.dtype != torch.int32 or tuple(cam_of.shape) != (B,):
        raise ValueError(f"cameras: cam_of is an int32 tensor (B,) with B = {B}, one camera row per trajectory, got "
                         f"{getattr(cam_of, 'dtype', type(cam_of))} {tuple(getattr(cam_of, 'shape', ()))}")
    if table.device != dev or cam_of.device != dev:
        raise ValueError(f"cameras: the table and cam_of live on the frames' device {dev}, got {table.device} and {cam_of.device}")
    return table, cam_of.contiguous()


def proj_corners(height: int, width: int, center, radius: float, intrinsics=NOCS_REAL_INTRINSICS) -> np.ndarray:
    """Image-space bounding box [[row_min, col_min], [row_max, col_max]] (inclusive, clamped) of the axis-aligned cube of
    half-size max(radius, 0.05) around `center` (camera frame, metres, looking down -z); nocs_data_process.py:136-148."""
    radius = max(float(radius), 0.05)
    c = np.asarray(center, np.float64).reshape(3)
    lo, hi = c - radius, c + radius
    box = np.array([[x, y, z] for y in (lo[1], hi[1]) for x in (lo[0], hi[0]) for z in (lo[2], hi[2])], np.float64) * 1000.0
    homog = -box / box[:, 2:3]
    homog[:, 2] = -homog[:, 2]
    uv = (np.asarray(intrinsics, np.float64) @ homog.T).T[:, :2].astype(np.int32)
    rows, cols = height - uv[:, 1], uv[:, 0]
    out = np.array([[rows.min(), cols.min()], [rows.max(), cols.max()]], np.int64)
    out[0] = np.maximum(out[0], 0)
    out[1] = np.minimum(out[1], np.array([height - 1, width - 1]))
    return out


def proj_corners_batch(height: int, width: int, centers, radii, intrinsics=NOCS_REAL_INTRINSICS) -> np.ndarray:
    """proj_corners for B instances at once -> (B, 2, 2) int64.  Same float64 operations per instance; the 3x3 projection is
    written out (u = K00 x + K01 y + K02 z, ... with z = 1 after the homogeneous division), so nothing depends on how a BLAS
    orders a 3-term sum."""
    c = np.asarray(centers, np.float64).reshape(-1, 3)
    r = np.maximum(np.asarray(radii, np.float64).reshape(-1, 1), 0.05)
    lo, hi = c - r, c + r
    sel = np.array([[x, y, z] for y in (0, 1) for x in (0, 1) for z in (0, 1)])                 # the 8 corners: lo / hi per axis
    box = np.where(sel[None] == 0, lo[:, None, :], hi[:, None, :]) * 1000.0                       # (B, 8, 3)
    homog = -box / box[:, :, 2:3]
    homog[:, :, 2] = -homog[:, :, 2]
    K = np.asarray(intrinsics, np.float64)
    u = (K[0, 0] * homog[:, :, 0] + K[0, 1] * homog[:, :, 1]) + K[0, 2] * homog[:, :, 2]
    v = (K[1, 0] * homog[:, :, 0] + K[1, 1] * homog[:, :, 1]) + K[1, 2] * homog[:, :, 2]
    rows, cols = height - v.astype(np.int32), u.astype(np.int32)
    out = np.stack([np.stack([rows.min(1), cols.min(1)], -1), np.stack([rows.max(1), cols.max(1)], -1)], 1).astype(np.int64)
    out[:, 0] = np.maximum(out[:, 0], 0)
    out[:, 1] = np.minimum(out[:, 1], np.array([height - 1, width - 1]))
    return out


_KINV_CACHE: dict = {}


def _kinv(intrinsics) -> np.ndarray:
    """Inverse intrinsics as 9 doubles (cached per matrix: numpy.linalg.inv costs 30 us of the loop's critical host path)."""
    K = np.asarray(intrinsics, np.float64)
    key = K.tobytes()
    if key not in _KINV_CACHE:
        _KINV_CACHE[key] = np.linalg.inv(K).reshape(9)
    return _KINV_CACHE[key]


def _device_fps(points_f32: torch.Tensor, num: int) -> torch.Tensor:
    from . import fused
    res = fused.fps_gather(points_f32.reshape(1, -1, 3).contiguous(), num)
    if res is None:   # beyond the register-resident kernel: the drop-in op
        from .pointnet_lib import pointnet2_utils as pn
        return pn.furthest_point_sample(points_f32.reshape(1, -1, 3).contiguous(), num).reshape(-1).long()
    return res[0].reshape(-1).long()


def crop_candidates(depth: torch.Tensor, mask: torch.Tensor, center, radius: float, num_points: int,
                    intrinsics=NOCS_REAL_INTRINSICS, _depth_retry: int = 0, depth_unit: float = 0.001):
    """Everything of the crop BEFORE the furthest-point sampling (nocs_data_process.py:92-109, 151-163;
    data_utils.py:146-152): -> (pts (n,3) float64 back-projected pixels, raw_mask (n,) bool, idx (c,) long = the ball
    members, list-doubled up to num_points, perm (5*num_points,) long or None = the thinning of an over-long list).
    The cloud handed to the sampler is pts[idx] (or pts[idx][perm]) as float32.  depth_unit: metres per depth count (the
    camera model; 0.001 = the reference's millimetres)."""
    H, W = depth.shape
    dev = depth.device
    box = proj_corners(H, W, center, radius, intrinsics)
    r0, c0, r1, c1 = int(box[0, 0]), int(box[0, 1]), int(box[1, 0]), int(box[1, 1])
    sub = depth[r0:r1 + 1, c0:c1 + 1]
    rc = torch.nonzero(sub > 0)                                   # row-major, like numpy.where
    rows, cols = rc[:, 0] + r0, rc[:, 1] + c0
    kinv = torch.from_numpy(np.linalg.inv(np.asarray(intrinsics, np.float64))).to(dev)
    grid = torch.stack([cols.double(), (H - rows).double(), torch.ones_like(cols, dtype=torch.float64)], dim=0)
    xyz = (kinv @ grid).t()                                        # (n,3) float64
    z = depth[rows, cols].float().double()
    pts = xyz * z[:, None] / xyz[:, 2:3]
    pts = torch.stack([pts[:, 0], pts[:, 1], -pts[:, 2]], dim=1) * float(depth_unit)
    raw_mask = mask[rows, cols].bool()

    c = torch.as_tensor(np.asarray(center, np.float64).reshape(1, 3), device=dev)
    dist = torch.sqrt(((pts - c) ** 2).sum(dim=-1))
    rad = max(float(radius), 0.05)
    idx = torch.empty(0, dtype=torch.long, device=dev)
    for _ in range(10):
        idx = torch.nonzero(dist <= rad).reshape(-1)
        if idx.numel() >= 10:
            break
        rad *= 1.10
    if idx.numel() == 0:
        idx = torch.arange(dist.numel(), device=dev)
    if idx.numel() == 0:
        if _depth_retry > 20:
            raise RuntimeError("crop_ball_from_depth: no valid depth pixel anywhere near the predicted centre")
        return crop_candidates(depth, mask, center, float(radius) * 1.2, num_points, intrinsics, _depth_retry + 1, depth_unit)
    while idx.numel() < num_points:
        idx = torch.cat([idx, idx])
    perm = None
    if idx.numel() > 5 * num_points:                                # data_utils.py:146-152
        perm = torch.from_numpy(np.random.permutation(idx.numel())[:5 * num_points]).to(dev)
    return pts, raw_mask, idx, perm


def _candidate_cloud(pts, idx, perm) -> torch.Tensor:
    cand = pts[idx]
    return (cand[perm] if perm is not None else cand).float()


def crop_ball_from_depth(depth: torch.Tensor, mask: torch.Tensor, center, radius: float, num_points: int,
                         intrinsics=NOCS_REAL_INTRINSICS, fps_fn=_device_fps):
    """depth (H,W) integer millimetres, mask (H,W) bool (the tracked instance), both on the compute device
    -> (points (num_points,3) float64 camera frame, obj_mask (num_points,) bool).  nocs_data_process.py:92-109, 151-163."""
    pts, raw_mask, idx, perm = crop_candidates(depth, mask, center, radius, num_points, intrinsics)
    picked = fps_fn(_candidate_cloud(pts, idx, perm), num_points)
    idx = idx[perm[picked] if perm is not None else picked]
    return pts[idx], raw_mask[idx]


def _full_data(pts, obj, gt_pose: dict) -> dict:
    dev = pts.device
    rot = torch.as_tensor(np.asarray(gt_pose["rotation"], np.float64).reshape(3, 3), device=dev)
    trans = torch.as_tensor(np.asarray(gt_pose["translation"], np.float64).reshape(1, 3), device=dev)
    scale = float(np.asarray(gt_pose["scale"], np.float64).reshape(-1)[0])
    nocs = torch.zeros_like(pts)
    nocs[obj] = ((pts[obj] - trans) / scale) @ rot
    return {"points": pts, "labels": 1 - obj.long(), "nocs": nocs}


def full_data_from_depth(depth, mask, center, radius, gt_pose: dict, num_points: int, intrinsics=NOCS_REAL_INTRINSICS,
                         fps_fn=_device_fps) -> dict:
    """-> {'points' (N,3), 'labels' (N,) (0 = object, 1 = background), 'nocs' (N,3)} float64 / int64 device tensors;
    gt_pose {'rotation' (3,3), 'translation' (3,1), 'scale' ()} of the instance (nocs_data_process.py:43-50, 227-236)."""
    pts, obj = crop_ball_from_depth(depth, mask, center, radius, num_points, intrinsics, fps_fn)
    return _full_data(pts, obj, gt_pose)


CROP_CAP = 65536          # ball members kept per instance by the crop kernel (more: that instance takes the torch path)


def _full_data_batch_torch(frames, num_points: int, intrinsics) -> list:
    """full_data_batch with the candidate extraction in torch ops, one instance after the other (the restatement the crop
    kernel is tested against); the sampling is already one ragged launch."""
    from . import fused
    cands = [crop_candidates(d, m, c, r, num_points, intrinsics) for d, m, c, r, _ in frames]
    clouds = [_candidate_cloud(p, i, pm) for p, _, i, pm in cands]
    counts = [int(c.shape[0]) for c in clouds]
    dev = clouds[0].device
    padded = torch.zeros(len(clouds), max(counts), 3, dtype=torch.float32, device=dev)
    for b, c in enumerate(clouds):
        padded[b, :counts[b]] = c
    res = fused.fps_gather(padded, num_points, n_per_cloud=torch.tensor(counts, dtype=torch.int32, device=dev))
    out = []
    for b, ((pts, raw_mask, idx, perm), frame) in enumerate(zip(cands, frames)):
        picked = res[0][b].long() if res is not None else _device_fps(clouds[b], num_points)
        sel = idx[perm[picked] if perm is not None else picked]
        out.append(_full_data(pts[sel], raw_mask[sel], frame[4]))
    return out


def stack_full_data(items: list) -> dict:
    """list of per-instance dicts -> {'points' (B,N,3), 'labels' (B,N), 'nocs' (B,N,3)}."""
    return {k: torch.stack([it[k] for it in items]) for k in ("points", "labels", "nocs")}


def full_data_batch(frames, num_points: int, intrinsics=NOCS_REAL_INTRINSICS, use_kernel: bool = True, stacked: bool = False):
    """The re-crop of ALL trajectories of a tracking step: one crop launch (captra_crop_ball, a workgroup per instance),
    one host round trip for the member counts, one furthest-point-sampling launch (captra_fps_gather_ragged).
    frames: list of (depth, mask, center, radius, gt_pose) -> list of full_data_from_depth's dicts, as if it had been
    called once per trajectory in list order (the thinning permutations are drawn in that order; nothing else draws).
    Instances on a rare path — fewer than 10 ball members (radius growth), more than CROP_CAP — take the torch path.
    stacked=True returns one dict of (B, …) tensors instead of the list (no per-instance slicing when nothing was rare)."""
    dev = frames[0][0].device
    if not use_kernel or dev.type != "cuda":
        res = _full_data_batch_torch(frames, num_points, intrinsics)
        return stack_full_data(res) if stacked else res
    gt = {"rotation": np.stack([np.asarray(f[4]["rotation"], np.float64).reshape(3, 3) for f in frames]),
          "translation": np.stack([np.asarray(f[4]["translation"], np.float64).reshape(3) for f in frames]),
          "scale": np.array([float(np.asarray(f[4]["scale"], np.float64).reshape(-1)[0]) for f in frames])}
    return full_data_batch_arrays(torch.stack([f[0] for f in frames]), torch.stack([f[1] for f in frames]),
                                  np.stack([np.asarray(f[2], np.float64).reshape(3) for f in frames]),
                                  np.array([float(f[3]) for f in frames], np.float64), gt, num_points, intrinsics, stacked)


_KMAT_DEV: dict = {}


def _intrinsics_on_device(intrinsics, dev) -> torch.Tensor:
    """[K (9 doubles), K^-1 (9 doubles)] on the device, uploaded once per (matrix, device)."""
    K = np.asarray(intrinsics, np.float64)
    key = (K.tobytes(), str(dev))
    if key not in _KMAT_DEV:
        _KMAT_DEV[key] = torch.from_numpy(np.concatenate([K.reshape(9), _kinv(intrinsics)])).to(dev)
    return _KMAT_DEV[key]


_ARANGE: dict = {}


def _arange(n: int, dev) -> torch.Tensor:
    key = (n, str(dev))
    if key not in _ARANGE:
        _ARANGE[key] = torch.arange(n, device=dev)
    return _ARANGE[key]


DET_KEYS = ("det_boxes", "det_class", "det_count", "det_masks")


def check_depth_filter_params(window, abs_mm, rel_permille, min_support, prefix: str = "") -> tuple:
    """The four parameters of captra_depth_support_filter as ints, or a ValueError that names the one outside the kernel's range
    (`prefix`: where the caller read them, e.g. 'track_cfg/depth_filter/').  abs_mm is in DEPTH COUNTS: millimetres for a millimetre
    sensor (the name's origin), `abs_mm * depth_unit` metres under a camera whose depth unit is not 0.001."""
    vals = {}
    for key, v in (("window", window), ("abs_mm", abs_mm), ("rel_permille", rel_permille), ("min_support", min_support)):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"{prefix}{key} must be an integer, got {v!r}")
        vals[key] = int(v)
    if vals["window"] not in (1, 2, 3):
        raise ValueError(f"{prefix}window must be 1, 2 or 3 (a square of 3, 5 or 7 pixels), got {vals['window']}")
    if not 0 <= vals["abs_mm"] <= 2 ** 31 - 1:
        raise ValueError(f"{prefix}abs_mm (millimetres) must be in [0, 2^31 - 1], got {vals['abs_mm']}")
    if not 0 <= vals["rel_permille"] <= 1000:
        raise ValueError(f"{prefix}rel_permille must be in [0, 1000], got {vals['rel_permille']}")
    most = (2 * vals["window"] + 1) ** 2 - 1
    if not 1 <= vals["min_support"] <= most:
        raise ValueError(f"{prefix}min_support must be in [1, {most}] (the other pixels of a window of {vals['window']}), got {vals['min_support']}")
    return vals["window"], vals["abs_mm"], vals["rel_permille"], vals["min_support"]


def depth_support_filter(depth: torch.Tensor, window: int, abs_mm: int, rel_permille: int, min_support: int):
    """Flying-pixel rejection on depth images (include/captra_hip.h: captra_depth_support_filter, where the rule is stated): a pixel
    with depth d > 0 is kept when at least `min_support` of the other in-image pixels of the (2 window + 1)^2 square around it have a
    depth within abs_mm + floor(d rel_permille / 1000) millimetres of d, else set to 0; pixels with d <= 0 pass through.
    depth: (B,H,W) or (H,W) int32 on the device, contiguous.  -> (filtered depth, a new tensor of depth's shape; removed: int32 (B,)
    on the device, the pixels of each image set to 0 -- for an (H,W) image a 0-dim tensor).  One launch, nothing visits the host."""
    from . import _lib as L
    L.require_device(depth)
    if depth.dtype != torch.int32 or depth.dim() not in (2, 3):
        raise ValueError(f"depth_support_filter takes an int32 tensor (B,H,W) or (H,W), got {depth.dtype} {tuple(depth.shape)}")
    window, abs_mm, rel_permille, min_support = check_depth_filter_params(window, abs_mm, rel_permille, min_support)
    B, H, W = (1, *depth.shape) if depth.dim() == 2 else depth.shape
    out = torch.empty_like(depth)
    removed = torch.zeros(B, dtype=torch.int32, device=depth.device)
    with torch.cuda.device(depth.device):
        L.call("captra_depth_support_filter", B, H, W, window, abs_mm, rel_permille, min_support, L.ptr(depth), L.ptr(out), L.ptr(removed))
    return out, (removed.reshape(()) if depth.dim() == 2 else removed)


IMAGE_FIT_CAP = 16384           # the most members captra_part_fit_ransac takes


def check_image_fit_params(cap, border, prefix: str = "") -> tuple:
    """cap and border of image_members as ints, or a ValueError that names the one outside its range (`prefix`: where the caller read
    them, e.g. 'init_frame/')."""
    vals = {}
    for key, v in (("cap", cap), ("border", border)):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"{prefix}{key} must be an integer, got {v!r}")
        vals[key] = int(v)
    if not 3 <= vals["cap"] <= IMAGE_FIT_CAP:
        raise ValueError(f"{prefix}cap must be in [3, {IMAGE_FIT_CAP}] (a fit needs three members, the fit kernel takes {IMAGE_FIT_CAP}), got {vals['cap']}")
    if not 0 <= vals["border"] <= 3:
        raise ValueError(f"{prefix}border must be in [0, 3] (pixels eroded from the mask), got {vals['border']}")
    return vals["cap"], vals["border"]


def image_members(depth: torch.Tensor, mask: torch.Tensor, coord: torch.Tensor, intrinsics=NOCS_REAL_INTRINSICS, cap: int = IMAGE_FIT_CAP,
                  border: int = 0, negate_z: bool = False, cameras=None) -> dict:
    """The correspondences of a first-pose fit from a frame's images (include/captra_hip.h: captra_image_members, where the rule is
    stated): the pixels of the instance mask, eroded by `border`, that carry a depth, in row-major order, at most `cap` of them (a
    fixed stride thins a larger instance), back-projected and paired with the NOCS coordinates the coordinate image encodes.
    depth (B,H,W) int32 millimetres, mask (B,H,W) bool or uint8, coord (B,H,W,3) uint8 (channel k = NOCS axis k), all on the device
    and contiguous; (H,W) / (H,W,3) for one image.
    -> {'src' (B,1,3,cap) fp32, 'tgt' (B,3,cap) fp32 metres, 'labels' (B,cap) int32 (0 = a member, -1 = an empty slot), 'pix' (B,cap)
    int32, 'counts' (B,3) int32 = members, used, holes}: what part_fit_ransac_cn(labels, src, tgt) reads.  One launch, nothing
    visits the host.
    `cameras` = (table (C,19) float64, cam_of (B,) int32) device tensors (camera_table): image i is back-projected with the K^-1 and
    the depth unit of camera cam_of[i] (captra_image_members_cam), `intrinsics` is not read and the depth is in that camera's counts.
    None: the call as it always was."""
    from . import _lib as L
    L.require_device(depth, mask, coord)
    single = depth.dim() == 2
    if single:
        depth, mask, coord = depth[None], mask[None], coord[None]
    if depth.dtype != torch.int32 or depth.dim() != 3:
        raise ValueError(f"image_members takes the depth as an int32 tensor (B,H,W) or (H,W), got {depth.dtype} {tuple(depth.shape)}")
    if mask.dtype not in (torch.bool, torch.uint8) or mask.shape != depth.shape:
        raise ValueError(f"image_members takes the mask as a bool or uint8 tensor of the depth's shape {tuple(depth.shape)}, got {mask.dtype} {tuple(mask.shape)}")
    if coord.dtype != torch.uint8 or coord.shape != (*depth.shape, 3):
        raise ValueError(f"image_members takes the coordinate image as a uint8 tensor {(*depth.shape, 3)}, got {coord.dtype} {tuple(coord.shape)}")
    if not (mask.device == depth.device == coord.device):
        raise ValueError("image_members takes its three images on one device")
    cap, border = check_image_fit_params(cap, border)
    B, H, W = depth.shape
    dev = depth.device
    if cameras is not None:
        cam_table, cam_of = _check_cameras(cameras, B, dev)
    else:
        kinv = _intrinsics_on_device(intrinsics, dev)[9:]
    out = {"src": torch.empty(B, 1, 3, cap, dtype=torch.float32, device=dev), "tgt": torch.empty(B, 3, cap, dtype=torch.float32, device=dev),
           "labels": torch.empty(B, cap, dtype=torch.int32, device=dev), "pix": torch.empty(B, cap, dtype=torch.int32, device=dev),
           "counts": torch.zeros(B, 3, dtype=torch.int32, device=dev)}
    with torch.cuda.device(dev):
        if cameras is not None:
            L.call("captra_image_members_cam", B, H, W, cap, border, 1 if negate_z else 0, L.ptr(depth), L.ptr(mask.view(torch.uint8)), L.ptr(coord),
                   cam_table.shape[0], L.ptr(cam_table), L.ptr(cam_of), L.ptr(out["src"]), L.ptr(out["tgt"]), L.ptr(out["labels"]), L.ptr(out["pix"]),
                   L.ptr(out["counts"]))
        else:
            L.call("captra_image_members", B, H, W, cap, border, 1 if negate_z else 0, L.ptr(depth), L.ptr(mask.view(torch.uint8)), L.ptr(coord),
                   L.ptr(kinv), L.ptr(out["src"]), L.ptr(out["tgt"]), L.ptr(out["labels"]), L.ptr(out["pix"]), L.ptr(out["counts"]))
    if H * W == 0:                      # images without a pixel: the call has nothing to do and writes nothing
        out["src"].zero_(); out["tgt"].zero_(); out["labels"].fill_(-1); out["pix"].fill_(-1)
    return {k: v[0] for k, v in out.items()} if single else out


def full_data_batch_arrays(depth, mask, centers, radii_in, gt, num_points: int, intrinsics=NOCS_REAL_INTRINSICS, stacked: bool = True,
                           pose_dev=None, gt_dev=None, defer=None, mean=None, det=None, thin=None, cameras=None):
    """full_data_batch on already-stacked inputs (the track loop's form: no per-trajectory Python on the frame's critical
    path): depth (B,H,W), mask (B,H,W) device tensors; centers (B,3), radii_in (B,) float64 host arrays (radius as handed to
    full_data_from_depth: clamped to 0.05 inside); gt = {'rotation' (B,3,3), 'translation' (B,3), 'scale' (B,)} float64 host arrays.
    `pose_dev` = (translation (B,3) fp32, scale (B,) fp32, radius_factor) ON THE DEVICE instead of centers / radii_in (pass None
    for both): the crop's box, centre and radius are then derived there (captra_crop_box: the same float64 operations) and the
    pose never visits the host -- the stage's ONE round trip is the member counts.  `gt_dev`: the same three arrays as float64 DEVICE
    tensors (uploaded once with the trajectory), used instead of three uploads per frame.
    `defer` (with pose_dev; an int = upper bound of the candidate lists' length): NO round trip at all -- see the branch below; the
    result is then {'points_cn' (B,3,N) fp32 = points - `mean` (B,3), 'labels' (B,N), 'nocs_cn' (B,3,N) fp32, '_info'}: the
    frame's tensors in the networks' layouts (captra_otf_finish) and the device int32 word [a rare-path instance was met, longest
    list, ..] for the caller to read a frame late.
    `det` (with pose_dev) = the detector route (reference nocs_data_process.py:206-229, `nocs2d_label`): {'det_boxes' (B,K,4) int32
    [y1,x1,y2,x2], 'det_class' (B,K) int32, 'det_count' (B,) int32, 'det_masks' (B,K,H,W) uint8, 'category' int} device tensors -- every
    trajectory crops with the mask of the detection of its category that overlaps its (grown) box best (captra_crop_box_det selects,
    captra_crop_ball_det reads that mask: two launches in place of two, nothing visits the host), `mask` where there is none.
    `thin` = (seed, frame, b0) (on the device only): a list of more than 5 num_points members is thinned ON THE DEVICE by
    captra_otf_thin's rule (include/captra_hip.h: a counter-based draw keyed by seed, trajectory b0 + row and frame; the kept members
    in ascending order -- NOT the reference's permutation) instead of by numpy.random.permutation, in both stages: with `defer` the
    launch sits between the crop and the candidate launch and such an instance is no rare-path instance; on the synchronous stage the
    same launch fills the row's table and nothing is drawn from numpy for it, so both stages produce the same clouds bit for bit.
    Instances on the torch path (fewer than 10 members or more than CROP_CAP: crop_candidates) keep the host's permutation.  The
    stacked results then carry '_thinned' (B,) int32: which instances were thinned.
    `cameras` = (table (C,19) float64, cam_of (B,) int32) device tensors (camera_table): the camera model -- trajectory i is projected
    and back-projected with camera cam_of[i]'s K, K^-1 and depth unit in every branch (the *_cam entry points, include/captra_hip.h;
    the host-box branch projects each row with its own K; a rare-path instance's torch path takes its K and unit), `intrinsics` is
    not read and the depth images are in their cameras' counts.  None: the calls as they always were, bit for bit."""
    from . import _lib as L, fused
    dev = depth.device
    if thin is not None and dev.type != "cuda":
        raise ValueError("thinning on the device (thin=(seed, frame, b0)) needs the frame on the device")
    B = depth.shape[0]
    depth = depth.to(torch.int32).contiguous()
    mask = mask.to(torch.uint8).contiguous()
    _, H, W = depth.shape
    cam_table = cam_of = cams_h = None
    if cameras is not None:
        if dev.type != "cuda":
            raise ValueError("the camera model of the re-crop (cameras=(table, cam_of)) runs on the device: it needs the frames there")
        cam_table, cam_of = _check_cameras(cameras, B, dev)
        ncam = int(cam_table.shape[0])

    def cameras_on_host():
        """(K (B,3,3), depth_unit (B,)) of the rows, fetched once: the host-box branch and the rare path's torch restatement."""
        nonlocal cams_h
        if cams_h is None:
            t = to_host(cam_table)[np.clip(to_host(cam_of), 0, ncam - 1)]
            cams_h = (t[:, :9].reshape(B, 3, 3).copy(), t[:, 18].copy())
        return cams_h

    if det is not None:
        if pose_dev is None or dev.type != "cuda":
            raise ValueError("the detector route of the re-crop selects its masks on the device: it takes the pose as `pose_dev`")
        det_boxes = det["det_boxes"].to(torch.int32).contiguous()
        K = det_boxes.shape[1]
        det_class = det["det_class"].to(torch.int32).contiguous()
        det_count = det["det_count"].to(torch.int32).contiguous()
        det_masks = det["det_masks"].to(torch.uint8).contiguous()
        if (tuple(det_boxes.shape) != (B, K, 4) or tuple(det_class.shape) != (B, K) or tuple(det_count.shape) != (B,)
                or tuple(det_masks.shape) != (B, K, H, W)):
            raise ValueError(f"detections of a frame: det_boxes (B,K,4), det_class (B,K), det_count (B,), det_masks (B,K,H,W) with B = {B}, "
                             f"H x W = {H} x {W}; got {tuple(det_boxes.shape)}, {tuple(det_class.shape)}, {tuple(det_count.shape)}, {tuple(det_masks.shape)}")
    pts = torch.empty(B, CROP_CAP, 3, dtype=torch.float64, device=dev)
    obj = torch.empty(B, CROP_CAP, dtype=torch.uint8, device=dev)
    pix = torch.empty(B, CROP_CAP, dtype=torch.int32, device=dev)
    counts = torch.empty(B, 2, dtype=torch.int32, device=dev)
    if pose_dev is not None:
        trans_d, scale_d, factor = pose_dev
        trans_d = trans_d.reshape(B, 3).float().contiguous()
        scale_d = scale_d.reshape(B).float().contiguous()
        kk = _intrinsics_on_device(intrinsics, dev)
        box_d = torch.empty(B, 4, dtype=torch.int32, device=dev)
        ctr_d = torch.empty(B, 3, dtype=torch.float64, device=dev)
        rad_d = torch.empty(B, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            if det is not None:
                raw_d = torch.empty(B, dtype=torch.float64, device=dev)
                sel_d = torch.empty(B, dtype=torch.int32, device=dev)
            if cameras is not None and det is not None:
                L.call("captra_crop_box_det_cam", B, H, W, K, int(det["category"]), float(factor), L.ptr(trans_d), L.ptr(scale_d), ncam, L.ptr(cam_table),
                       L.ptr(cam_of), L.ptr(det_boxes), L.ptr(det_class), L.ptr(det_count), L.ptr(box_d), L.ptr(ctr_d), L.ptr(rad_d), L.ptr(raw_d),
                       L.ptr(sel_d))
                L.call("captra_crop_ball_det_cam", B, H, W, CROP_CAP, K, L.ptr(depth), L.ptr(mask), L.ptr(det_masks), L.ptr(sel_d), L.ptr(box_d),
                       L.ptr(ctr_d), L.ptr(rad_d), ncam, L.ptr(cam_table), L.ptr(cam_of), L.ptr(pts), L.ptr(obj), L.ptr(pix), L.ptr(counts))
            elif cameras is not None:
                L.call("captra_crop_box_cam", B, H, W, float(factor), L.ptr(trans_d), L.ptr(scale_d), ncam, L.ptr(cam_table), L.ptr(cam_of),
                       L.ptr(box_d), L.ptr(ctr_d), L.ptr(rad_d))
                L.call("captra_crop_ball_cam", B, H, W, CROP_CAP, L.ptr(depth), L.ptr(mask), L.ptr(box_d), L.ptr(ctr_d), L.ptr(rad_d), ncam,
                       L.ptr(cam_table), L.ptr(cam_of), L.ptr(pts), L.ptr(obj), L.ptr(pix), L.ptr(counts))
            elif det is not None:
                L.call("captra_crop_box_det", B, H, W, K, int(det["category"]), float(factor), L.ptr(trans_d), L.ptr(scale_d), kk.data_ptr(),
                       L.ptr(det_boxes), L.ptr(det_class), L.ptr(det_count), L.ptr(box_d), L.ptr(ctr_d), L.ptr(rad_d), L.ptr(raw_d), L.ptr(sel_d))
                L.call("captra_crop_ball_det", B, H, W, CROP_CAP, K, L.ptr(depth), L.ptr(mask), L.ptr(det_masks), L.ptr(sel_d), L.ptr(box_d),
                       L.ptr(ctr_d), L.ptr(rad_d), kk.data_ptr() + 72, L.ptr(pts), L.ptr(obj), L.ptr(pix), L.ptr(counts))
            else:
                L.call("captra_crop_box", B, H, W, float(factor), L.ptr(trans_d), L.ptr(scale_d), kk.data_ptr(), L.ptr(box_d), L.ptr(ctr_d), L.ptr(rad_d))
                L.call("captra_crop_ball", B, H, W, CROP_CAP, L.ptr(depth), L.ptr(mask), L.ptr(box_d), L.ptr(ctr_d), L.ptr(rad_d),
                       kk.data_ptr() + 72, L.ptr(pts), L.ptr(obj), L.ptr(pix), L.ptr(counts))
    else:
        centers = np.ascontiguousarray(np.asarray(centers, np.float64).reshape(B, 3))
        radii_in = np.asarray(radii_in, np.float64).reshape(B)
        radii = np.maximum(radii_in, 0.05)
        if cameras is not None:        # each row projected with its own K (the same float64 operations, one row at a time)
            boxes = np.stack([proj_corners_batch(H, W, centers[b:b + 1], radii_in[b:b + 1], cameras_on_host()[0][b]).reshape(4)
                              for b in range(B)]).astype(np.int32)
        else:
            boxes = proj_corners_batch(H, W, centers, radii_in, intrinsics).reshape(B, 4).astype(np.int32)
        kinv = _kinv(intrinsics)
        # ONE host-to-device copy for everything the crop kernel reads from the host: the doubles (centres, radii, K^-1), then
        # the int32 boxes (this stretch of host work sits between the pose round trip and the crop launch: the GPU waits for it)
        ndbl = 4 * B + 9
        blob = np.empty(8 * ndbl + 16 * B, np.uint8)
        blob[:8 * ndbl].view(np.float64)[:] = np.concatenate([centers.reshape(-1), radii, kinv])
        blob[8 * ndbl:].view(np.int32)[:] = boxes.reshape(-1)
        host = to_device(blob, dev)
        hp = host.data_ptr()
        with torch.cuda.device(dev):
            if cameras is not None:
                L.call("captra_crop_ball_cam", B, H, W, CROP_CAP, L.ptr(depth), L.ptr(mask), hp + 8 * ndbl, hp, hp + 8 * 3 * B, ncam,
                       L.ptr(cam_table), L.ptr(cam_of), L.ptr(pts), L.ptr(obj), L.ptr(pix), L.ptr(counts))
            else:
                L.call("captra_crop_ball", B, H, W, CROP_CAP, L.ptr(depth), L.ptr(mask), hp + 8 * ndbl, hp,
                       hp + 8 * 3 * B, hp + 8 * 4 * B, L.ptr(pts), L.ptr(obj), L.ptr(pix), L.ptr(counts))
    table_t = thinned_t = None
    if thin is not None:
        # the thinning launch (a workgroup per instance, which leaves at once when its list is not over-long): behind the crop in BOTH
        # stages, with the same (seed, frame, b0 + row), so that a frame run again on the synchronous stage thins as its first run did
        seed, frame, b0 = (int(x) for x in thin)
        buf = torch.empty(B * (5 * num_points + 1), dtype=torch.int32, device=dev)         # (one allocation: the table, then the flags)
        table_t, thinned_t = buf[:B * 5 * num_points].view(B, 5 * num_points), buf[B * 5 * num_points:]
        with torch.cuda.device(dev):
            L.call("captra_otf_thin", B, CROP_CAP, num_points, b0, frame & 0xFFFFFFFF, seed & 0xFFFFFFFFFFFFFFFF, L.ptr(counts), None,
                   L.ptr(table_t), L.ptr(thinned_t))
    if defer is not None and pose_dev is not None:
        # ---- NO round trip: the candidate lists' lengths, the member table and the ragged sampler's
        # per-cloud counts are derived from the crop's counts ON THE DEVICE; the sampler's padded stride is an upper bound the
        # caller knows without them (`defer` = that bound: the previous frame's longest list with a margin, at most 5 N).  What
        # the host would have decided from the counts -- an instance on a rare path (< 10 members: radius growth; a list longer
        # than the bound or than 5 N: thinning, which draws from numpy's generator on the host) -- comes back as a device word
        # [any rare instance, longest list] the caller reads one frame LATE and, when set, answers by running the frame again on
        # the synchronous path below.  Rare rows are clamped so that every launch stays inside its buffers; their output is unused.
        stride = int(min(max(int(defer), num_points), 5 * num_points))
        cand = torch.empty(B, stride, 3, dtype=torch.float32, device=dev)
        lens = torch.empty(B, dtype=torch.int32, device=dev)
        info = torch.empty(4, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            if thin is not None:
                L.call("captra_otf_candidates_thin", B, CROP_CAP, stride, num_points, L.ptr(pts), L.ptr(counts), L.ptr(cand), L.ptr(lens), L.ptr(info),
                       L.ptr(table_t), L.ptr(thinned_t))
            else:
                L.call("captra_otf_candidates", B, CROP_CAP, stride, num_points, L.ptr(pts), L.ptr(counts), L.ptr(cand), L.ptr(lens), L.ptr(info))
        res = fused.fps_gather(cand, num_points, n_per_cloud=lens)
        if gt_dev is not None:
            rot, trans, scale = (gt_dev["rotation"].reshape(B, 3, 3).contiguous(), gt_dev["translation"].reshape(B, 3).contiguous(),
                                 gt_dev["scale"].reshape(B).contiguous())
        else:
            rot = to_device(np.ascontiguousarray(np.asarray(gt["rotation"], np.float64).reshape(B, 3, 3)), dev)
            trans = to_device(np.ascontiguousarray(np.asarray(gt["translation"], np.float64).reshape(B, 3)), dev)
            scale = to_device(np.ascontiguousarray(np.asarray(gt["scale"], np.float64).reshape(B)), dev)
        mean_d = (torch.zeros(B, 3, dtype=torch.float32, device=dev) if mean is None else mean.reshape(B, 3).float().contiguous())
        points_cn = torch.empty(B, 3, num_points, dtype=torch.float32, device=dev)
        labels = torch.empty(B, num_points, dtype=torch.int64, device=dev)
        nocs_cn = torch.empty(B, 3, num_points, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            if thin is not None:
                L.call("captra_otf_finish_thin", B, CROP_CAP, stride, num_points, L.ptr(pts), L.ptr(obj), L.ptr(counts), L.ptr(res[0]), L.ptr(mean_d),
                       L.ptr(rot), L.ptr(trans), L.ptr(scale), L.ptr(points_cn), L.ptr(labels), L.ptr(nocs_cn), L.ptr(table_t), L.ptr(thinned_t))
                return {"points_cn": points_cn, "labels": labels, "nocs_cn": nocs_cn, "_info": info, "_thinned": thinned_t}
            L.call("captra_otf_finish", B, CROP_CAP, stride, num_points, L.ptr(pts), L.ptr(obj), L.ptr(counts), L.ptr(res[0]), L.ptr(mean_d),
                   L.ptr(rot), L.ptr(trans), L.ptr(scale), L.ptr(points_cn), L.ptr(labels), L.ptr(nocs_cn))
        return {"points_cn": points_cn, "labels": labels, "nocs_cn": nocs_cn, "_info": info}
    n_members = to_host(counts[:, 0].contiguous())                                               # the one sync of the stage
    sel_h = None
    if pose_dev is not None and any(int(c) < 10 or int(c) > CROP_CAP for c in n_members):
        # a rare-path instance (radius growth / more members than the table holds) takes the torch path, which wants the centre on the host
        # (the detector route: and the radius as the selection grew it, and the selection -- exact in a float64 -- in the same round trip)
        if det is not None:
            cs = to_host(torch.cat([ctr_d, raw_d.reshape(B, 1), sel_d.double().reshape(B, 1)], dim=1))
            sel_h = cs[:, 4].astype(np.int64)
        else:
            cs = to_host(torch.cat([ctr_d, (float(factor) * scale_d.double()).reshape(B, 1)], dim=1))
        centers, radii_in = np.ascontiguousarray(cs[:, :3]), np.ascontiguousarray(cs[:, 3])

    def gt_of(b):
        return {"rotation": gt["rotation"][b], "translation": np.asarray(gt["translation"][b]).reshape(3, 1), "scale": gt["scale"][b]}

    # host: the candidate list of every instance as indices into its member table (list doubling = index modulo count,
    # thinning = a prefix of numpy's permutation), in trajectory order because the permutations consume numpy's generator
    lengths, perms, slow = [0] * B, {}, {}
    for b in range(B):
        c = int(n_members[b])
        if c < 10 or c > CROP_CAP:
            mask_b = det_masks[b, int(sel_h[b])] if sel_h is not None and sel_h[b] >= 0 else mask[b]
            if cameras is not None:
                slow[b] = crop_candidates(depth[b], mask_b.bool(), centers[b], float(radii_in[b]), num_points, cameras_on_host()[0][b],
                                          depth_unit=float(cameras_on_host()[1][b]))
            else:
                slow[b] = crop_candidates(depth[b], mask_b.bool(), centers[b], float(radii_in[b]), num_points, intrinsics)
            continue
        length = c
        while length < num_points:
            length *= 2
        if length > 5 * num_points:
            # (thin: the row of table_t the launch above filled -- no draw from numpy)
            perms[b] = None if thin is not None else np.random.permutation(length)[:5 * num_points]
            length = 5 * num_points
        lengths[b] = length
    fast = [b for b in range(B) if lengths[b] > 0]
    out = [None] * B
    if fast:
        lens = [lengths[b] for b in fast]
        cnt_f = counts[fast, 0].long() if len(fast) < B else counts[:, 0].long()
        # candidate j of an instance = member (j mod count): computed on the device (no table upload); only a thinned
        # list needs its permutation prefix from the host
        table_d = torch.arange(max(lens), device=dev).unsqueeze(0) % cnt_f.unsqueeze(1)
        for i, b in enumerate(fast):
            if b in perms:
                table_d[i, :lens[i]] = table_t[b].long() if perms[b] is None else to_device(perms[b], dev) % cnt_f[i]
        if len(fast) == B:
            pts_f, obj_f = pts, obj
        else:
            fidx = to_device(np.asarray(fast, np.int64), dev)
            pts_f, obj_f = pts[fidx], obj[fidx]
        cand = torch.gather(pts_f, 1, table_d.unsqueeze(-1).expand(-1, -1, 3)).float()
        res = fused.fps_gather(cand, num_points, n_per_cloud=to_device(np.asarray(lens, np.int32), dev))
        sel = torch.gather(table_d, 1, res[0].long())                                             # (F, N) member numbers
        P = torch.gather(pts_f, 1, sel.unsqueeze(-1).expand(-1, -1, 3))                            # (F, N, 3) float64
        O = torch.gather(obj_f, 1, sel).bool()
        sub = slice(None) if len(fast) == B else np.asarray(fast)
        if gt_dev is not None:
            pick = (lambda t: t) if len(fast) == B else (lambda t: t[fidx])
            rot, trans, scale = pick(gt_dev["rotation"].reshape(B, 3, 3)), pick(gt_dev["translation"].reshape(B, 1, 3)), pick(gt_dev["scale"].reshape(B))
        else:
            rot = to_device(np.ascontiguousarray(np.asarray(gt["rotation"], np.float64).reshape(B, 3, 3)[sub]), dev)
            trans = to_device(np.ascontiguousarray(np.asarray(gt["translation"], np.float64).reshape(B, 1, 3)[sub]), dev)
            scale = to_device(np.ascontiguousarray(np.asarray(gt["scale"], np.float64).reshape(B)[sub]), dev)
        nocs = torch.where(O.unsqueeze(-1), torch.bmm((P - trans) / scale.reshape(-1, 1, 1), rot), torch.zeros_like(P))
        labels = 1 - O.long()
        if stacked and len(fast) == B:
            return {"points": P, "labels": labels, "nocs": nocs, **({} if thin is None else {"_thinned": thinned_t})}
        for i, b in enumerate(fast):
            out[b] = {"points": P[i], "labels": labels[i], "nocs": nocs[i]}
    for b, (p_all, raw_mask, idx, perm) in slow.items():
        picked = _device_fps(_candidate_cloud(p_all, idx, perm), num_points)
        sel_b = idx[perm[picked] if perm is not None else picked]
        out[b] = _full_data(p_all[sel_b], raw_mask[sel_b], gt_of(b))
    if stacked and thin is not None:
        return {**stack_full_data(out), "_thinned": thinned_t}
    return stack_full_data(out) if stacked else out
