"""Float64 numpy restatement of the detector route's selection (captra_crop_box_det, include/captra_hip.h; reference
datasets/nocs_data/nocs_data_process.py:166-179, 206-229): which 2D detection's mask the re-crop takes, and how far the crop's
radius grows before one overlaps.  Written as the reference evaluates it -- integer areas with exclusive extents, one float64
division, times `same`, numpy's first arg max -- on top of nocs_otf.proj_corners, which golden G11 pins against the reference's
get_proj_corners.  Golden G16 (tests/golden/g16_otf_det.npz) pins this judge against the reference itself.

The two rules outside the reference's contract are the header's: a union of 0 counts as IoU 0, and a growth step that does not
enlarge the radius ends the loop."""
from __future__ import annotations

import numpy as np

from captra_amd import nocs_otf


def box_ious(box, boxes) -> np.ndarray:
    """IoU of `box` [y1,x1,y2,x2] with every row of `boxes` (n,4): int64 areas max(x2 - x1, 0) * max(y2 - y1, 0), one division."""
    box = np.asarray(box, np.int64).reshape(4)
    boxes = np.asarray(boxes, np.int64).reshape(-1, 4)

    def area(x1, x2, y1, y2):
        return np.maximum(x2 - x1, 0) * np.maximum(y2 - y1, 0)

    inter = area(np.maximum(box[1], boxes[:, 1]), np.minimum(box[3], boxes[:, 3]), np.maximum(box[0], boxes[:, 0]), np.minimum(box[2], boxes[:, 2]))
    union = area(box[1], box[3], box[0], box[2]) + area(boxes[:, 1], boxes[:, 3], boxes[:, 0], boxes[:, 2]) - inter
    out = np.zeros(len(boxes), np.float64)
    ok = union != 0
    out[ok] = inter[ok].astype(np.float64) / union[ok].astype(np.float64)
    return out


def select(height, width, center, radius, det_boxes, det_class, det_count, category, intrinsics=nocs_otf.NOCS_REAL_INTRINSICS):
    """One trajectory: -> (sel, radius as the reference hands it on (grown, unclamped), corners (2,2) of the last round, rounds grown).
    Only the first det_count detections take part."""
    n = int(det_count)
    boxes = np.asarray(det_boxes).reshape(-1, 4)[:n]
    same = np.asarray(det_class).reshape(-1)[:n] == int(category)
    radius = np.float64(radius)
    corners = nocs_otf.proj_corners(height, width, center, radius, intrinsics)
    if same.sum() == 0:
        return -1, radius, corners, 0
    rounds = 0
    while True:
        corners = nocs_otf.proj_corners(height, width, center, radius, intrinsics)
        ious = box_ious(corners.reshape(-1), boxes) * same
        if np.max(ious) > 0.05 or radius > 0.5:
            break
        grown = radius * np.float64(1.2)
        if not grown > radius:
            break
        radius = grown
        rounds += 1
    return int(np.argmax(ious)), radius, corners, rounds


def select_batch(height, width, trans_f32, scale_f32, radius_factor, det_boxes, det_class, det_count, category,
                 intrinsics=nocs_otf.NOCS_REAL_INTRINSICS):
    """captra_crop_box_det's outputs for a batch, from the fp32 pose as the kernel reads it: -> dict of box (B,4) int32, center (B,3),
    radius (B,) = max(grown, 0.05), radius_raw (B,), sel (B,) int32, rounds (B,)."""
    trans = np.asarray(trans_f32, np.float32).reshape(-1, 3).astype(np.float64)
    scale = np.asarray(scale_f32, np.float32).reshape(-1).astype(np.float64)
    B = len(scale)
    out = {"box": np.zeros((B, 4), np.int32), "center": trans, "radius": np.zeros(B), "radius_raw": np.zeros(B),
           "sel": np.zeros(B, np.int32), "rounds": np.zeros(B, np.int64)}
    for b in range(B):
        sel, raw, corners, rounds = select(height, width, trans[b], np.float64(radius_factor) * scale[b], det_boxes[b], det_class[b],
                                           det_count[b], category, intrinsics)
        out["box"][b] = corners.reshape(-1)
        out["radius_raw"][b] = raw
        out["radius"][b] = raw if raw > 0.05 else 0.05
        out["sel"][b] = sel
        out["rounds"][b] = rounds
    return out
