"""Per-part pose fits from NOCS <-> camera correspondences, one HIP launch each.

Mirrors `part_fit_st_no_ransac` / `filter_model_valid` of the reference's pose_utils/pose_fit.py
(l.26-53).  The reference builds a one-hot mask and runs transform_pts_mask (~30 ATen kernels and
a host SVD for symmetric objects); here the labels go straight to captra_part_fit_st.

`part_fit_ransac` is the estimator that needs no previous pose: the RANSAC similarity fit `pose_fit` of the reference's
datasets/nocs_data/preproc_nocs/align_pose.py:49-93 (host numpy there), captra_part_fit_ransac here.
"""
from __future__ import annotations

import torch

from .. import _lib as L


def filter_model_valid(model: dict, valid: torch.Tensor) -> torch.Tensor:
    for key in ("scale", "translation", "rotation"):
        tmp = model[key] if key == "scale" else model[key].sum((-1, -2))
        valid = torch.logical_and(valid, torch.isfinite(tmp))
    return valid


def part_fit_st_cn(labels_i32, src_cn, tgt_cn, rotation, sym: bool, given_scale=None, tgt_per_part=False):
    """Channel-major fast path used by the track loop (no transposes):
    labels (B,N) int32, src_cn (B,P,3,N), tgt_cn (B,3,N) [or (B,P,3,N)], rotation (B,P,3,3)
    -> scale (B,P), translation (B,P,3,1), valid (B,P) bool."""
    L.require_device(labels_i32, src_cn, tgt_cn, rotation, given_scale)
    B, P, _, N = src_cn.shape
    dev = src_cn.device
    scale = torch.empty(B, P, dtype=torch.float32, device=dev)
    trans = torch.empty(B, P, 3, dtype=torch.float32, device=dev)
    valid = torch.empty(B, P, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.call("captra_part_fit_st", B, P, N, 1 if sym else 0, L.ptr(labels_i32), L.ptr(src_cn), L.ptr(tgt_cn),
               1 if tgt_per_part else 0, L.ptr(rotation), L.ptr(given_scale), L.ptr(scale), L.ptr(trans), L.ptr(valid))
    return scale, trans.unsqueeze(-1), valid.bool()


def part_fit_st_track(labels_i32, src_cn, pts_cn, pts_mean, rotation, prev_scale, prev_trans, sym: bool):
    """The track loop's fit in one launch (networks.py:219-232): target = pts (B,3,N) + pts_mean (B,3,1) formed inside the
    kernel, invalid fits keep prev_scale (B,P) / prev_trans (B,P,3,1) -> scale (B,P), translation (B,P,3,1), valid (B,P) bool."""
    B, P, _, N = src_cn.shape
    dev = src_cn.device
    pts_mean = pts_mean.reshape(B, 3).float().contiguous()
    prev_scale = prev_scale.float().contiguous()
    prev_trans = prev_trans.reshape(B, P, 3).float().contiguous()
    L.require_device(labels_i32, src_cn, pts_cn, pts_mean, rotation, prev_scale, prev_trans)
    scale = torch.empty(B, P, dtype=torch.float32, device=dev)
    trans = torch.empty(B, P, 3, dtype=torch.float32, device=dev)
    valid = torch.empty(B, P, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.call("captra_part_fit_st_track", B, P, N, 1 if sym else 0, L.ptr(labels_i32), L.ptr(src_cn), L.ptr(pts_cn), L.ptr(pts_mean),
               L.ptr(rotation), L.ptr(prev_scale), L.ptr(prev_trans), L.ptr(scale), L.ptr(trans), L.ptr(valid))
    return scale, trans.unsqueeze(-1), valid.bool()


def part_fit_st_no_ransac(labels, source, target, rotation, cfg, given_scale=None):
    """labels (B,N); source, target (B,P,N,3); rotation (B,P,3,3); cfg {'num_parts','sym'}
    -> ({'rotation','scale' (B,P),'translation' (B,P,3,1)}, valid (B,P) bool)."""
    src_cn = source.transpose(-1, -2).float().contiguous()
    tgt_cn = target.transpose(-1, -2).float().contiguous()
    rot = rotation.float().contiguous()
    gs = None if given_scale is None else given_scale.float().contiguous()
    scale, translation, valid = part_fit_st_cn(labels.int().contiguous(), src_cn, tgt_cn, rot, bool(cfg["sym"]),
                                               given_scale=gs, tgt_per_part=True)
    model = {"rotation": rotation, "scale": scale, "translation": translation}
    return model, filter_model_valid(model, valid)


def part_fit_ransac_cn(labels_i32, src_cn, tgt_cn, num_hyps=64, inlier_th=1e-3, sample_rank=None, seed=0, target_mean=None,
                       tgt_per_part=False, want_samples=False, yaxis_only=False):
    """Channel-major form (no transposes): labels (B,N) int32, src_cn (B,P,3,N), tgt_cn (B,3,N) [or (B,P,3,N) with
    tgt_per_part], target_mean (B,3[,1]) or None (the target is tgt + mean, one fp32 addition in the kernel), sample_rank
    (B,P,H,3) int32 member ranks or None (drawn in the kernel from `seed`, include/captra_hip.h)
    -> rotation (B,P,3,3), scale (B,P), translation (B,P,3,1), valid (B,P) bool, info {'best', 'num_inliers' (B,P) int32
    [, 'samples' (B,P,H,3) int32 point indices]}.  An invalid fit is identity / 1 / 0.
    yaxis_only: the axis-only inlier test of the symmetric categories (captra_part_fit_ransac_sym)."""
    B, P, _, N = src_cn.shape
    dev = src_cn.device
    if target_mean is not None:
        target_mean = target_mean.reshape(B, 3).float().contiguous()
    if sample_rank is not None:
        sample_rank = sample_rank.reshape(B, P, num_hyps, 3).int().contiguous()
    L.require_device(labels_i32, src_cn, tgt_cn, target_mean, sample_rank)
    rot = torch.empty(B, P, 3, 3, dtype=torch.float32, device=dev)
    scale = torch.empty(B, P, dtype=torch.float32, device=dev)
    trans = torch.empty(B, P, 3, dtype=torch.float32, device=dev)
    valid = torch.empty(B, P, dtype=torch.int32, device=dev)
    best = torch.empty(B, P, dtype=torch.int32, device=dev)
    ninl = torch.empty(B, P, dtype=torch.int32, device=dev)
    samples = torch.empty(B, P, num_hyps, 3, dtype=torch.int32, device=dev) if want_samples else None
    with torch.cuda.device(dev):
        L.call("captra_part_fit_ransac_sym" if yaxis_only else "captra_part_fit_ransac", B, P, N, int(num_hyps), float(inlier_th), L.ptr(labels_i32), L.ptr(src_cn), L.ptr(tgt_cn),
               1 if tgt_per_part else 0, L.ptr(target_mean), L.ptr(sample_rank), int(seed) & 0xFFFFFFFFFFFFFFFF, L.ptr(rot), L.ptr(scale),
               L.ptr(trans), L.ptr(valid), L.ptr(best), L.ptr(ninl), L.ptr(samples))
    info = {"best": best, "num_inliers": ninl}
    if want_samples:
        info["samples"] = samples
    return rot, scale, trans.unsqueeze(-1), valid.bool(), info


def part_fit_ransac(labels, source, target, cfg, num_hyps=64, inlier_th=1e-3, sample_rank=None, seed=0, target_mean=None,
                    yaxis_only=False):
    """The reference layouts of part_fit_st_no_ransac: labels (B,N); source (B,P,N,3); target (B,P,N,3) or (B,N,3);
    cfg {'num_parts'} -> ({'rotation' (B,P,3,3), 'scale' (B,P), 'translation' (B,P,3,1)}, valid (B,P) bool,
    info {'best', 'num_inliers'})."""
    assert source.shape[1] == int(cfg["num_parts"]), (source.shape, cfg["num_parts"])
    src_cn = source.transpose(-1, -2).float().contiguous()
    tgt_cn = target.transpose(-1, -2).float().contiguous()
    rot, scale, trans, valid, info = part_fit_ransac_cn(labels.int().contiguous(), src_cn, tgt_cn, num_hyps=num_hyps, inlier_th=inlier_th,
                                                        sample_rank=sample_rank, seed=seed, target_mean=target_mean,
                                                        tgt_per_part=target.dim() == 4, yaxis_only=yaxis_only)
    return {"rotation": rot, "scale": scale, "translation": trans}, valid, info


def _part_fit_st_ransac_call(labels_i32, src_cn, tgt_cn, tgt_per_part, tgt_mean, rotation, prev_scale, prev_trans, sym, inlier_th,
                             num_hyps, seed, b0, sample_rank):
    """captra_part_fit_st_ransac on prepared tensors -> scale (B,P), trans (B,P,3), valid (B,P) int32, inliers, best (B,P) int32."""
    B, P, _, N = src_cn.shape
    dev = src_cn.device
    if sample_rank is not None:
        sample_rank = sample_rank.reshape(B, P, int(num_hyps), 3).int().contiguous()
    L.require_device(labels_i32, src_cn, tgt_cn, tgt_mean, rotation, prev_scale, prev_trans, sample_rank)
    scale = torch.empty(B, P, dtype=torch.float32, device=dev)
    trans = torch.empty(B, P, 3, dtype=torch.float32, device=dev)
    valid = torch.empty(B, P, dtype=torch.int32, device=dev)
    best = torch.empty(B, P, dtype=torch.int32, device=dev)
    ninl = torch.empty(B, P, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.call("captra_part_fit_st_ransac", B, P, N, 1 if sym else 0, int(b0), int(num_hyps), float(inlier_th), L.ptr(labels_i32),
               L.ptr(src_cn), L.ptr(tgt_cn), 1 if tgt_per_part else 0, L.ptr(tgt_mean), L.ptr(rotation), L.ptr(prev_scale),
               L.ptr(prev_trans), L.ptr(sample_rank), int(seed) & 0xFFFFFFFFFFFFFFFF, L.ptr(scale), L.ptr(trans), L.ptr(valid),
               L.ptr(best), L.ptr(ninl))
    return scale, trans, valid, ninl, best


def part_fit_st_ransac_track(labels_i32, src_cn, pts_cn, pts_mean, rotation, prev_scale, prev_trans, sym: bool, inlier_th,
                             num_hyps=64, seed=0, b0=0, sample_rank=None):
    """The track loop's ROBUST fit in one launch (captra_part_fit_st_ransac, include/captra_hip.h): part_fit_st_track's arguments --
    target = pts (B,3,N) + pts_mean (B,3,1) formed inside the kernel, invalid fits keep prev_scale (B,P) / prev_trans (B,P,3,1) --
    plus the inlier distance, the number of three-member hypotheses, the seed of the kernel's draws with b0 = the index of the first
    trajectory within the whole batch (or sample_rank (B,P,H,3) int32 member ranks)
    -> scale (B,P), translation (B,P,3,1), valid (B,P) bool, info {'inliers', 'best' (B,P) int32}."""
    B, P, _, N = src_cn.shape
    pts_mean = pts_mean.reshape(B, 3).float().contiguous()
    prev_scale = prev_scale.float().contiguous()
    prev_trans = prev_trans.reshape(B, P, 3).float().contiguous()
    scale, trans, valid, ninl, best = _part_fit_st_ransac_call(labels_i32, src_cn, pts_cn, False, pts_mean, rotation, prev_scale, prev_trans,
                                                               sym, inlier_th, num_hyps, seed, b0, sample_rank)
    return scale, trans.unsqueeze(-1), valid.bool(), {"inliers": ninl, "best": best}


def part_fit_st_ransac(labels, source, target, rotation, cfg, inlier_th=1e-3, num_hyps=64, seed=0, sample_rank=None, target_mean=None):
    """The counterpart the reference's part_fit_st_no_ransac is named after, with its argument order and return value: labels (B,N);
    source, target (B,P,N,3); rotation (B,P,3,3); cfg {'num_parts','sym'}
    -> ({'rotation','scale' (B,P),'translation' (B,P,3,1)}, valid (B,P) bool).  An invalid fit holds 1 / 0."""
    assert source.shape[1] == int(cfg["num_parts"]), (source.shape, cfg["num_parts"])
    B = source.shape[0]
    src_cn = source.transpose(-1, -2).float().contiguous()
    tgt_cn = target.transpose(-1, -2).float().contiguous()
    mean = None if target_mean is None else target_mean.reshape(B, 3).float().contiguous()
    scale, trans, valid, _, _ = _part_fit_st_ransac_call(labels.int().contiguous(), src_cn, tgt_cn, target.dim() == 4, mean,
                                                         rotation.float().contiguous(), None, None, bool(cfg["sym"]), inlier_th, num_hyps,
                                                         seed, 0, sample_rank)
    model = {"rotation": rotation, "scale": scale, "translation": trans.unsqueeze(-1)}
    return model, filter_model_valid(model, valid.bool())


SIZE_STATE_KEYS = ("size_mean", "size_n", "size_miss")      # the size state as it travels in the pose dict


def part_fit_st_size_track(labels_i32, src_cn, pts_cn, pts_mean, rotation, prev_scale, prev_trans, sym: bool, state, min_frames, max_ratio,
                           max_frames=None, reset_after=None, free=None, inlier_th=0.0, num_hyps=64, seed=0, b0=0, sample_rank=None):
    """Holding the track's size in one launch (captra_part_fit_st_size, include/captra_hip.h): part_fit_st_track's arguments, the size
    state {'size_mean' (B,P) float32, 'size_n', 'size_miss' (B,P) int32} and its options.  free = (scale (B,P), translation (B,P,3[,1]),
    valid (B,P)) of part_fit_st_track on the same arguments: PLAIN mode (inlier_th, num_hyps, seed, b0, sample_rank are not used);
    free = None: ROBUST mode, the kernel computes part_fit_st_ransac_track's fit itself (in place of that launch) from its arguments.
    -> ({'scale' (B,P), 'translation' (B,P,3,1), 'valid' (B,P) bool}, the new state, info {'held', 'accepted', 'n' (B,P) int32,
        'free' (B,P) float32: the record; 'free_translation' (B,P,3,1), 'free_valid' (B,P) int32, 'held_inliers', 'held_best' (B,P) int32
        [, 'inliers', 'best' (B,P) int32: the free robust fit's]})."""
    B, P, _, N = src_cn.shape
    dev = src_cn.device
    pts_mean = pts_mean.reshape(B, 3).float().contiguous()
    prev_scale = prev_scale.float().contiguous()
    prev_trans = prev_trans.reshape(B, P, 3).float().contiguous()
    mean_in, n_in, miss_in = (state[k].contiguous() for k in SIZE_STATE_KEYS)
    assert mean_in.dtype == torch.float32 and n_in.dtype == torch.int32 and miss_in.dtype == torch.int32 and mean_in.shape == (B, P)
    robust = free is None
    if robust:
        if sample_rank is not None:
            sample_rank = sample_rank.reshape(B, P, int(num_hyps), 3).int().contiguous()
        free_in = (None, None, None)
    else:
        num_hyps, sample_rank = 0, None
        free_in = (free[0].float().contiguous(), free[1].reshape(B, P, 3).float().contiguous(), free[2].int().contiguous())
    L.require_device(labels_i32, src_cn, pts_cn, pts_mean, rotation, prev_scale, prev_trans, sample_rank, mean_in, n_in, miss_in, *free_in)
    f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
    i32 = lambda: torch.empty(B, P, dtype=torch.int32, device=dev)
    scale, trans, valid = f32(B, P), f32(B, P, 3), i32()
    free_out = (f32(B, P), f32(B, P, 3), i32(), i32(), i32()) if robust else (None,) * 5
    mean_out, n_out, miss_out, held, accepted, held_best, held_inl = f32(B, P), i32(), i32(), i32(), i32(), i32(), i32()
    with torch.cuda.device(dev):
        L.call("captra_part_fit_st_size", B, P, N, 1 if sym else 0, int(b0), int(num_hyps), float(inlier_th), L.ptr(labels_i32), L.ptr(src_cn),
               L.ptr(pts_cn), 0, L.ptr(pts_mean), L.ptr(rotation), L.ptr(prev_scale), L.ptr(prev_trans), L.ptr(sample_rank),
               int(seed) & 0xFFFFFFFFFFFFFFFF, L.ptr(free_in[0]), L.ptr(free_in[1]), L.ptr(free_in[2]), L.ptr(mean_in), L.ptr(n_in),
               L.ptr(miss_in), int(min_frames), float(max_ratio), int(max_frames or 0), int(reset_after or 0), L.ptr(scale), L.ptr(trans),
               L.ptr(valid), *(L.ptr(t) for t in free_out), L.ptr(mean_out), L.ptr(n_out), L.ptr(miss_out), L.ptr(held), L.ptr(accepted),
               L.ptr(held_best), L.ptr(held_inl))
    fs, ft, fv = free_out[:3] if robust else free_in
    info = {"held": held, "accepted": accepted, "free": fs, "n": n_out, "free_translation": ft.unsqueeze(-1), "free_valid": fv,
            "held_inliers": held_inl, "held_best": held_best}
    if robust:
        info["inliers"], info["best"] = free_out[4], free_out[3]
    return ({"scale": scale, "translation": trans.unsqueeze(-1), "valid": valid.bool()},
            {"size_mean": mean_out, "size_n": n_out, "size_miss": miss_out}, info)


GUARD_VERDICTS = ("ok", "too_few", "lost", "recovered")      # the codes 0..3 of captra_part_fit_guard


def lost_ratio(lost_below) -> tuple[int, int]:
    """The fraction `lost_below` as the two ints (L, D) the guard compares with (inliers * D < L * count): the fraction the number
    was WRITTEN as (0.3 -> 3/10, not the binary float next to it), denominators up to 2^20; a pair (L, D) passes through."""
    from fractions import Fraction
    if isinstance(lost_below, (tuple, list)):
        num, den = int(lost_below[0]), int(lost_below[1])
    else:
        f = Fraction(repr(float(lost_below))).limit_denominator(1 << 20)
        num, den = f.numerator, f.denominator
    if num < 0 or den < 1 or num > den:
        raise ValueError(f"lost_below must be a fraction in [0, 1], got {lost_below!r}")
    return num, den


def part_fit_guard_cn(labels_i32, src_cn, pts_cn, pts_mean, pose, inlier_th, lost_below, min_members=4, refit=False, num_hyps=64,
                      seed=0, b0=0, yaxis_only=False):
    """Track health in one launch (captra_part_fit_guard, include/captra_hip.h): labels (B,N) int32, src_cn (B,P,3,N) predicted
    NOCS, pts_cn (B,3,N), pts_mean (B,3[,1]) or None, pose {'rotation' (B,P,3,3), 'scale' (B,P), 'translation' (B,P,3,1)} = the
    step's pose; lost_below a fraction (see lost_ratio); b0 = the index of the first trajectory within the whole batch.
    -> (pose dict, info {'count', 'inliers' (B,P) int32, 'rms' (B,P) float32, 'verdict' (B,P) int32: GUARD_VERDICTS}).
    refit=False: the pose dict IS `pose` (nothing is written); refit=True: new tensors, the re-fit where verdict == 3 and the input
    bits everywhere else.  yaxis_only: the axis-only inlier test of the symmetric categories in the check and in the re-fit
    (captra_part_fit_guard_sym)."""
    B, P, _, N = src_cn.shape
    dev = src_cn.device
    num, den = lost_ratio(lost_below)
    if pts_mean is not None:
        pts_mean = pts_mean.reshape(B, 3).float().contiguous()
    rot = pose["rotation"].float().contiguous()
    scale = pose["scale"].float().contiguous()
    trans = pose["translation"].reshape(B, P, 3).float().contiguous()
    L.require_device(labels_i32, src_cn, pts_cn, pts_mean, rot, scale, trans)
    count = torch.empty(B, P, dtype=torch.int32, device=dev)
    inliers = torch.empty(B, P, dtype=torch.int32, device=dev)
    rms = torch.empty(B, P, dtype=torch.float32, device=dev)
    verdict = torch.empty(B, P, dtype=torch.int32, device=dev)
    out = (torch.empty_like(rot), torch.empty_like(scale), torch.empty_like(trans)) if refit else (None, None, None)
    with torch.cuda.device(dev):
        L.call("captra_part_fit_guard_sym" if yaxis_only else "captra_part_fit_guard", B, P, N, int(b0), L.ptr(labels_i32), L.ptr(src_cn), L.ptr(pts_cn), L.ptr(pts_mean), L.ptr(rot),
               L.ptr(scale), L.ptr(trans), float(inlier_th), num, den, int(min_members), 1 if refit else 0, int(num_hyps),
               int(seed) & 0xFFFFFFFFFFFFFFFF, L.ptr(count), L.ptr(inliers), L.ptr(rms), L.ptr(verdict), L.ptr(out[0]), L.ptr(out[1]),
               L.ptr(out[2]))
    info = {"count": count, "inliers": inliers, "rms": rms, "verdict": verdict}
    if not refit:
        return pose, info
    return {"rotation": out[0], "scale": out[1], "translation": out[2].unsqueeze(-1)}, info


def pose_extrapolate(rot0, trans0, rot1, trans1, measured0, sym: bool, max_angle, max_shift, gain=1.0, verdict=None):
    """The motion model in one launch (captra_pose_extrapolate, include/captra_hip.h): rot0 (B,P,3,3), trans0 (B,P,3[,1]) = the result
    of the frame before, rot1 / trans1 = this frame's result, measured0 (B,P) int32 (nonzero: rot0 / trans0 are a measured result),
    verdict (B,P) int32 = the guard's codes of this frame (GUARD_VERDICTS) or None (all ok); max_angle in degrees inside (0, 90],
    max_shift in the translation's units, gain inside (0, 1]; sym: only the y-axis of a symmetric category moves.
    -> (rot_next (B,P,3,3), trans_next (B,P,3,1) = the pose the next frame starts from, measured1 (B,P) int32,
        info {'used' (B,P) int32, 'angle' (B,P) float32 degrees, 'shift' (B,P) float32})."""
    B, P = rot0.shape[:2]
    dev = rot0.device
    rot0, rot1 = rot0.float().contiguous(), rot1.float().contiguous()
    trans0, trans1 = trans0.reshape(B, P, 3).float().contiguous(), trans1.reshape(B, P, 3).float().contiguous()
    measured0 = measured0.int().contiguous()
    if verdict is not None:
        verdict = verdict.int().contiguous()
    L.require_device(rot0, trans0, rot1, trans1, measured0, verdict)
    rot_next, trans_next = torch.empty_like(rot1), torch.empty_like(trans1)
    measured1 = torch.empty(B, P, dtype=torch.int32, device=dev)
    used = torch.empty(B, P, dtype=torch.int32, device=dev)
    angle = torch.empty(B, P, dtype=torch.float32, device=dev)
    shift = torch.empty(B, P, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        L.call("captra_pose_extrapolate", B, P, 1 if sym else 0, L.ptr(rot0), L.ptr(trans0), L.ptr(rot1), L.ptr(trans1), L.ptr(measured0),
               L.ptr(verdict), float(gain), float(max_angle), float(max_shift), L.ptr(rot_next), L.ptr(trans_next), L.ptr(measured1),
               L.ptr(used), L.ptr(angle), L.ptr(shift))
    return rot_next, trans_next.unsqueeze(-1), measured1, {"used": used, "angle": angle, "shift": shift}


BOX_BINS = (64, 128, 256, 512)      # the histogram widths captra_part_box_hist takes


def part_box_hist(labels_i32, src_cn, state, *, bins, radial, quantile_permille, min_points, verdict=None):
    """Holding the track's box in one launch (captra_part_box_hist, include/captra_hip.h): labels (B,N) int32 = the labels the fit used,
    src_cn (B,P,3,N) predicted NOCS, state = the histograms (B,P,3,bins) int32 that entered the frame or None (a track's start: empty),
    verdict (B,P) int32 = the guard's codes of this frame (GUARD_VERDICTS) or None (every frame counts); radial: a symmetric category's
    x and z extents from the radius sqrt(x^2 + z^2).
    -> (new state (B,P,3,bins) int32 -- a new tensor, `state` is not written --,
        info {'extent' (B,P,3) float32: the held half-extents after this frame, 0 where fewer than min_points values are held,
              'frame' (B,P,3) float32: this frame's own, 'added' (B,P) int32: the frame's members, 'total' (B,P) int32: values held})."""
    B, P, _, N = src_cn.shape
    dev = src_cn.device
    bins = int(bins)
    if state is not None:
        state = state.contiguous()
        assert state.dtype == torch.int32 and tuple(state.shape) == (B, P, 3, bins), (state.dtype, tuple(state.shape))
    if verdict is not None:
        verdict = verdict.int().contiguous()
    L.require_device(labels_i32, src_cn, state, verdict)
    new_state = torch.empty(B, P, 3, bins, dtype=torch.int32, device=dev)
    extent = torch.empty(B, P, 3, dtype=torch.float32, device=dev)
    frame = torch.empty(B, P, 3, dtype=torch.float32, device=dev)
    added = torch.empty(B, P, dtype=torch.int32, device=dev)
    total = torch.empty(B, P, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.call("captra_part_box_hist", B, P, N, bins, 1 if radial else 0, int(quantile_permille), int(min_points), L.ptr(labels_i32),
               L.ptr(src_cn), L.ptr(verdict), L.ptr(state), L.ptr(new_state), L.ptr(extent), L.ptr(frame), L.ptr(added), L.ptr(total))
    return new_state, {"extent": extent, "frame": frame, "added": added, "total": total}
