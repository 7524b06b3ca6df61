"""Evaluation beside the tracking step: `EvalTrackModel.compute_loss(eval_iou=True)` with cfg['eval_device'] off (host numpy
protocol) and on (captra_amd/csrc/box_iou.hip), the IoU launches alone between device events, and the tracking step, all in one
process, for synthetic drawers and bottle trajectories.  One JSON line.

Every figure is the median of repeated blocks with a device synchronise on both sides, after a warm-up of the same shapes; the
min / max of the blocks are reported as the run-to-run spread.  The host path costs seconds per call at 32 drawers
trajectories, so it gets fewer repeats (`--host_reps`).

Usage: python tools/bench_eval.py [--batch 32] [--frames 4] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from bench import build_workload  # noqa: E402
from captra_amd.pose_utils import bbox_utils as BU  # noqa: E402


def _stats(ms):
    ms = sorted(ms)
    return {"median": round(ms[(len(ms) - 1) // 2], 4), "min": round(ms[0], 4), "max": round(ms[-1], 4), "blocks": len(ms)}


def _host_timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return out


def _flat_iou(d, prefix=""):
    out = {}
    for k, v in d.items():
        if isinstance(v, dict):
            out.update(_flat_iou(v, f"{prefix}{k}/"))
        else:
            out[f"{prefix}{k}"] = float(v)
    return out


def run(category, args, device):
    cfg, _, model, data = build_workload(args.batch, device, frames=args.frames, category=category)
    evaluated = args.frames - 1
    model.eval_device = False
    with torch.no_grad():
        model.forward()
    # the tracking step, as bench.py launches it (eager), blocks of `--steps` steps
    pose = {k: v.clone() for k, v in model.pred_dict["poses"][0].items()}

    def steps():
        p = pose
        with torch.no_grad():
            for i in range(args.steps):
                f = 1 + i % evaluated
                _, p = model.track_step(model.feed_dict[f], model.npcs_feed_dict[f], p)

    step_ms = [t / args.steps for t in _host_timed(steps, 2, args.reps)]
    loss = lambda: model.compute_loss(test=True, per_instance=False, eval_iou=True, test_prefix="test")
    off_ms = [t / evaluated for t in _host_timed(loss, 0, args.host_reps)]       # numpy on the host: nothing to warm
    iou_off = _flat_iou(model.loss_dict["avg_iou"])
    model.eval_device = True
    on_ms = [t / evaluated for t in _host_timed(loss, 3, args.reps)]
    iou_on = _flat_iou(model.loss_dict["avg_iou"])
    # the IoU launches alone: the call compute_loss makes, captured once and replayed between events
    captured, real = [], BU.box_iou_device
    BU.box_iou_device = lambda *a, **k: (captured.append((a, k)), real(*a, **k))[1]
    try:
        loss()
    finally:
        BU.box_iou_device = real
    kernel_ms = []
    for r in range(3 + args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for a, k in captured:
            real(*a, **k)
        e1.record()
        e1.synchronize()
        if r >= 3:
            kernel_ms.append(e0.elapsed_time(e1) / evaluated)
    pairs = sum(int(a[0].shape[0] * a[0].shape[1]) for a, _ in captured)
    res = {"batch": args.batch, "evaluated_frames": evaluated, "box_pairs_per_call": pairs, "iou_calls_per_compute_loss": len(captured),
           "track_step_ms": _stats(step_ms), "eval_off_ms_per_frame": _stats(off_ms), "eval_on_ms_per_frame": _stats(on_ms),
           "iou_launches_ms_per_frame": _stats(kernel_ms),
           "max_abs_iou_difference_on_vs_off": max(abs(iou_on[k] - iou_off[k]) for k in iou_off)}
    res["speedup_compute_loss"] = round(res["eval_off_ms_per_frame"]["median"] / res["eval_on_ms_per_frame"]["median"], 1)
    res["eval_on_below_track_step"] = res["eval_on_ms_per_frame"]["max"] < res["track_step_ms"]["min"]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=4, help="frames per trajectory (the first is the initialisation)")
    ap.add_argument("--steps", type=int, default=20, help="tracking steps per timed block")
    ap.add_argument("--reps", type=int, default=9, help="timed blocks (device path, tracking step, IoU launches)")
    ap.add_argument("--host_reps", type=int, default=2, help="timed blocks of the host path")
    ap.add_argument("--categories", default="drawers,bottle")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval needs a GPU")
    device = torch.device("cuda:0")
    out = {"tool": "bench_eval", "device": torch.cuda.get_device_name(0), "timing": "median of blocks, synchronise on both sides; ms",
           "compute_loss_per_frame": "one compute_loss(eval_iou=True) call over the trajectory / evaluated frames (pose errors, "
                                     "segmentation and NOCS losses included: only the IoU part differs between off and on)"}
    for category in args.categories.split(","):
        out[category] = run(category, args, device)
    line = json.dumps(out)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
