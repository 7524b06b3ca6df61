"""The motion model (csrc/pose_motion.hip, track_cfg/motion) measured twice, in one process:
  cost    ms per step with the option on and off, alternating: the pre-cropped hipGraph loop at 32 and at 1 trajectories and the
          on-the-fly re-crop loop at 32; off is the parent's path, on adds one launch per step and a longer hand-over;
  effect  the error of the pose that ENTERS frame i against frame i's ground truth (eval_part_full: degrees / metres) and the error
          of the pose the frame ends with, on and off, over the frames that can be predicted (i >= 2): make_trajectory('nocs', 32, 16)
          as it is, every third frame of a 48-frame trajectory (three times the velocity), make_otf_trajectory at step_px 6 and 18.
          The weights are make_physical_state_dict's, not a trained network's.
Prints one JSON line: median, p10 and p90 over the timed blocks, and the mean errors.

Usage: python tools/bench_motion.py [--blocks 7] [--block-seconds 1.0] [--frames 16] [--out profiles/motion_bench.json]
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

from captra_amd.configs import make_config  # noqa: E402
from captra_amd.pose_utils.part_dof_utils import eval_part_full  # noqa: E402
from captra_amd.synthetic import cat_trajectories, make_otf_trajectory, make_physical_state_dict, make_trajectory  # noqa: E402
from captra_amd.trainer import Trainer  # noqa: E402

OPTION = {"predict": True, "max_angle": 30, "max_shift": 0.2, "gain": 1.0}
MODES = ("off", "on")


def stats(v) -> dict:
    return {"median": round(float(np.median(v)), 4), "p10": round(float(np.percentile(v, 10)), 4), "p90": round(float(np.percentile(v, 90)), 4)}


def make_trainer(dev, on: bool, otf: bool):
    cfg = make_config("1", experiment_dir="/tmp/captra_motion_bench", nocs_otf=otf, hipgraph=True, **{"init_frame/gt": True})
    cfg["device"] = dev
    if on:
        cfg["track_cfg"]["motion"] = dict(OPTION)
    trainer = Trainer(cfg)
    shapes = {k: tuple(v.shape) for k, v in trainer.model.state_dict().items()}
    trainer.model.load_state_dict(make_physical_state_dict(shapes, 31, 1, True, "nocs"))
    trainer.model.eval()
    return trainer


def otf_scene(batch: int, frames: int, dev, step_px: float = 6.0):
    """`batch` trajectories: copies of two seeded ones; the images already on the device, so a pass pays no host-to-device copy."""
    singles = [make_otf_trajectory(1, frames, seed=s, step_px=step_px) for s in (1, 2)]
    data = singles[0] if batch == 1 else cat_trajectories([singles[b % 2] for b in range(batch)])
    for f in data:
        f["meta"]["pre_fetched"] = {k: v.to(dev) for k, v in f["meta"]["pre_fetched"].items() if k in ("depth", "mask")}
    return data


def one_loop(trainer, data) -> float:
    """One pass (set_data + the loop) over `data` -> seconds (host clock around a device synchronisation on both sides)."""
    np.random.seed(0)
    torch.manual_seed(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    trainer.model.set_data(data)
    trainer.model.test(save=False, no_eval=True)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def bench_cost(trainers, data, blocks: int, block_seconds: float) -> dict:
    steps = len(data) - 1
    passes = {}
    for mode in MODES:
        one_loop(trainers[mode], data)                                   # warm-up: graph capture and allocator
        t = min(one_loop(trainers[mode], data) for _ in range(2))
        passes[mode] = max(1, int(np.ceil(block_seconds / t)))
    ms = {mode: [] for mode in MODES}
    for _ in range(blocks):
        for mode in MODES:                                               # alternating: drift of the box hits both modes alike
            t = sum(one_loop(trainers[mode], data) for _ in range(passes[mode]))
            ms[mode].append(1e3 * t / (passes[mode] * steps))
    return {mode: {**stats(v), "passes_per_block": passes[mode]} for mode, v in ms.items()}


def effect(trainers, data) -> dict:
    """Mean rotation (degrees) and translation (metres) error over the frames i >= 2 and the trajectories: of the pose entering the
    frame and of the pose it ends with, per mode; and the share of (frame, trajectory) starts that were predictions."""
    out = {}
    for mode in MODES:
        model = trainers[mode].model
        one_loop(trainers[mode], data)
        pred, feed, sym = model.pred_dict, model.feed_dict, model.sym
        enter, final = {"rdiff": [], "tdiff": []}, {"rdiff": [], "tdiff": []}
        for i in range(2, len(feed)):
            start = pred["poses"][i - 1]
            if mode == "on":
                rec = pred["motion"][i - 1]
                start = {"rotation": rec["rotation"], "scale": start["scale"], "translation": rec["translation"]}
            for pose, acc in ((start, enter), (pred["poses"][i], final)):
                diff, _ = eval_part_full(feed[i]["gt_part"], pose, per_instance=False, yaxis_only=sym)
                for k in acc:
                    acc[k].append(float(diff[k + "_0"]))
        out[mode] = {"entering": {k: round(float(np.mean(v)), 5) for k, v in enter.items()},
                     "final": {k: round(float(np.mean(v)), 5) for k, v in final.items()}}
        if mode == "on":
            used = torch.stack([pred["motion"][i]["used"] for i in range(1, len(feed) - 1)]).float()
            out[mode]["predicted_share"] = round(float(used.mean()), 4)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--block-seconds", type=float, default=1.0)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_motion needs a GPU: there is no CPU fall-back and no CPU timing")
    dev = torch.device("cuda:0")
    pre = {mode: make_trainer(dev, mode == "on", otf=False) for mode in MODES}
    otf = {mode: make_trainer(dev, mode == "on", otf=True) for mode in MODES}
    cost = {"unit": "ms per step of B trajectories (set_data included)", "frames": args.frames}
    for name, trainers, data in (("precropped B=32", pre, make_trajectory("nocs", 32, args.frames, seed=7)),
                                 ("precropped B=1", pre, make_trajectory("nocs", 1, args.frames, seed=7)),
                                 ("nocs_otf B=32", otf, otf_scene(32, args.frames, dev))):
        cost[name] = bench_cost(trainers, data, args.blocks, args.block_seconds)
        print(f"# cost {name}: " + "  ".join(f"{m} {cost[name][m]['median']:.3f}" for m in MODES) + " ms per step (median)", file=sys.stderr, flush=True)
    eff = {"unit": "mean over frames >= 2 and trajectories: rdiff degrees, tdiff metres", "frames": args.frames}
    for name, trainers, data in (("make_trajectory(nocs, 32, 16)", pre, make_trajectory("nocs", 32, args.frames, seed=7)),
                                 ("every third frame of 48", pre, make_trajectory("nocs", 32, 3 * args.frames, seed=7)[::3]),
                                 ("make_otf_trajectory step_px 6", otf, otf_scene(32, args.frames, dev, step_px=6.0)),
                                 ("make_otf_trajectory step_px 18", otf, otf_scene(32, args.frames, dev, step_px=18.0))):
        eff[name] = effect(trainers, data)
        print(f"# effect {name}: " + json.dumps(eff[name]), file=sys.stderr, flush=True)
    line = json.dumps({"bench": "motion", "option": OPTION, "blocks": args.blocks, "block_seconds": args.block_seconds, "cost": cost, "effect": eff})
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
