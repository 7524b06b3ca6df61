"""Holding the track's size (csrc/pose_size.hip, track_cfg/size) measured twice, in one process:
  cost    ms per step with the option on and off, alternating: the pre-cropped hipGraph loop at 32 and at 1 trajectories and the
          on-the-fly re-crop loop at 32 -- in plain mode (one launch behind the one-pass fit) against the parent's path, and in robust
          mode (in place of the robust fit's launch) against track_cfg/st_fit alone;
  effect  over the frames of each trajectory, on and off: the spread (max / min) of the frame's own (free) scale and of the pose's
          scale -- times data_radius the re-crop's radius --, and the standard deviation of the translation error against ground
          truth (metres), averaged over the trajectories: make_trajectory('nocs', 32, 16) and make_otf_trajectory at step_px 6 and 18.
          The weights are make_physical_state_dict's, not a trained network's.
Prints one JSON line: median, p10 and p90 over the timed blocks, and the effect's means.

Usage: python tools/bench_size.py [--blocks 7] [--block-seconds 1.0] [--frames 16] [--out profiles/size_bench.json]
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
from captra_amd.synthetic import cat_trajectories, make_otf_trajectory, make_physical_state_dict, make_trajectory  # noqa: E402
from captra_amd.trainer import Trainer  # noqa: E402

# a test setting, not a recommendation: max_ratio depends on the trained network's scale scatter
OPTION = {"hold": True, "max_ratio": 1.2, "min_frames": 3, "max_frames": None, "reset_after": 5, "init_frames": 0}
ROBUST = {"ransac": True}
MODES = {"plain": ("off", "on"), "robust": ("off_robust", "on_robust")}


def stats(v) -> dict:
    return {"median": round(float(np.median(v)), 4), "p10": round(float(np.percentile(v, 10)), 4), "p90": round(float(np.percentile(v, 90)), 4)}


def make_trainer(dev, mode: str, otf: bool):
    cfg = make_config("1", experiment_dir="/tmp/captra_size_bench", nocs_otf=otf, hipgraph=True, **{"init_frame/gt": True})
    cfg["device"] = dev
    if mode.startswith("on"):
        cfg["track_cfg"]["size"] = dict(OPTION)
    if mode.endswith("robust"):
        cfg["track_cfg"]["st_fit"] = dict(ROBUST)
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


def bench_cost(trainers, modes, data, blocks: int, block_seconds: float) -> dict:
    steps = len(data) - 1
    passes = {}
    for mode in modes:
        one_loop(trainers[mode], data)                                   # warm-up: graph capture and allocator
        t = min(one_loop(trainers[mode], data) for _ in range(2))
        passes[mode] = max(1, int(np.ceil(block_seconds / t)))
    ms = {mode: [] for mode in modes}
    for _ in range(blocks):
        for mode in modes:                                               # alternating: drift of the box hits both modes alike
            t = sum(one_loop(trainers[mode], data) for _ in range(passes[mode]))
            ms[mode].append(1e3 * t / (passes[mode] * steps))
    return {mode: {**stats(v), "passes_per_block": passes[mode]} for mode, v in ms.items()}


def effect(trainers, modes, data) -> dict:
    """Per mode, means over the trajectories of: max / min of the free scale and of the pose's scale over the frames >= 1, and the
    standard deviation over those frames of |t_pred - t_gt| (metres); with the option on also the share of (frame, trajectory) held."""
    out = {}
    for mode in modes:
        model = trainers[mode].model
        one_loop(trainers[mode], data)
        pred, feed, root = model.pred_dict, model.feed_dict, model.root
        frames = range(1, len(feed))
        scale = torch.stack([pred["poses"][i]["scale"][:, root] for i in frames]).double()                    # (T-1, B)
        free = torch.stack([pred["size"][i]["free"][:, root] for i in frames]).double() if "size" in pred else scale
        terr = torch.stack([(pred["poses"][i]["translation"][:, root] - feed[i]["gt_part"]["translation"][:, root].to(scale.device)).double().flatten(1).norm(dim=1)
                            for i in frames])
        spread = lambda x: round(float((x.max(0).values / x.min(0).values).mean()), 5)       # noqa: E731
        out[mode] = {"free_scale_spread": spread(free), "pose_scale_spread": spread(scale), "terr_std": round(float(terr.std(0).mean()), 6),
                     "terr_mean": round(float(terr.mean()), 6)}
        if "size" in pred:
            out[mode]["held_share"] = round(float(torch.stack([pred["size"][i]["held"] for i in frames]).float().mean()), 4)
            out[mode]["accepted_share"] = round(float(torch.stack([pred["size"][i]["accepted"] for i in frames]).float().mean()), 4)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--block-seconds", type=float, default=1.0)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_size needs a GPU: there is no CPU fall-back and no CPU timing")
    dev = torch.device("cuda:0")
    every = [m for pair in MODES.values() for m in pair]
    pre = {mode: make_trainer(dev, mode, otf=False) for mode in every}
    otf = {mode: make_trainer(dev, mode, otf=True) for mode in every}
    cost = {"unit": "ms per step of B trajectories (set_data included)", "frames": args.frames}
    for name, trainers, data in (("precropped B=32", pre, make_trajectory("nocs", 32, args.frames, seed=7)),
                                 ("precropped B=1", pre, make_trajectory("nocs", 1, args.frames, seed=7)),
                                 ("nocs_otf B=32", otf, otf_scene(32, args.frames, dev))):
        cost[name] = {}
        for kind, modes in MODES.items():
            cost[name].update(bench_cost(trainers, modes, data, args.blocks, args.block_seconds))
        print(f"# cost {name}: " + "  ".join(f"{m} {cost[name][m]['median']:.3f}" for m in every) + " ms per step (median)", file=sys.stderr, flush=True)
    eff = {"unit": "means over the trajectories; spreads are max / min over the frames, terr in metres", "frames": args.frames}
    for name, trainers, data in (("make_trajectory(nocs, 32, 16)", pre, make_trajectory("nocs", 32, args.frames, seed=7)),
                                 ("make_otf_trajectory step_px 6", otf, otf_scene(32, args.frames, dev, step_px=6.0)),
                                 ("make_otf_trajectory step_px 18", otf, otf_scene(32, args.frames, dev, step_px=18.0))):
        eff[name] = effect(trainers, every, data)
        print(f"# effect {name}: " + json.dumps(eff[name]), file=sys.stderr, flush=True)
    line = json.dumps({"bench": "size", "option": OPTION, "st_fit": ROBUST, "blocks": args.blocks, "block_seconds": args.block_seconds,
                       "cost": cost, "effect": eff})
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
