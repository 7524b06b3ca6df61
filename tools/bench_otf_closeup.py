"""The on-the-fly re-crop loop on a CLOSE-UP scene, whose crops hold more ball members than the 5 x num_points an unthinned candidate
list holds (make_otf_trajectory(..., blob_px=90): about 25 000), in three modes, alternating in one process:
  off   track_cfg/otf_thin off, sync-free stage: every frame is a rare-path frame, read a frame late and run again
  sync  track_cfg/otf_thin off, the synchronous stage (CAPTRA_OTF_DEFER=0)
  on    track_cfg/otf_thin/device True: thinned on the device, no rare path
and the same three on the shipped scene (blob_px=70), where nothing is thinned.  Prints one JSON line: median, p10 and p90 of the
milliseconds per step over the timed blocks, per scene, batch size and mode.

Usage: python tools/bench_otf_closeup.py [--batches 1 32] [--frames 16] [--blocks 7] [--block-seconds 1.0] [--out FILE]
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

import captra_amd.model as M  # noqa: E402
from captra_amd.configs import make_config  # noqa: E402
from captra_amd.synthetic import cat_trajectories, make_otf_trajectory, make_physical_state_dict  # noqa: E402
from captra_amd.trainer import Trainer  # noqa: E402

MODES = ("off", "sync", "on")


def scene(batch: int, frames: int, blob_px: int, dev):
    """`batch` trajectories: copies of two seeded ones (the host builds 2 x frames depth images, not batch x frames)."""
    singles = [make_otf_trajectory(1, frames, seed=s, blob_px=blob_px) for s in (1, 2)]
    data = singles[0] if batch == 1 else cat_trajectories([singles[b % 2] for b in range(batch)])
    for f in data:
        f["meta"]["pre_fetched"] = {k: v.to(dev) for k, v in f["meta"]["pre_fetched"].items()}
    return data


def make_trainer(dev, thin: bool):
    cfg = make_config("1", experiment_dir="/tmp/captra_otf_closeup_bench", nocs_otf=True, hipgraph=True, **{"init_frame/gt": True})
    cfg["device"] = dev
    if thin:
        cfg["track_cfg"]["otf_thin"] = {"device": True, "seed": 0}
    trainer = Trainer(cfg)
    shapes = {k: tuple(v.shape) for k, v in trainer.model.state_dict().items()}
    trainer.model.load_state_dict(make_physical_state_dict(shapes, 31, 1, True, "nocs"))
    trainer.model.eval()
    return trainer


def one_loop(trainer, data, mode: str) -> float:
    """One pass of the loop over `data` -> seconds (host clock around a device synchronisation on both sides)."""
    M.OTF_DEFER = mode != "sync"
    np.random.seed(0)
    torch.manual_seed(0)
    trainer.model.set_data(data)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    trainer.model.test(save=False, no_eval=True)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--block-seconds", type=float, default=1.0)
    ap.add_argument("--blobs", type=int, nargs="+", default=[90, 70])
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    defer0 = M.OTF_DEFER
    trainers = {"off": make_trainer(dev, False), "on": make_trainer(dev, True)}
    trainers["sync"] = trainers["off"]
    results = {}
    for blob in args.blobs:
        for batch in args.batches:
            data = scene(batch, args.frames, blob, dev)
            steps = args.frames - 1
            # warm-up: graph capture and allocator; then how many passes make a block of the wanted length
            passes = {}
            for mode in MODES:
                one_loop(trainers[mode], data, mode)
                t = min(one_loop(trainers[mode], data, mode) for _ in range(2))
                passes[mode] = max(1, int(np.ceil(args.block_seconds / t)))
            ms = {mode: [] for mode in MODES}
            for _ in range(args.blocks):
                for mode in MODES:                                           # alternating: drift of the box hits every mode alike
                    t = sum(one_loop(trainers[mode], data, mode) for _ in range(passes[mode]))
                    ms[mode].append(1e3 * t / (passes[mode] * steps))
            results.setdefault(f"blob_px={blob}", {})[f"B={batch}"] = {
                mode: {"median_ms": round(float(np.median(v)), 4), "p10_ms": round(float(np.percentile(v, 10)), 4),
                       "p90_ms": round(float(np.percentile(v, 90)), 4), "passes_per_block": passes[mode]} for mode, v in ms.items()}
            print(f"# blob_px={blob} B={batch}: " + "  ".join(f"{m} {results[f'blob_px={blob}'][f'B={batch}'][m]['median_ms']:.3f}" for m in MODES)
                  + " ms per step (median)", file=sys.stderr, flush=True)
    M.OTF_DEFER = defer0
    line = json.dumps({"bench": "otf_closeup", "num_points": 4096, "frames": args.frames, "blocks": args.blocks,
                       "block_seconds": args.block_seconds, "unit": "ms per step of B trajectories", "results": results})
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
