"""The depth support filter (csrc/depth_filter.hip, track_cfg/depth_filter) priced twice, in one process:
  kernel  captra_depth_support_filter on 32 x 480 x 640 depth images (the scene with flying pixels) for windows 1, 2 and 3, many launches
          between one pair of events, against a clone() of the same tensor timed the same way -- both read and write every pixel once,
          so the copy is what the memory system allows;
  loop    the on-the-fly re-crop loop on make_otf_trajectory(..., flying=0.5) at 1 and 32 trajectories with the option on and off,
          alternating; a pass includes set_data (the upload, where the filter runs), the time is per step of B trajectories.
Prints one JSON line: median, p10 and p90 over the timed blocks.

Usage: python tools/bench_depth_filter.py [--batches 1 32] [--frames 16] [--blocks 7] [--block-seconds 1.0] [--launches 4000] [--out FILE]
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

from captra_amd import _lib as L  # noqa: E402
from captra_amd.configs import make_config  # noqa: E402
from captra_amd.nocs_otf import depth_support_filter  # noqa: E402
from captra_amd.synthetic import cat_trajectories, make_frame, make_otf_trajectory, make_physical_state_dict  # noqa: E402
from captra_amd.trainer import Trainer  # noqa: E402

OPTION = {"window": 3, "abs_mm": 10, "rel_permille": 0, "min_support": 12}
MODES = ("off", "on")


def stats(v) -> dict:
    return {"median": round(float(np.median(v)), 4), "p10": round(float(np.percentile(v, 10)), 4), "p90": round(float(np.percentile(v, 90)), 4)}


def events_us(fn, launches: int) -> float:
    """Microseconds per call of `fn`, `launches` calls between one pair of events."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(launches):
        fn()
    stop.record()
    stop.synchronize()
    return 1e3 * start.elapsed_time(stop) / launches


def bench_kernel(dev, images: int, launches: int, blocks: int) -> dict:
    frames = [make_frame(s, flying=0.5)[0].astype(np.int32) for s in range(4)]
    depth = torch.from_numpy(np.stack([frames[i % 4] for i in range(images)])).to(dev)
    B, H, W = depth.shape
    out, removed = torch.empty_like(depth), torch.zeros(B, dtype=torch.int32, device=dev)
    jobs = {"clone": depth.clone}
    for window in (1, 2, 3):
        ms = ((2 * window + 1) ** 2 - 1) // 4
        # the launch alone, into buffers that exist (the wrapper adds an allocation and the zeroing of `removed`, which here goes on
        # counting: 10^7 launches would overflow it, a run makes some 10^5)
        jobs[f"window{window}"] = lambda window=window, ms=ms: L.call("captra_depth_support_filter", B, H, W, window, 10, 0, ms, L.ptr(depth),
                                                                      L.ptr(out), L.ptr(removed))
        got = depth_support_filter(depth, window, 10, 0, ms)
        jobs[f"window{window}"]()
        assert torch.equal(got[0], out)                                      # the timed call computes what the wrapper does
    us = {name: [] for name in jobs}
    for fn in jobs.values():                                                 # warm-up: code objects, allocator
        events_us(fn, 10)
    for _ in range(blocks):
        for name, fn in jobs.items():                                        # alternating: drift of the box hits every job alike
            us[name].append(events_us(fn, launches))
    nbytes = 2 * depth.numel() * 4
    res = {"shape": list(depth.shape), "launches_per_block": launches, "bytes_read_plus_written": nbytes, "unit": "us per call",
           "note": "a window call is the launch alone, into existing buffers; clone() allocates from torch's cache"}
    for name, v in us.items():
        res[name] = {**stats(v), "GBps_at_median": round(nbytes / (np.median(v) * 1e-6) / 1e9, 1)}
    return res


def scene(batch: int, frames: int, dev):
    """`batch` trajectories: copies of two seeded ones; the images already on the device, so a pass pays no host-to-device copy."""
    singles = [make_otf_trajectory(1, frames, seed=s, flying=0.5) for s in (1, 2)]
    data = singles[0] if batch == 1 else cat_trajectories([singles[b % 2] for b in range(batch)])
    for f in data:
        f["meta"]["pre_fetched"] = {k: v.to(dev) for k, v in f["meta"]["pre_fetched"].items() if k in ("depth", "mask")}
    return data


def make_trainer(dev, on: bool):
    cfg = make_config("1", experiment_dir="/tmp/captra_depth_filter_bench", nocs_otf=True, hipgraph=True, **{"init_frame/gt": True})
    cfg["device"] = dev
    if on:
        cfg["track_cfg"]["depth_filter"] = dict(OPTION)
    trainer = Trainer(cfg)
    shapes = {k: tuple(v.shape) for k, v in trainer.model.state_dict().items()}
    trainer.model.load_state_dict(make_physical_state_dict(shapes, 31, 1, True, "nocs"))
    trainer.model.eval()
    return trainer


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


def bench_loop(dev, batches, frames: int, blocks: int, block_seconds: float) -> dict:
    trainers = {"off": make_trainer(dev, False), "on": make_trainer(dev, True)}
    out = {"unit": "ms per step of B trajectories (set_data included)", "frames": frames, "option": OPTION}
    for batch in batches:
        data = scene(batch, frames, dev)
        steps = frames - 1
        passes = {}
        for mode in MODES:
            one_loop(trainers[mode], data)                                   # warm-up: graph capture and allocator
            t = min(one_loop(trainers[mode], data) for _ in range(2))
            passes[mode] = max(1, int(np.ceil(block_seconds / t)))
        ms = {mode: [] for mode in MODES}
        for _ in range(blocks):
            for mode in MODES:
                t = sum(one_loop(trainers[mode], data) for _ in range(passes[mode]))
                ms[mode].append(1e3 * t / (passes[mode] * steps))
        out[f"B={batch}"] = {mode: {**stats(v), "passes_per_block": passes[mode]} for mode, v in ms.items()}
        print(f"# loop B={batch}: " + "  ".join(f"{m} {out[f'B={batch}'][m]['median']:.3f}" for m in MODES) + " ms per step (median)",
              file=sys.stderr, flush=True)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--block-seconds", type=float, default=1.0)
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--launches", type=int, default=4000)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_depth_filter needs a GPU: there is no CPU fall-back and no CPU timing")
    dev = torch.device("cuda:0")
    kernel = bench_kernel(dev, args.images, args.launches, args.blocks)
    print("# kernel: " + "  ".join(f"{k} {v['median']:.1f}" for k, v in kernel.items() if isinstance(v, dict)) + " us per call (median)",
          file=sys.stderr, flush=True)
    loop = bench_loop(dev, args.batches, args.frames, args.blocks, args.block_seconds)
    line = json.dumps({"bench": "depth_filter", "blocks": args.blocks, "block_seconds": args.block_seconds, "kernel": kernel, "loop": loop})
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
