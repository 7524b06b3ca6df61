"""The camera model (csrc/crop.hip, csrc/image_fit.hip: the *_cam entry points; the `camera` option) priced in the on-the-fly re-crop
loop, in one process: the hipGraph loop on make_otf_trajectory at 32 trajectories and at one, in three modes that alternate --
  off   no camera anywhere: the plain entry points;
  one   every trajectory carries the NOCS REAL camera: a table of one row;
  each  every trajectory carries a camera of its own (the NOCS REAL matrix with the principal point moved by b / 1024 of a pixel: the
        same work, B distinct rows).
A pass includes set_data (where the table is built and uploaded); the time is per step of B trajectories.  The yardstick is the off
mode of the same run: for each on mode the result says whether its median lies inside the off mode's p10 - p90 band.
Prints one JSON line: median, p10 and p90 over the timed blocks.

Usage: python tools/bench_camera.py [--batches 32 1] [--frames 16] [--blocks 7] [--block-seconds 1.0] [--out FILE]
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
from captra_amd.nocs_otf import NOCS_REAL_INTRINSICS  # noqa: E402
from captra_amd.synthetic import cat_trajectories, make_otf_trajectory, make_physical_state_dict  # noqa: E402
from captra_amd.trainer import Trainer  # noqa: E402

MODES = ("off", "one", "each")


def stats(v) -> dict:
    return {"median": round(float(np.median(v)), 4), "p10": round(float(np.percentile(v, 10)), 4), "p90": round(float(np.percentile(v, 90)), 4)}


def scenes(batch: int, frames: int, dev) -> dict:
    """mode -> `batch` trajectories (copies of two seeded ones; the images already on the device, shared by the three modes, so a pass
    pays no host-to-device copy of an image), with the mode's cameras in every frame's meta['pre_fetched']."""
    singles = [make_otf_trajectory(1, frames, seed=s) for s in (1, 2)]
    base = singles[0] if batch == 1 else cat_trajectories([singles[b % 2] for b in range(batch)])
    images = [{k: v.to(dev) for k, v in f["meta"]["pre_fetched"].items() if k in ("depth", "mask")} for f in base]
    K_one = np.broadcast_to(NOCS_REAL_INTRINSICS, (batch, 3, 3)).copy()
    K_each = K_one.copy()
    K_each[:, 0, 2] += np.arange(batch) / 1024.0
    unit = torch.full((batch,), 0.001, dtype=torch.float64)
    out = {}
    for mode, K in (("off", None), ("one", K_one), ("each", K_each)):
        data = []
        for f, img in zip(base, images):
            pre = dict(img)
            if K is not None:
                pre["camera"] = {"K": torch.from_numpy(K), "depth_unit": unit}
            data.append({**f, "meta": {**f["meta"], "pre_fetched": pre}})
        out[mode] = data
    return out


def make_trainer(dev):
    cfg = make_config("1", experiment_dir="/tmp/captra_camera_bench", nocs_otf=True, hipgraph=True, **{"init_frame/gt": True})
    cfg["device"] = dev
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
    trainer = make_trainer(dev)                      # ONE model: the camera is the data's, so the three modes share every buffer and graph
    out = {"unit": "ms per step of B trajectories (set_data included)", "frames": frames}
    for batch in batches:
        data = scenes(batch, frames, dev)
        steps = frames - 1
        passes = {}
        for mode in MODES:
            one_loop(trainer, data[mode])                                    # warm-up: graph capture and allocator
            assert (trainer.model.camera is None) == (mode == "off")
            if mode != "off":
                assert trainer.model.camera[0].shape[0] == (1 if mode == "one" else batch)
            t = min(one_loop(trainer, data[mode]) for _ in range(2))
            passes[mode] = max(1, int(np.ceil(block_seconds / t)))
        ms = {mode: [] for mode in MODES}
        for _ in range(blocks):
            for mode in MODES:                                               # alternating: drift of the box hits every mode alike
                t = sum(one_loop(trainer, data[mode]) for _ in range(passes[mode]))
                ms[mode].append(1e3 * t / (passes[mode] * steps))
        res = {mode: {**stats(v), "passes_per_block": passes[mode]} for mode, v in ms.items()}
        for mode in MODES[1:]:
            res[mode]["median_inside_off_p10_p90"] = bool(res["off"]["p10"] <= res[mode]["median"] <= res["off"]["p90"])
            res[mode]["median_over_off_median"] = round(res[mode]["median"] / res["off"]["median"], 4)
        out[f"B={batch}"] = res
        print(f"# loop B={batch}: " + "  ".join(f"{m} {res[m]['median']:.3f}" for m in MODES) + " ms per step (median)", file=sys.stderr, flush=True)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batches", type=int, nargs="+", default=[32, 1])
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--block-seconds", type=float, default=1.0)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_camera needs a GPU: there is no CPU fall-back and no CPU timing")
    loop = bench_loop(torch.device("cuda:0"), args.batches, args.frames, args.blocks, args.block_seconds)
    line = json.dumps({"bench": "camera", "blocks": args.blocks, "block_seconds": args.block_seconds, "loop": loop})
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
