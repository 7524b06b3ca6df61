"""Holding the track's box (csrc/pose_box.hip, track_cfg/box) measured three times, in one process:
  launch  captra_part_box_hist alone at B = 32, N = 4096 for P = 1 and P = 4, 128 and 512 bins, in both LDS forms (one histogram per
          workgroup / one per wave: captra_part_box_set_subhists), against clone() of the NOCS maps it reads once -- microseconds per
          launch from replays of a captured graph of 50 launches between one pair of events, jobs alternating;
  cost    ms per step with the option off and on, alternating: the pre-cropped hipGraph loop at 32 trajectories and at one.  The
          yardstick is the off mode of the same run: the on mode's median is reported against the off mode's p10-p90 band;
  effect  make_trajectory('nocs', 32, 16) with make_physical_state_dict's weights and OUTLIERS planted into CoordinateNet's NOCS maps
          (a share of every cloud's points replaced by uniform draws from the NOCS cube, the same draws off and on): the spread
          (max / min over the frames, mean over trajectories and axes) of the per-frame maximum -- the reference's box --, of the
          per-frame quantile and of the held box, their means against the ground-truth half-extents, and the three box IoUs of
          compute_loss(eval_iou=True) off and on.  The weights are not a trained network's.
Prints one JSON line.

Usage: python tools/bench_box.py [--blocks 7] [--block-seconds 1.0] [--frames 16] [--out profiles/box_bench.json]
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

from captra_amd import _lib  # noqa: E402
from captra_amd.configs import make_config  # noqa: E402
from captra_amd.pose_utils.pose_fit import part_box_hist  # noqa: E402
from captra_amd.synthetic import make_physical_state_dict, make_trajectory  # noqa: E402
from captra_amd.trainer import Trainer  # noqa: E402

# a test setting, not a recommendation: the quantile depends on the trained network's outlier rate
OPTION = {"hold": True, "quantile": 0.95, "bins": 128, "min_points": 16, "radial": True}
OUTLIERS = 0.02
GRAPH_LAUNCHES = 50


def stats(v) -> dict:
    return {"median": round(float(np.median(v)), 4), "p10": round(float(np.percentile(v, 10)), 4), "p90": round(float(np.percentile(v, 90)), 4)}


# ---- the launch alone ----------------------------------------------------------------------------------------------------------
def launch_inputs(dev, B: int, P: int, N: int, bins: int):
    """A cuboid's surface with 4 mm noise and 2 % outliers per part (most members fall into a handful of bins), labels uniform over
    the parts, a state of ten such frames."""
    g = torch.Generator(device="cpu").manual_seed(P * 1000 + bins)
    half = torch.tensor([0.11, 0.34, 0.11])
    pts = (torch.rand(B, P, N, 3, generator=g) * 2 - 1) * half
    face = torch.randint(0, 3, (B, P, N), generator=g)
    sign = torch.where(torch.rand(B, P, N, generator=g) < 0.5, -1.0, 1.0)
    pts.scatter_(-1, face[..., None], (sign * half[face])[..., None])
    pts += 0.004 * torch.randn(B, P, N, 3, generator=g)
    out = torch.rand(B, P, N, generator=g) < OUTLIERS
    pts[out] = torch.rand(int(out.sum()), 3, generator=g) - 0.5
    src = pts.transpose(-1, -2).contiguous().to(dev)
    labels = torch.randint(0, P, (B, N), generator=g, dtype=torch.int32).to(dev)
    state = None
    for _ in range(10):
        state, _ = part_box_hist(labels, src, state, bins=bins, radial=False, quantile_permille=950, min_points=16)
    return labels, src, state


def bench_launch(dev, blocks: int, launches: int) -> dict:
    B, N = 32, 4096
    jobs = {}
    for P in (1, 4):
        for bins in (128, 512):
            labels, src, state = launch_inputs(dev, B, P, N, bins)
            jobs[f"clone P={P}"] = (lambda src=src: src.clone(), 0)
            for sub in (1, 4):
                jobs[f"box P={P} bins={bins} subhists={sub}"] = (
                    lambda labels=labels, src=src, state=state, bins=bins: part_box_hist(labels, src, state, bins=bins, radial=False,
                                                                                           quantile_permille=950, min_points=16), sub)
    # Each job is captured as a hipGraph of GRAPH_LAUNCHES launches back to back, as the step's launches are: launched one by one
    # from Python the binding's own 14 us per call (five output tensors, the ctypes call) hide a kernel of a few microseconds.
    graphs = {}
    side = torch.cuda.Stream(device=dev)
    for name, (fn, sub) in jobs.items():
        _lib.lib().captra_part_box_set_subhists(sub)                     # (the LDS form is chosen at the launch: captured with it)
        with torch.cuda.stream(side):
            fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            keep = [fn() for _ in range(GRAPH_LAUNCHES)]
        graphs[name] = (g, keep)
    _lib.lib().captra_part_box_set_subhists(0)
    replays = max(1, launches // GRAPH_LAUNCHES)
    us = {name: [] for name in jobs}
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for block in range(blocks + 1):                                      # (block 0 warms up)
        for name, (g, _) in graphs.items():                              # alternating: drift hits every job alike
            g.replay()
            torch.cuda.synchronize()
            start.record()
            for _ in range(replays):
                g.replay()
            stop.record()
            torch.cuda.synchronize()
            if block:
                us[name].append(1e3 * start.elapsed_time(stop) / (replays * GRAPH_LAUNCHES))
    return {"unit": f"microseconds per launch, {GRAPH_LAUNCHES} launches back to back in one captured graph", "B": B, "N": N,
            "launches_per_block": replays * GRAPH_LAUNCHES,
            "src_bytes": {f"P={P}": B * P * 3 * N * 4 for P in (1, 4)}, **{name: stats(v) for name, v in us.items()}}


# ---- the loop --------------------------------------------------------------------------------------------------------------------
def make_trainer(dev, on: bool, hipgraph: bool = True, eval_device: bool = False):
    cfg = make_config("1", experiment_dir="/tmp/captra_box_bench", hipgraph=hipgraph, **{"init_frame/gt": True})
    cfg["device"] = dev
    if eval_device:
        cfg["eval_device"] = True
    if on:
        cfg["track_cfg"]["box"] = dict(OPTION)
    trainer = Trainer(cfg)
    shapes = {k: tuple(v.shape) for k, v in trainer.model.state_dict().items()}
    trainer.model.load_state_dict(make_physical_state_dict(shapes, 31, 1, True, "nocs"))
    trainer.model.eval()
    return trainer


def one_loop(trainer, data, no_eval: bool = True) -> float:
    """One pass (set_data + the loop) over `data` -> seconds (host clock around a device synchronisation on both sides)."""
    np.random.seed(0)
    torch.manual_seed(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    trainer.model.set_data(data)
    trainer.model.test(save=False, no_eval=no_eval)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def bench_cost(trainers, data, blocks: int, block_seconds: float) -> dict:
    steps = len(data) - 1
    passes = {}
    for mode in trainers:
        one_loop(trainers[mode], data)                                   # warm-up: graph capture and allocator
        t = min(one_loop(trainers[mode], data) for _ in range(2))
        passes[mode] = max(1, int(np.ceil(block_seconds / t)))
    ms = {mode: [] for mode in trainers}
    for _ in range(blocks):
        for mode in trainers:                                            # alternating: drift of the machine hits both modes alike
            t = sum(one_loop(trainers[mode], data) for _ in range(passes[mode]))
            ms[mode].append(1e3 * t / (passes[mode] * steps))
    out = {mode: {**stats(v), "passes_per_block": passes[mode]} for mode, v in ms.items()}
    off, on = out["off"], out["on"]["median"]
    out["on_against_off_band"] = "inside" if off["p10"] <= on <= off["p90"] else f"{on - off['p90']:+.4f} ms beyond p90" if on > off["p90"] else f"{on - off['p10']:+.4f} ms below p10"
    return out


# ---- the effect ------------------------------------------------------------------------------------------------------------------
class PlantedOutliers:
    """A forward hook on CoordinateNet: a share of every cloud's points gets uniform draws from the NOCS cube in place of its predicted
    coordinates (all parts' maps of the point), from a generator seeded per run: the same draws with the option off and on."""

    def __init__(self, share: float, dev):
        self.share, self.dev, self.gen = share, dev, None

    def reset(self):
        self.gen = torch.Generator(device=self.dev).manual_seed(99)

    def __call__(self, module, args, output):
        nocs = output["nocs"]                                            # (B, 3 P, N)
        B, C, N = nocs.shape
        hit = torch.rand(B, 1, N, device=nocs.device, generator=self.gen) < self.share
        draws = torch.rand(B, C, N, device=nocs.device, generator=self.gen) - 0.5
        output["nocs"] = torch.where(hit, draws.to(nocs.dtype), nocs)
        return output


def effect(trainers, data, hook) -> dict:
    from captra_amd.loss import choose_coord_by_label
    from captra_amd.pose_utils.bbox_utils import pred_nocs_corners_device
    out = {}
    for mode, trainer in trainers.items():
        model = trainer.model
        handle = model.npcs_net.register_forward_hook(hook)
        hook.reset()
        try:
            one_loop(trainer, data, no_eval=False)
        finally:
            handle.remove()
        pred, feed = model.pred_dict, model.feed_dict
        frames = range(1, len(feed))
        gt = feed[0]["meta"]["nocs_corners"].abs().amax(-2).to(model.device).double()                          # (B,P,3)
        per_max = []
        for i in frames:
            labels = torch.max(pred["npcs_pred"][i]["seg"], dim=-2)[1]
            own = choose_coord_by_label(pred["npcs_pred"][i]["nocs"].transpose(-1, -2), labels)
            per_max.append(pred_nocs_corners_device(labels, own, model.num_parts)[..., 1, :].double())
        per_max = torch.stack(per_max)                                                                       # (T-1,B,P,3)
        spread = lambda x: round(float((x.amax(0) / x.amin(0).clamp_min(1e-9)).mean()), 5)       # noqa: E731
        ratio = lambda x: round(float((x / gt).mean()), 5)                                        # noqa: E731
        row = {"frame_max_spread": spread(per_max), "frame_max_over_gt": ratio(per_max),
               "iou": {name: {str(p): round(float(v), 5) for p, v in d.items()} for name, d in model.loss_dict["avg_iou"].items()}}
        if "box" in pred:
            own_q = torch.stack([pred["box"][i]["frame"] for i in frames]).double()
            held = torch.stack([pred["box"][i]["extent"] for i in frames]).double()
            row.update({"frame_quantile_spread": spread(own_q), "frame_quantile_over_gt": ratio(own_q), "held_spread": spread(held),
                        "held_over_gt": ratio(held), "established_share": round(float((held > 0).all(-1).double().mean()), 4)})
        out[mode] = row
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--block-seconds", type=float, default=1.0)
    ap.add_argument("--launches", type=int, default=2000)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_box needs a GPU: there is no CPU fall-back and no CPU timing")
    dev = torch.device("cuda:0")
    launch = bench_launch(dev, args.blocks, args.launches)
    for name, v in launch.items():
        if isinstance(v, dict) and "median" in v:
            print(f"# launch {name}: {v['median']:.2f} us (p10 {v['p10']:.2f}, p90 {v['p90']:.2f})", file=sys.stderr, flush=True)
    trainers = {"off": make_trainer(dev, False), "on": make_trainer(dev, True)}
    cost = {"unit": "ms per step of B trajectories (set_data included)", "frames": args.frames}
    for name, data in (("precropped B=32", make_trajectory("nocs", 32, args.frames, seed=7)), ("precropped B=1", make_trajectory("nocs", 1, args.frames, seed=7))):
        cost[name] = bench_cost(trainers, data, args.blocks, args.block_seconds)
        print(f"# cost {name}: off {cost[name]['off']['median']:.3f} (p10 {cost[name]['off']['p10']:.3f}, p90 {cost[name]['off']['p90']:.3f})  "
              f"on {cost[name]['on']['median']:.3f} ms per step: {cost[name]['on_against_off_band']}", file=sys.stderr, flush=True)
    eager = {"off": make_trainer(dev, False, hipgraph=False, eval_device=True), "on": make_trainer(dev, True, hipgraph=False, eval_device=True)}
    eff = {"unit": "means over trajectories and axes; spreads are max / min over the frames; *_over_gt against the ground-truth half-extents",
           "frames": args.frames, "outliers": OUTLIERS,
           "make_trajectory(nocs, 32, frames)": effect(eager, make_trajectory("nocs", 32, args.frames, seed=7), PlantedOutliers(OUTLIERS, dev))}
    print("# effect: " + json.dumps(eff["make_trajectory(nocs, 32, frames)"]), file=sys.stderr, flush=True)
    line = json.dumps({"bench": "box", "option": OPTION, "blocks": args.blocks, "block_seconds": args.block_seconds, "launch": launch, "cost": cost,
                       "effect": eff})
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
