"""captra_rot_pool_consensus against captra_rot_pool_compose on the same inputs, and inside the captured step: N = 4096, H = 64 with
B = 32, P = 1 (sym = 0 and 1) and B = 8, P = 4 (sym = 0) on recipe votes (tests/rot_consensus_judge.py: 70 % true votes, 15 % clustered
at 90 degrees, 15 % scattered; threshold 15 degrees), and the 32-trajectory captured step (graph.TrackStepGraph on the synthetic bottle
batch) with track_cfg/rot_pool off and on, in one process, the two alternating block by block.  One JSON line.

Device figures: `--launches` launches (step: `--steps` replays) between ONE pair of events per block, median / min / max of `--reps`
blocks after a warm-up block; microseconds per launch / per step.

Usage: python tools/bench_rot_pool.py [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tests import rot_consensus_judge as RJ  # noqa: E402


def _stats(us):
    us = sorted(us)
    return {"median": round(us[(len(us) - 1) // 2], 2), "min": round(us[0], 2), "max": round(us[-1], 2), "blocks": len(us)}


def _block(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1) / launches


def _timed_pair(fns, launches, reps):
    """The functions of `fns` alternating block by block (a drift of the clocks meets both alike); the first round is the warm-up."""
    out = {k: [] for k in fns}
    for r in range(reps + 1):
        for k, fn in fns.items():
            us = _block(fn, launches)
            if r:
                out[k].append(us)
    return {k: _stats(v) for k, v in out.items()}


def build(B, P, N, sym, seed):
    """Every point belongs to one of the P parts (N / P members each, recipe votes) -> labels, raw (B*P,R,N), prev_rot, R_true."""
    rng = np.random.default_rng(seed)
    R = 3 if sym else 6
    labels = np.tile(np.arange(N, dtype=np.int32) % P, (B, 1))
    raw = rng.normal(size=(B, P, R, N)).astype(np.float32)
    true = np.zeros((B, P, 3, 3))
    for b in range(B):
        for p in range(P):
            pts = np.nonzero(labels[b] == p)[0]
            vals, _, Rt = RJ.recipe_part(rng, len(pts), sym)
            raw[b, p][:, pts], true[b, p] = vals, Rt
    prev = np.tile(np.eye(3, dtype=np.float32), (B, P, 1, 1))
    return labels, raw.reshape(B * P, R, N), prev, true


def _angle(dR, Rt, sym):
    c = np.einsum("bpi,bpi->bp", dR[..., 1], Rt[..., 1]) if sym else (np.einsum("bpij,bpij->bp", Rt, dR) - 1) / 2
    return np.rad2deg(np.arccos(np.clip(c, -1, 1)))


def kernel_case(B, P, N, sym, hyps, launches, reps, dev):
    """The two launches alone: the C ABI on pre-allocated outputs, nothing but the ctypes call between the events."""
    from captra_amd import _lib as L
    labels, raw, prev, true = build(B, P, N, sym, seed=B * 10 + P + sym)
    d = [torch.from_numpy(a).to(dev) for a in (labels, raw, prev)]
    rot, delta = torch.empty(B, P, 3, 3, device=dev), torch.empty(B, P, 3, 3, device=dev)
    i32 = [torch.empty(B, P, dtype=torch.int32, device=dev) for _ in range(3)]
    lib, stream = L.lib(), L.stream_ptr()
    cos_th = float(RJ.cos_th_of(RJ.TH_DEG))

    def plain():
        L.check(lib.captra_rot_pool_compose(B, P, N, int(sym), 1, L.ptr(d[1]), L.ptr(d[0]), L.ptr(d[2]), L.ptr(rot), L.ptr(delta), stream),
                "captra_rot_pool_compose")

    def consensus():
        L.check(lib.captra_rot_pool_consensus(B, P, N, int(sym), 1, 0, hyps, cos_th, L.ptr(d[1]), L.ptr(d[0]), L.ptr(d[2]), None, 1, L.ptr(rot),
                                              L.ptr(delta), L.ptr(i32[0]), L.ptr(i32[1]), L.ptr(i32[2]), stream), "captra_rot_pool_consensus")

    res = {}
    for name, us in _timed_pair({"plain": plain, "consensus": consensus}, launches, reps).items():
        res[f"{name}_us"] = us
    for name, fn in (("plain", plain), ("consensus", consensus)):       # what each read-out finds: degrees from the true rotation
        fn()
        torch.cuda.synchronize()
        res[f"{name}_deg_max"] = round(float(_angle(delta.cpu().numpy().astype(np.float64), true, sym).max()), 3)
    res["inlier_fraction_mean"] = round(float((i32[1].float() / i32[0].float()).mean()), 4)
    return res


def step_graph(rot_pool, B):
    from captra_amd import synthetic as clouds
    from captra_amd.configs import make_config
    from captra_amd.graph import TrackStepGraph
    from captra_amd.trainer import Trainer
    cat, objcfg, kind, _, _, wseed, _ = clouds.PHYSICAL_SETUPS["bottle"]
    cfg = make_config(cat, objcfg, experiment_dir="/tmp/captra_bench_rot_pool")
    if rot_pool is not None:
        cfg["track_cfg"]["rot_pool"] = rot_pool
    trainer = Trainer(cfg)
    model = trainer.model
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(clouds.make_physical_state_dict(shapes, wseed, cfg["num_parts"], bool(cfg["obj_sym"]), kind))
    model.eval()
    model.set_data(clouds.make_trajectory(kind, B, 2, seed=7))
    f = model.feed_dict[1]
    pose = {k: v.clone() for k, v in model.feed_dict[0]["gt_part"].items()}
    g = TrackStepGraph(model, f["points"], f["points_mean"], pose)
    return g, (lambda: g.replay(f["points"], f["points_mean"], pose))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--hyps", type=int, default=64)
    ap.add_argument("--angle_th", type=float, default=30.0, help="the step's threshold in degrees (synthetic weights: a test setting)")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rot_pool needs a GPU")
    dev = torch.device("cuda:0")
    out = {"tool": "bench_rot_pool", "device": torch.cuda.get_device_name(0), "N": args.points, "H": args.hyps,
           "timing": f"{args.launches} launches ({args.steps} steps) between one pair of events, us per launch (step), median of blocks, "
                     "the two variants alternating block by block"}
    for B, P, sym in ((32, 1, False), (32, 1, True), (8, 4, False)):
        out[f"B{B}_P{P}{'_sym' if sym else ''}"] = kernel_case(B, P, args.points, sym, args.hyps, args.launches, args.reps, dev)
    with torch.no_grad():
        g_off, off = step_graph(None, 32)
        g_on, on = step_graph({"consensus": True, "angle_th": args.angle_th, "num_hyps": args.hyps}, 32)
        step = _timed_pair({"off": off, "on": on}, args.steps, args.reps)
    out["step32_off_us"], out["step32_on_us"] = step["off"], step["on"]
    out["step32_on_minus_off_us"] = round(step["on"]["median"] - step["off"]["median"], 2)
    out["step32_inlier_fraction_mean"] = round(float((g_on.npcs_pred["rot_inliers"].float() / g_on.npcs_pred["rot_count"].float().clamp(min=1)).mean()), 4)
    line = json.dumps(out)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
