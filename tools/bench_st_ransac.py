"""captra_part_fit_st_ransac against captra_part_fit_st_track on the same inputs, and inside the captured step: B = 32 at N = 4096,
H = 64 with P = 1 (sym = 0 and 1) and P = 4 (drawers: sym = 0) on recipe clouds (tests/ransac_judge.py: 70 % inliers, the true rotation
given), and the 32-trajectory captured step (graph.TrackStepGraph on the synthetic bottle batch) with track_cfg/st_fit off and on, in
one process.  One JSON line.

Device figures: `--launches` launches (step: `--steps` replays) between ONE pair of events per block, median / min / max of `--reps`
blocks after a warm-up block; microseconds per launch / per step.

Usage: python tools/bench_st_ransac.py [--out FILE]
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

from tests import ransac_judge as J  # noqa: E402
from tests.sym_judge import rot_y  # noqa: E402


def _stats(us):
    us = sorted(us)
    return {"median": round(us[(len(us) - 1) // 2], 2), "min": round(us[0], 2), "max": round(us[-1], 2), "blocks": len(us)}


def _timed(fn, launches, reps):
    out = []
    for r in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        e1.synchronize()
        if r:
            out.append(1e3 * e0.elapsed_time(e1) / launches)
    return out


def build(B, P, N, sym, seed):
    """Every point belongs to one of the P parts (N / P members each, recipe clouds with one scale) -> arrays, the true rotations
    (sym: times R_y(phi)) and the true scales."""
    rng = np.random.default_rng(seed)
    labels = np.tile(np.arange(N, dtype=np.int32) % P, (B, 1))
    src, tgt = np.zeros((B, P, 3, N), np.float32), np.zeros((B, 3, N), np.float32)
    rot, scale = np.zeros((B, P, 3, 3), np.float32), np.zeros((B, P), np.float32)
    ext = 0.2
    for b in range(B):
        for p in range(P):
            pts = np.nonzero(labels[b] == p)[0]
            S, T, _, _, (R, s, _) = J.recipe_cloud(rng, len(pts), ext=ext)
            src[b, p][:, pts], tgt[b][:, pts] = S.T, T.T
            rot[b, p], scale[b, p] = (R @ rot_y(rng.uniform(0.5, 2.5)) if sym else R), s
    return labels, src, tgt, np.float32(0.02 * ext), rot, scale


def kernel_case(B, P, N, sym, hyps, launches, reps, dev):
    """The two launches alone: the C ABI on pre-allocated outputs, nothing but the ctypes call between the events."""
    from captra_amd import _lib as L
    labels, src, tgt, th, rot, scale = build(B, P, N, sym, seed=B * 10 + P + sym)
    d = [torch.from_numpy(a).to(dev) for a in (labels, src, tgt, rot)]
    mean = torch.zeros(B, 3, device=dev)
    prev_s, prev_t = torch.ones(B, P, device=dev), torch.zeros(B, P, 3, device=dev)
    o_s, o_t = torch.empty(B, P, device=dev), torch.empty(B, P, 3, device=dev)
    i32 = [torch.empty(B, P, dtype=torch.int32, device=dev) for _ in range(3)]
    lib, stream = L.lib(), L.stream_ptr()

    def plain():
        L.check(lib.captra_part_fit_st_track(B, P, N, int(sym), L.ptr(d[0]), L.ptr(d[1]), L.ptr(d[2]), L.ptr(mean), L.ptr(d[3]), L.ptr(prev_s),
                                             L.ptr(prev_t), L.ptr(o_s), L.ptr(o_t), L.ptr(i32[0]), stream), "captra_part_fit_st_track")

    def robust():
        L.check(lib.captra_part_fit_st_ransac(B, P, N, int(sym), 0, hyps, float(th), L.ptr(d[0]), L.ptr(d[1]), L.ptr(d[2]), 0, L.ptr(mean),
                                              L.ptr(d[3]), L.ptr(prev_s), L.ptr(prev_t), None, 1, L.ptr(o_s), L.ptr(o_t), L.ptr(i32[0]),
                                              L.ptr(i32[1]), L.ptr(i32[2]), stream), "captra_part_fit_st_ransac")

    res = {}
    true = torch.from_numpy(scale).to(dev)
    for name, fn in (("one_pass", plain), ("ransac", robust)):
        res[f"{name}_us"] = _stats(_timed(fn, launches, reps))
        res[f"{name}_scale_err"] = float(((o_s - true).abs() / true).max())           # (of the last launch: what each estimator finds)
    res["inliers_mean"] = float(i32[2].float().mean())
    return res


def step_case(st_fit, B, steps, reps):
    from captra_amd import synthetic as clouds
    from captra_amd.configs import make_config
    from captra_amd.graph import TrackStepGraph
    from captra_amd.trainer import Trainer
    cat, objcfg, kind, _, _, wseed, _ = clouds.PHYSICAL_SETUPS["bottle"]
    cfg = make_config(cat, objcfg, experiment_dir="/tmp/captra_bench_st_ransac")
    if st_fit is not None:
        cfg["track_cfg"]["st_fit"] = st_fit
    trainer = Trainer(cfg)
    model = trainer.model
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(clouds.make_physical_state_dict(shapes, wseed, cfg["num_parts"], bool(cfg["obj_sym"]), kind))
    model.eval()
    model.set_data(clouds.make_trajectory(kind, B, 2, seed=7))
    f = model.feed_dict[1]
    pose = {k: v.clone() for k, v in model.feed_dict[0]["gt_part"].items()}
    g = TrackStepGraph(model, f["points"], f["points_mean"], pose)
    res = {"step_us": _stats(_timed(lambda: g.replay(f["points"], f["points_mean"], pose), steps, reps))}
    if st_fit is not None:
        res["valid"] = int(g.npcs_pred["st_valid"].sum())
        res["inliers_mean"] = float(g.npcs_pred["st_inliers"].float().mean())
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--hyps", type=int, default=64)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_st_ransac needs a GPU")
    dev = torch.device("cuda:0")
    out = {"tool": "bench_st_ransac", "device": torch.cuda.get_device_name(0), "N": args.points, "H": args.hyps,
           "timing": f"{args.launches} launches ({args.steps} steps) between one pair of events, us per launch (step), median of blocks"}
    for P, sym in ((1, False), (1, True), (4, False)):
        out[f"B32_P{P}{'_sym' if sym else ''}"] = kernel_case(32, P, args.points, sym, args.hyps, args.launches, args.reps, dev)
    out["step32_off"] = step_case(None, 32, args.steps, args.reps)
    out["step32_on"] = step_case({"ransac": True}, 32, args.steps, args.reps)
    line = json.dumps(out)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
