"""captra_part_fit_guard alone and inside the captured step: B in {1, 32} x P in {1, 4} at N = 4096 on recipe clouds
(tests/ransac_judge.py: 70 % inliers) with no part lost (the true poses) and with every part lost (poses 3 th off, refit on), and the
32-trajectory captured step (graph.TrackStepGraph on the synthetic bottle batch) with the guard off, monitoring and refitting, in
one process.  One JSON line.

Device figures: `--launches` launches (step: `--steps` replays) between ONE pair of events per block, median / min / max of `--reps`
blocks after a warm-up block; microseconds per launch / per step.  The refitting step runs with lost_below = 1, which sends every
part that has a single outlier into the re-fit: the most the guard can cost.

--yaxis-only: every figure a second time, in the same process, with the axis-only inlier test of the symmetric categories
(captra_part_fit_guard_sym; track_cfg/guard/yaxis_only in the step), under keys that end in `_yaxis`.

Usage: python tools/bench_track_guard.py [--yaxis-only] [--out FILE]
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

from captra_amd.pose_utils.pose_fit import part_fit_guard_cn  # noqa: E402
from tests import ransac_judge as J  # noqa: E402


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


def build(B, P, N, seed):
    """Every point belongs to one of the P parts (N / P members each, recipe clouds with one scale) -> arrays and the true poses."""
    rng = np.random.default_rng(seed)
    labels = np.tile(np.arange(N, dtype=np.int32) % P, (B, 1))
    src, tgt = np.zeros((B, P, 3, N), np.float32), np.zeros((B, 3, N), np.float32)
    rot, scale, trans = np.zeros((B, P, 3, 3), np.float32), np.zeros((B, P), np.float32), np.zeros((B, P, 3, 1), np.float32)
    ext = 0.2
    for b in range(B):
        for p in range(P):
            pts = np.nonzero(labels[b] == p)[0]
            S, T, th, _, (R, s, t) = J.recipe_cloud(rng, len(pts), ext=ext)
            src[b, p][:, pts], tgt[b][:, pts] = S.T, T.T
            rot[b, p], scale[b, p], trans[b, p, :, 0] = R, s, t
    return labels, src, tgt, np.float32(0.02 * ext), rot, scale, trans


def _direct(d, th, hyps, B, P, N, dev, sym=False):
    """The launch alone: the C ABI on pre-allocated outputs, nothing but the ctypes call between the events."""
    from captra_amd import _lib as L
    i32 = [torch.empty(B, P, dtype=torch.int32, device=dev) for _ in range(3)]
    rms = torch.empty(B, P, device=dev)
    po = (torch.empty(B, P, 3, 3, device=dev), torch.empty(B, P, device=dev), torch.empty(B, P, 3, device=dev))
    name = "captra_part_fit_guard_sym" if sym else "captra_part_fit_guard"
    fn, stream = getattr(L.lib(), name), L.stream_ptr()
    fixed = (B, P, N, 0, L.ptr(d[0]), L.ptr(d[1]), L.ptr(d[2]), None)
    outs = (L.ptr(i32[0]), L.ptr(i32[1]), L.ptr(rms), L.ptr(i32[2]), L.ptr(po[0]), L.ptr(po[1]), L.ptr(po[2]), stream)

    def run(pose, refit):
        ptrs = (pose["rotation"].data_ptr(), pose["scale"].data_ptr(), pose["translation"].data_ptr())
        L.check(fn(*fixed, *ptrs, th, 1, 2, 4, 1 if refit else 0, hyps, 1, *outs), name)
    run.keep = (i32, rms, po)
    return run


def step_case(guard, B, steps, reps):
    from captra_amd import synthetic as clouds
    from captra_amd.configs import make_config
    from captra_amd.graph import TrackStepGraph
    from captra_amd.trainer import Trainer
    cat, objcfg, kind, _, _, wseed, _ = clouds.PHYSICAL_SETUPS["bottle"]
    cfg = make_config(cat, objcfg, experiment_dir="/tmp/captra_bench_guard")
    if guard is not None:
        cfg["track_cfg"]["guard"] = guard
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
    if guard is not None:
        res["verdicts"] = np.bincount(g.npcs_pred["guard_verdict"].cpu().numpy().ravel(), minlength=4).tolist()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--hyps", type=int, default=64)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--yaxis-only", action="store_true", help="measure the axis-only inlier test too, beside the full-rotation one")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_track_guard needs a GPU")
    tests = ((False, ""), (True, "_yaxis")) if args.yaxis_only else ((False, ""),)
    dev = torch.device("cuda:0")
    out = {"tool": "bench_track_guard", "device": torch.cuda.get_device_name(0), "N": args.points, "H": args.hyps,
           "timing": f"{args.launches} launches ({args.steps} steps) between one pair of events, us per launch (step), median of blocks"}
    for B in (1, 32):
        for P in (1, 4):
            labels, src, tgt, th, rot, scale, trans = build(B, P, args.points, seed=B * 10 + P)
            d = [torch.from_numpy(a).to(dev) for a in (labels, src, tgt)]
            good = {"rotation": torch.from_numpy(rot).to(dev), "scale": torch.from_numpy(scale).to(dev), "translation": torch.from_numpy(trans).to(dev)}
            bad = dict(good, translation=good["translation"] + 3 * float(th))
            for sym, sfx in tests:
                check = lambda pose, refit: part_fit_guard_cn(d[0], d[1], d[2], None, pose, inlier_th=float(th), lost_below=0.5, refit=refit,   # noqa: E731
                                                              num_hyps=args.hyps, seed=1, yaxis_only=sym)
                v_ok, v_lost = check(good, False)[1]["verdict"], check(bad, True)[1]["verdict"]
                run = _direct(d, float(th), args.hyps, B, P, args.points, dev, sym)
                out[f"B{B}_P{P}{sfx}"] = {"none_lost_verdicts": np.bincount(v_ok.cpu().numpy().ravel(), minlength=4).tolist(),
                                          "all_lost_verdicts": np.bincount(v_lost.cpu().numpy().ravel(), minlength=4).tolist(),
                                          "none_lost_us": _stats(_timed(lambda: run(good, False), args.launches, args.reps)),
                                          "none_lost_refit_on_us": _stats(_timed(lambda: run(good, True), args.launches, args.reps)),
                                          "all_lost_refit_us": _stats(_timed(lambda: run(bad, True), args.launches, args.reps))}
    out["step32_off"] = step_case(None, 32, args.steps, args.reps)
    for sym, sfx in tests:
        for name, guard in (("monitoring", {"refit": False, "lost_below": 1.0}), ("refitting", {"refit": True, "lost_below": 1.0})):
            out[f"step32_{name}{sfx}"] = step_case(dict(guard, yaxis_only=True) if sym else guard, 32, args.steps, args.reps)
    line = json.dumps(out)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
