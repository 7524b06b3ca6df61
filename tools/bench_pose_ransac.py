"""captra_part_fit_ransac alone: B in {1, 32} x P in {1, 4} at N = 4096, H = 64, on recipe clouds (tests/ransac_judge.py: 70 %
inliers), beside captra_part_fit_st at the same shape (the yardstick of a one-pass fit) and the numpy float32 mirror of ONE part
on the host.  One JSON line.

Device figures: `--launches` launches between ONE pair of events per block, median / min / max of `--reps` blocks after a warm-up
block; microseconds per launch.  Host figure: wall clock of the mirror, median of `--host_reps` calls.

Usage: python tools/bench_pose_ransac.py [--yaxis-only] [--out FILE]   (--yaxis-only: captra_part_fit_ransac_sym too, same process)
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

from captra_amd.pose_utils.pose_fit import part_fit_ransac_cn, part_fit_st_cn  # noqa: E402
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
    """Every point belongs to one of the P parts (N / P members each, recipe clouds with one scale); one target per trajectory."""
    rng = np.random.default_rng(seed)
    labels = np.tile(np.arange(N, dtype=np.int32) % P, (B, 1))
    src, tgt = np.zeros((B, P, 3, N), np.float32), np.zeros((B, 3, N), np.float32)
    ext = 0.2
    for b in range(B):
        for p in range(P):
            pts = np.nonzero(labels[b] == p)[0]
            S, T, th, _, _ = J.recipe_cloud(rng, len(pts), ext=ext)
            src[b, p][:, pts], tgt[b][:, pts] = S.T, T.T
    return labels, src, tgt, np.float32(0.02 * ext)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--hyps", type=int, default=64)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host_reps", type=int, default=5)
    ap.add_argument("--yaxis-only", action="store_true",
                    help="captra_part_fit_ransac_sym (the axis-only inlier test) too, in the same process: ransac_yaxis_us")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pose_ransac needs a GPU")
    dev = torch.device("cuda:0")
    out = {"tool": "bench_pose_ransac", "device": torch.cuda.get_device_name(0), "N": args.points, "H": args.hyps,
           "timing": f"{args.launches} launches between one pair of events, us per launch, median of blocks"}
    for B in (1, 32):
        for P in (1, 4):
            labels, src, tgt, th = build(B, P, args.points, seed=B * 10 + P)
            d = [torch.from_numpy(a).to(dev) for a in (labels, src, tgt)]
            rot = torch.eye(3, device=dev).expand(B, P, 3, 3).contiguous()
            ransac = lambda: part_fit_ransac_cn(d[0], d[1], d[2], num_hyps=args.hyps, inlier_th=float(th), seed=1)   # noqa: E731
            st = lambda: part_fit_st_cn(d[0], d[1], d[2], rot, False)                                               # noqa: E731
            valid, info = ransac()[3:]
            res = {"valid_fits": int(valid.sum()), "inliers_mean": float(info["num_inliers"].float().mean()),
                   "ransac_us": _stats(_timed(ransac, args.launches, args.reps)), "part_fit_st_us": _stats(_timed(st, args.launches, args.reps))}
            if args.yaxis_only:
                sym = lambda: part_fit_ransac_cn(d[0], d[1], d[2], num_hyps=args.hyps, inlier_th=float(th), seed=1, yaxis_only=True)   # noqa: E731
                valid, info = sym()[3:]
                res.update(valid_fits_yaxis=int(valid.sum()), inliers_mean_yaxis=float(info["num_inliers"].float().mean()),
                           ransac_yaxis_us=_stats(_timed(sym, args.launches, args.reps)))
            if B == 1:      # the float32 mirror of one part on the host
                pts = np.nonzero(labels[0] == 0)[0]
                S, T = src[0, 0][:, pts].T.copy(), tgt[0][:, pts].T.copy()
                tri = J.draw_ranks(1, 0, 0, args.hyps, len(pts))
                ms = []
                for _ in range(args.host_reps):
                    t0 = time.perf_counter()
                    J.fit(S, T, tri, float(th), np.float32)
                    ms.append(1e6 * (time.perf_counter() - t0))
                res["host_mirror_one_part_us"] = _stats(ms)
            out[f"B{B}_P{P}"] = res
    line = json.dumps(out)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
