"""The first-pose image fit (csrc/image_fit.hip, init_frame/image_fit) priced in one process, on 32 images of 480 x 640 (copies of four
seeded frames with their rendered coordinate images), at border 0 and 2:
  members  captra_image_members alone, the launch into existing buffers, many launches between one pair of events -- with the launcher's
           own geometry and with 1, 4 and 75 workgroups per image (captra_image_members_set_split): the forms the kernel was chosen among;
  chain    image_members + part_fit_ransac_cn as the model calls them (allocations included);
  clone    clone() of the depth tensor timed the same way: the yardstick for "the images read once";
  host     the numpy judge (tests/image_fit_judge.py) on the four distinct images, per image, for scale.
The jobs alternate, so a drift of the box hits every job alike.  Prints one JSON line: median, p10 and p90 over the timed blocks.

Usage: python tools/bench_image_fit.py [--images 32] [--blocks 7] [--launches 2000] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from captra_amd import _lib as L  # noqa: E402
from captra_amd.nocs_otf import NOCS_REAL_INTRINSICS, _intrinsics_on_device, image_members  # noqa: E402
from captra_amd.pose_utils.pose_fit import part_fit_ransac_cn  # noqa: E402
from captra_amd.synthetic import make_frame, render_coord_image  # noqa: E402

CAP, INLIER_TH, SPLITS = 16384, 0.003, (0, 1, 4, 75)


def stats(v) -> dict:
    return {"median": round(float(np.median(v)), 3), "p10": round(float(np.percentile(v, 10)), 3), "p90": round(float(np.percentile(v, 90)), 3)}


def events_us(fn, launches: int) -> float:
    """Microseconds per call of `fn`, `launches` calls between one pair of events."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(launches):
        fn()
    stop.record()
    stop.synchronize()
    return 1e3 * start.elapsed_time(stop) / launches


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--launches", type=int, default=2000)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_image_fit needs a GPU: there is no CPU fall-back and no CPU timing of the kernel")
    dev = torch.device("cuda:0")
    frames = [make_frame(s) for s in range(4)]
    host = [(f[0].astype(np.int32), f[1].astype(np.uint8), render_coord_image(f[0], f[1], f[3])) for f in frames]
    depth, mask, coord = (torch.from_numpy(np.stack([host[i % 4][k] for i in range(args.images)])).to(dev) for k in range(3))
    B, H, W = depth.shape
    kinv = _intrinsics_on_device(NOCS_REAL_INTRINSICS, dev)[9:]
    lib = L.lib()
    jobs, counts = {"clone": depth.clone}, {}
    for border in (0, 2):
        out = image_members(depth, mask, coord, cap=CAP, border=border)
        counts[f"border{border}"] = out["counts"][:4].cpu().tolist()

        def launch(border=border, out=out):
            L.call("captra_image_members", B, H, W, CAP, border, 0, L.ptr(depth), L.ptr(mask), L.ptr(coord), L.ptr(kinv), L.ptr(out["src"]),
                   L.ptr(out["tgt"]), L.ptr(out["labels"]), L.ptr(out["pix"]), L.ptr(out["counts"]))

        for split in SPLITS:
            def with_split(split=split, launch=launch):
                lib.captra_image_members_set_split(ctypes.c_int(split))
                launch()
                lib.captra_image_members_set_split(ctypes.c_int(0))
            jobs[f"members_border{border}_split{split or 'auto'}"] = with_split
            ref = {k: v.clone() for k, v in out.items()}
            with_split()
            assert all(torch.equal(ref[k], out[k]) for k in out)                 # every geometry computes what the wrapper did

        def chain(border=border):
            m = image_members(depth, mask, coord, cap=CAP, border=border)
            return part_fit_ransac_cn(m["labels"], m["src"], m["tgt"], num_hyps=64, inlier_th=INLIER_TH)
        assert bool(chain()[3].all())
        jobs[f"chain_border{border}"] = chain
    us = {name: [] for name in jobs}
    for fn in jobs.values():                                                     # warm-up: code objects, allocator
        events_us(fn, 10)
    for _ in range(args.blocks):
        for name, fn in jobs.items():
            us[name].append(events_us(fn, args.launches if name.startswith(("members", "clone")) else max(args.launches // 10, 10)))
    from tests import image_fit_judge as IJ
    host_ms = {}
    for border in (0, 2):
        t0 = time.perf_counter()
        for d, m, c in host:
            IJ.members(d[None], m[None], c[None], IJ.kinv_of(NOCS_REAL_INTRINSICS), CAP, border)
        host_ms[f"border{border}"] = round(1e3 * (time.perf_counter() - t0) / len(host), 2)
    res = {"bench": "image_fit", "shape": [B, H, W], "cap": CAP, "blocks": args.blocks, "launches_per_block": args.launches, "unit": "us per call",
           "members_used_holes_of_the_four_frames": counts, "images_read_once_bytes": B * H * W * 8,
           "host_numpy_judge_ms_per_image": host_ms,
           "note": "a members call is the launch alone, into existing buffers; chain = the wrapper and the fit, allocations included; clone() of the depth tensor reads and writes 4 bytes per pixel"}
    for name, v in us.items():
        res[name] = stats(v)
    print("# " + "  ".join(f"{k} {v['median']:.1f}" for k, v in res.items() if isinstance(v, dict) and "median" in v) + " us per call (median)",
          file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
