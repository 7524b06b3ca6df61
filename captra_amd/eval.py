"""`python -m captra_amd.eval`: error tables from the per-trajectory result pickles (counterpart of the reference's
misc/eval/eval.py:27-111).  For every frame after the first of every `<experiment_dir>/results/data/*.pkl`
(written by `captra_amd.track --save`, layout of model.py:482-509): rotation / translation / scale errors and the
5 deg 5 cm / 10 deg 10 cm flags per part (part_dof_utils.py:54-67), box IoUs (pose_utils/bbox_utils.py), and for
articulated objects the joint-state error; writes results/err.pkl + results/err.csv and prints the averages.
`--eval_device` computes the box IoUs on the GPU, all frames of a pickle in one call (same columns; grid IoUs agree with the
host protocol within the grid's resolution).
"""
from __future__ import annotations

import argparse
import os
import pickle
from os.path import join as pjoin

import numpy as np
import torch

from .configs.config import get_config
from .pose_utils.bbox_utils import eval_instance_part_iou, eval_single_part_iou_device
from .pose_utils.metrics import rot_diff_degree
from .pose_utils.part_dof_utils import eval_part_full


def get_joint_state(info: dict, pose: dict) -> np.ndarray:
    """Joint value of every child part w.r.t. its parent: relative rotation angle (revolute) or the offset along the
    joint's main axis in the parent frame (prismatic); eval.py:58-77."""
    states = []
    for child, parent in enumerate(info["tree"]):
        if parent == -1:
            continue
        rot, trans = np.asarray(pose["rotation"], np.float64), np.asarray(pose["translation"], np.float64)
        if info["type"] == "revolute":
            states.append(float(rot_diff_degree(torch.as_tensor(pose["rotation"][child]), torch.as_tensor(pose["rotation"][parent]))))
        else:
            rel = rot[parent].T @ (trans[child] - trans[parent])
            states.append(float(rel.reshape(-1)[info["main_axis"][len(states)]]))
    return np.array(states)


def device_ious(data: dict, sym: bool, rigid: bool, device) -> np.ndarray:
    """`--eval_device`: the 'iou' entry of eval_instance_part_iou for every frame after the first of one result pickle, on the GPU
    in one call (pose_utils/bbox_utils.py eval_single_part_iou_device) -> (T-1, P) float64."""
    frames = range(1, len(data["pred"]["poses"]))
    stack = lambda poses: {k: torch.as_tensor(np.stack([np.asarray(poses[i][k], np.float32) for i in frames])).unsqueeze(1).to(device)
                           for k in ("rotation", "translation", "scale")}
    pred_corners = torch.as_tensor(np.stack([np.asarray(data["pred"]["corners"][i], np.float32) for i in frames])).unsqueeze(1).to(device)
    gt_corners = torch.as_tensor(np.asarray(data["gt"]["corners"], np.float32)).unsqueeze(0).to(device)
    res = eval_single_part_iou_device(gt_corners, pred_corners, stack(data["gt"]["poses"]), stack(data["pred"]["poses"]), nocs=rigid, sym=sym)
    return res["iou"][:, 0].double().cpu().numpy()


def eval_data(name: str, data: dict, obj_info: dict, device=None) -> dict:
    sym, rigid = obj_info["sym"], obj_info["num_parts"] == 1
    gt_corners = np.asarray(data["gt"]["corners"])
    errors = {}
    ious = device_ious(data, sym, rigid, device) if device is not None and len(data["pred"]["poses"]) > 1 else None
    for i in range(1, len(data["pred"]["poses"])):          # frame 0 is the initialisation
        gt = {k: torch.as_tensor(np.asarray(v)) for k, v in data["gt"]["poses"][i].items()}
        pred = {k: torch.as_tensor(np.asarray(v)) for k, v in data["pred"]["poses"][i].items()}
        _, per = eval_part_full(gt, pred, per_instance=True, yaxis_only=sym)
        row = {k: float(np.asarray(v)) for k, v in per.items()}
        if ious is not None:
            row.update({f"iou_{j}": float(v) for j, v in enumerate(ious[i - 1])})
        else:
            iou = eval_instance_part_iou(gt_corners, np.asarray(data["pred"]["corners"][i]), {k: v.numpy() for k, v in gt.items()},
                                         {k: v.numpy() for k, v in pred.items()}, nocs=rigid, sym=sym)
            row.update({f"iou_{j}": float(v) for j, v in enumerate(iou["iou"])})
        if not rigid:
            diff = np.abs(get_joint_state(obj_info, {k: v.numpy() for k, v in pred.items()})
                          - get_joint_state(obj_info, {k: v.numpy() for k, v in gt.items()}))
            row.update({f"theta_diff_{j}": float(v) for j, v in enumerate(diff)})
        errors[f"{name}_{i}"] = row
    return errors


def guard_table(name: str, data: dict) -> list:
    """The track guard's record of one result pickle (present when the run had track_cfg/guard): one line per part with the frames
    whose verdict was lost / recovered / too_few."""
    from .pose_utils.pose_fit import GUARD_VERDICTS
    frames = [(i, np.asarray(g["verdict"]).reshape(-1)) for i, g in enumerate(data["guard"]) if g is not None and "verdict" in g]
    lines = []
    for p in range(len(frames[0][1]) if frames else 0):
        cols = []
        for code in (2, 3, 1):
            hit = [str(i) for i, v in frames if int(v[p]) == code]
            cols.append(f"{GUARD_VERDICTS[code]} {len(hit)}" + (f" [{' '.join(hit)}]" if hit else ""))
        lines.append(f"{name} part {p}: " + "; ".join(cols) + f" (of {len(frames)} frames)")
    return lines


def guard_test_name(data: dict) -> str:
    """Which inlier test the run's guard used: the boolean a run with track_cfg/guard/yaxis_only carries in the slot of frame 0."""
    head = data["guard"][0] if data["guard"] else None
    return "axis-only" if head is not None and bool(np.all(head.get("yaxis_only", False))) else "full-rotation"


def st_fit_table(name: str, data: dict) -> list:
    """The robust scale / translation fit's record of one result pickle (present when the run had track_cfg/st_fit/ransac): one line
    per part with the frames whose fit was kept / replaced by the previous value, and over the frames kept the mean number of
    inliers -- as a fraction of the part's members where the pickle also carries the guard's record (its `count`: the frame record
    of the fit itself is two integers, inliers and valid)."""
    frames = [(i, np.asarray(r["valid"]).reshape(-1), np.asarray(r["inliers"]).reshape(-1)) for i, r in enumerate(data["st_fit"])
              if r is not None and "valid" in r]
    guard = data.get("guard")
    lines = []
    for p in range(len(frames[0][1]) if frames else 0):
        kept = [(i, int(n[p])) for i, v, n in frames if int(v[p]) != 0]
        held = [str(i) for i, v, _ in frames if int(v[p]) == 0]
        col = f"mean inliers {np.mean([n for _, n in kept]):.1f}" if kept else "mean inliers -"
        if kept and guard is not None and all(guard[i] is not None and "count" in guard[i] for i, _ in kept):
            frac = [n / max(int(np.asarray(guard[i]["count"]).reshape(-1)[p]), 1) for i, n in kept]
            col += f", mean inlier fraction {np.mean(frac):.3f}"
        lines.append(f"{name} part {p}: kept {len(kept)}; previous value {len(held)}" + (f" [{' '.join(held)}]" if held else "")
                     + f"; {col} (of {len(frames)} frames)")
    return lines


def rot_pool_table(name: str, data: dict) -> list:
    """The consensus rotation read-out's record of one result pickle (present when the run had track_cfg/rot_pool/consensus): one
    line per part with the frames, over the frames with members the mean and the minimum fraction of the part's votes that were
    inliers of the winning vote, and the frames without members."""
    frames = [(i, np.asarray(r["inliers"]).reshape(-1), np.asarray(r["count"]).reshape(-1)) for i, r in enumerate(data["rot_pool"])
              if r is not None and "count" in r]
    lines = []
    for p in range(len(frames[0][1]) if frames else 0):
        frac = [int(n[p]) / int(c[p]) for _, n, c in frames if int(c[p]) > 0]
        empty = [str(i) for i, _, c in frames if int(c[p]) == 0]
        col = f"inlier fraction mean {np.mean(frac):.3f} min {np.min(frac):.3f}" if frac else "inlier fraction -"
        lines.append(f"{name} part {p}: frames {len(frames)}; {col}; without members {len(empty)}" + (f" [{' '.join(empty)}]" if empty else ""))
    return lines


def motion_table(name: str, data: dict) -> list:
    """The motion model's record of one result pickle (present when the run had track_cfg/motion/predict): one line per part with the
    frames whose start pose was predicted (`used`: the NEXT frame started from an extrapolation) and the largest step the history
    saw, in degrees and in the translation's units."""
    frames = [(np.asarray(r["used"]).reshape(-1), np.asarray(r["angle"]).reshape(-1), np.asarray(r["shift"]).reshape(-1))
              for r in data["motion"] if r is not None and "used" in r]
    lines = []
    for p in range(len(frames[0][0]) if frames else 0):
        used = sum(1 for u, _, _ in frames if int(u[p]) != 0)
        lines.append(f"{name} part {p}: predicted {used} / {len(frames)} frames; largest step {max(float(a[p]) for _, a, _ in frames):.2f} deg, "
                     f"{max(float(s[p]) for _, _, s in frames):.4f}")
    return lines


def size_table(name: str, data: dict) -> list:
    """The held size's record of one result pickle (present when the run had track_cfg/size/hold): one line per part with the frames
    whose scale was held at the running mean, the frames accepted into the mean, the frames kept out of it (gated by max_ratio, or
    without a valid fit of their own) and the restarts (an accepted frame that left ONE frame in a mean that had some), the final
    mean -- replayed in float64 from the record, starting at frame 0's scale -- and the smallest and largest free scale, over the
    frames whose own fit was valid where the pickle also carries the robust fit's record, else over all frames."""
    frames = [(i, {k: np.asarray(r[k]).reshape(-1) for k in ("held", "accepted", "free", "n")}) for i, r in enumerate(data["size"])
              if r is not None and "held" in r]
    st = data.get("st_fit")
    lines = []
    for p in range(len(frames[0][1]["held"]) if frames else 0):
        mean, prev_n, restarts, free = float(np.asarray(data["pred"]["poses"][0]["scale"]).reshape(-1)[p]), None, 0, []
        for i, r in frames:
            n, f = int(r["n"][p]), float(r["free"][p])
            if int(r["accepted"][p]) != 0:
                restarts += int(n == 1 and prev_n is not None and prev_n >= 1)
                mean = f if n == 1 else mean + (f - mean) / n
            prev_n = n
            if st is None or st[i] is None or int(np.asarray(st[i]["valid"]).reshape(-1)[p]) != 0:
                free.append(f)
        held = sum(1 for _, r in frames if int(r["held"][p]) != 0)
        accepted = sum(1 for _, r in frames if int(r["accepted"][p]) != 0)
        span = f"free scale min {min(free):.5f} max {max(free):.5f}" if free else "free scale -"
        lines.append(f"{name} part {p}: held {held}; accepted {accepted}; gated or invalid {len(frames) - accepted}; restarted {restarts} "
                     f"(of {len(frames)} frames); final mean {mean:.5f} over {prev_n if prev_n is not None else 0} frames; {span}")
    return lines


def box_table(name: str, data: dict) -> list:
    """The held box's record of one result pickle (present when the run had track_cfg/box/hold): one line per part with the final
    half-extents, the first frame after which the box was established (all three extents > 0), the frames that stayed out of the
    histograms on the guard's verdict (members, but no growth of the held count) and, per axis, the range of the frames' own
    extents against the range of the held ones (over the frames with members / with an established box)."""
    frames = [(i, {"extent": np.asarray(r["extent"], np.float64).reshape(-1, 3), "frame": np.asarray(r["frame"], np.float64).reshape(-1, 3),
                   "added": np.asarray(r["added"]).reshape(-1), "total": np.asarray(r["total"]).reshape(-1)})
              for i, r in enumerate(data["box"]) if r is not None and "extent" in r]
    lines = []
    for p in range(len(frames[0][1]["added"]) if frames else 0):
        first, skipped, prev_total, own, held = None, 0, 0, [], []
        for i, r in frames:
            established = bool((r["extent"][p] > 0).all())
            if established and first is None:
                first = i
            if established:
                held.append(r["extent"][p])
            if int(r["added"][p]) > 0:
                own.append(r["frame"][p])
                skipped += int(int(r["total"][p]) == prev_total and prev_total < 2 ** 31 - 1)
            prev_total = int(r["total"][p])
        span = lambda rows, k: f"{min(x[k] for x in rows):.4f}-{max(x[k] for x in rows):.4f}" if rows else "-"
        final = " ".join(f"{v:.4f}" for v in frames[-1][1]["extent"][p])
        axes = "; ".join(f"{a} frame {span(own, k)} held {span(held, k)}" for k, a in enumerate("xyz"))
        lines.append(f"{name} part {p}: half-extents {final}; established at frame {'-' if first is None else first}; skipped on the guard's "
                     f"verdict {skipped} (of {len(frames)} frames); {prev_total} values held; {axes}")
    return lines


def otf_thin_table(name: str, data: dict) -> list:
    """The re-crop's on-device thinning record of one result pickle (present when the run had track_cfg/otf_thin/device): one line
    with the frames whose candidate list was thinned, of the frames re-cropped."""
    frames = [(i, int(np.asarray(r["thinned"]).reshape(-1)[0])) for i, r in enumerate(data["otf_thin"]) if r is not None and "thinned" in r]
    return [f"{name}: thinned {sum(1 for _, t in frames if t != 0)} / {len(frames)} frames"]


def depth_filter_table(name: str, data: dict) -> list:
    """The depth filter's record of one result pickle (present when the run had track_cfg/depth_filter): one line with the pixels
    the filter set to 0 in the trajectory's depth images -- their sum, mean and maximum over the frames that had a depth image."""
    counts = [int(np.asarray(r["removed"]).reshape(-1)[0]) for r in data["depth_filter"] if r is not None and "removed" in r]
    if not counts:
        return [f"{name}: removed 0 pixels in 0 frames"]
    return [f"{name}: removed {sum(counts)} pixels in {len(counts)} frames (mean {np.mean(counts):.1f}, max {max(counts)} per frame)"]


def image_fit_table(name: str, data: dict) -> list:
    """The first-pose image fit's record of one result pickle (present when the run had init_frame/image_fit): one line with the
    members the eroded mask held, those the fit used, the holes, the inliers of the fit and whether it was valid."""
    r = {k: int(np.asarray(v).reshape(-1)[0]) for k, v in data["image_fit"].items()}
    return [f"{name}: members {r['members']}; used {r['used']}; holes {r['holes']}; inliers {r['inliers']}; valid {'yes' if r['valid'] else 'no'}"]


def camera_table(name: str, data: dict) -> list:
    """The camera of one result pickle's trajectory (present when the run had a camera: the `camera` section or the frames' own): one
    line with fx, fy, cx, cy (and the skew when there is one) and the depth unit in metres per count."""
    K = np.asarray(data["camera"]["K"], np.float64).reshape(-1, 3, 3)[0]
    unit = float(np.asarray(data["camera"]["depth_unit"], np.float64).reshape(-1)[0])
    skew = f"; skew {K[0, 1]:g}" if K[0, 1] != 0 else ""
    return [f"{name}: fx {K[0, 0]:g}; fy {K[1, 1]:g}; cx {K[0, 2]:g}; cy {K[1, 2]:g}{skew}; depth unit {unit:g} m"]


# the options' records a result pickle may carry, in the order they are printed: (pickle key, its table, the heading -- {tests}: the
# inlier tests the runs' guards used)
RECORD_TABLES = (
    ("guard", guard_table, "track guard ({tests} inlier test), frames per trajectory and part:"),
    ("st_fit", st_fit_table, "robust scale / translation fit (track_cfg/st_fit), frames per trajectory and part:"),
    ("rot_pool", rot_pool_table, "consensus rotation read-out (track_cfg/rot_pool), per trajectory and part:"),
    ("motion", motion_table, "constant-velocity start pose (track_cfg/motion), per trajectory and part:"),
    ("size", size_table, "held size (track_cfg/size), frames per trajectory and part:"),
    ("box", box_table, "held box (track_cfg/box), per trajectory and part:"),
    ("otf_thin", otf_thin_table, "re-crop lists thinned on the device (track_cfg/otf_thin), frames per trajectory:"),
    ("depth_filter", depth_filter_table, "flying depth pixels removed at upload (track_cfg/depth_filter), per trajectory:"),
    ("image_fit", image_fit_table, "first pose fitted from frame 0's images (init_frame/image_fit), per trajectory:"),
    ("camera", camera_table, "camera (camera / the frames' own), per trajectory:"),
)


def write_csv(errors: dict, path: str) -> None:
    keys = list(next(iter(errors.values())).keys())
    with open(path, "w") as f:
        f.write("," + ",".join(keys) + "\n")
        for inst, row in errors.items():
            f.write(inst + "," + ",".join(str(row[k]) for k in keys) + "\n")


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", type=str, default="config_track.yml")
    ap.add_argument("--obj_config", type=str, default=None)
    ap.add_argument("--obj_category", type=str, default=None)
    ap.add_argument("--experiment_dir", type=str, default=None)
    ap.add_argument("--eval_device", action="store_true", default=False,
                    help="box IoUs on the GPU, all frames of a pickle in one call (opt-in; default the host numpy protocol)")
    args = ap.parse_args(argv)
    device = None
    if args.eval_device:
        if not torch.cuda.is_available():
            raise SystemExit("--eval_device needs a GPU (there is no fall-back: drop the flag for the host protocol)")
        device = torch.device("cuda", torch.cuda.current_device())
    del args.eval_device
    cfg = get_config(args, save=False)
    data_path = pjoin(cfg["experiment_dir"], "results", "data")
    errors, lines, guard_tests = {}, {key: [] for key, _, _ in RECORD_TABLES}, set()
    for raw in sorted(os.listdir(data_path)):
        with open(pjoin(data_path, raw), "rb") as f:
            data = pickle.load(f)
        errors.update(eval_data(raw.rsplit(".", 1)[0], data, cfg["obj_info"], device))
        for key, table, _ in RECORD_TABLES:
            if key in data:
                lines[key] += table(raw.rsplit(".", 1)[0], data)
        if "guard" in data:
            guard_tests.add(guard_test_name(data))
    if not errors:
        raise SystemExit(f"no result pickles under {data_path}")
    err_path = pjoin(cfg["experiment_dir"], "results", "err.pkl")
    with open(err_path, "wb") as f:
        pickle.dump(errors, f)
    write_csv(errors, err_path.replace("pkl", "csv"))
    avg = {k: float(np.mean([row[k] for row in errors.values()])) for k in next(iter(errors.values()))}
    for k, v in avg.items():
        print(f"{k}: {v}")
    for key, _, heading in RECORD_TABLES:
        if lines[key]:
            print(heading.format(tests=" / ".join(sorted(guard_tests))))
            for line in lines[key]:
                print("  " + line)
    return avg


if __name__ == "__main__":
    main()
