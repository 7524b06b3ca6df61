"""Pre-cropped trajectory files for the `track` harness.

The reference feeds `Trainer.test` a list over frames of frame dicts produced by its dataset classes
(network/data/dataset.py:71-91, 157-194; layout in SURVEY.md §8b "Loop API").  The datasets, the depth-crop
pipeline and cv2 are out of scope here (§8f row 1), so the harness reads the same frame dicts from one `.npz`
per trajectory -- the arrays a dataset item holds after cropping to N points:

    points       (T,3,N) f32   camera-frame points minus their mean
    points_mean  (T,3,1) f32
    labels       (T,N)   i64   part label per point (num_parts = background)
    nocs         (T,3,N) f32   ground-truth normalised coordinates
    rotation     (T,P,3,3) f32, translation (T,P,3,1) f32, scale (T,P) f32   ground-truth nocs2camera per part
    nocs_corners (P,2,3) f32
    paths        (T,) str      "…/<instance>/<track>/<frame>.<ext>" (drives the result file names, model.py:497-509)
    depth, mask  (T,H,W) uint16 mm / bool, optional: the frames' depth images and instance masks for `--nocs_otf True`
                               (the reference's meta['pre_fetched'], dataset.py:157-194)
    det_boxes (T,K,4) i32 [y1,x1,y2,x2], det_class (T,K) i32, det_count (T,) i32, det_masks (T,K,H,W) u8, optional (with depth / mask):
                               the frames' 2D detections for `--track_cfg/nocs2d_label True`, K slots of which the first det_count hold one
    coord        (H,W,3) uint8 optional (with depth / mask): FRAME 0's NOCS coordinate image, channel k = NOCS axis k, for
                               `--init_frame/image_fit True` (the first pose fitted from images alone)
    camera_K (3,3) f64, camera_depth_unit () f64, optional (with depth / mask): the trajectory's camera -- intrinsics and metres per
                               depth count (the `camera` option, track_options.py); a trajectory without them is seen through the
                               configuration's camera, or the NOCS REAL one
    ori_paths    (T,) str      optional: "…/<scene>/<frame>_depth.png" (meta['ori_path']): names the detector result file of a frame

`stack_trajectories` batches B trajectories of equal length into the (B, …) frame dicts `set_data` takes.  The images of one batch
share their size H x W: a batch with several image sizes is a ValueError.
"""
from __future__ import annotations

import numpy as np
import torch

_KEYS = ("points", "points_mean", "labels", "nocs", "rotation", "translation", "scale", "nocs_corners", "paths")
DET_KEYS = ("det_boxes", "det_class", "det_count", "det_masks")
_DET_DTYPES = {"det_boxes": np.int32, "det_class": np.int32, "det_count": np.int32, "det_masks": np.uint8}
CAMERA_KEYS = ("camera_K", "camera_depth_unit")


def _default_camera(default_camera) -> tuple:
    """(K (3,3), depth_unit) a trajectory without a camera of its own gets in a mixed batch: the configuration's ({'K', 'depth_unit'},
    track_options.camera_cfg) or the NOCS REAL camera, which is what such a trajectory was always seen through."""
    from .nocs_otf import CAMERA_PRESETS
    if default_camera is None:
        K, unit = CAMERA_PRESETS["nocs_real"]
        return np.asarray(K, np.float64), float(unit)
    return np.asarray(default_camera["K"], np.float64).reshape(3, 3), float(default_camera["depth_unit"])


def _one_image_size(shapes, what: str) -> None:
    sizes = sorted({tuple(int(x) for x in s[-2:]) for s in shapes})
    if len(sizes) > 1:
        raise ValueError(f"{what}: the images of one batch share their size H x W, got {sizes} (batch the trajectories by image size)")


def save_trajectory_npz(path: str, frames: list, b: int = 0) -> None:
    """Write trajectory `b` of a list of batched frame dicts (the structure above) to `path`."""
    P = len(frames[0]["meta"]["nocs2camera"])
    out = {
        "points": np.stack([f["points"][b].cpu().numpy() for f in frames]).astype(np.float32),
        "points_mean": np.stack([f["meta"]["points_mean"][b].cpu().numpy() for f in frames]).astype(np.float32),
        "labels": np.stack([f["labels"][b].cpu().numpy() for f in frames]).astype(np.int64),
        "nocs": np.stack([f["nocs"][b].cpu().numpy() for f in frames]).astype(np.float32),
        "rotation": np.stack([np.stack([f["meta"]["nocs2camera"][p]["rotation"][b].cpu().numpy() for p in range(P)]) for f in frames]),
        "translation": np.stack([np.stack([f["meta"]["nocs2camera"][p]["translation"][b].cpu().numpy() for p in range(P)]) for f in frames]),
        "scale": np.stack([np.stack([f["meta"]["nocs2camera"][p]["scale"][b].cpu().numpy() for p in range(P)]) for f in frames]),
        "nocs_corners": frames[0]["meta"]["nocs_corners"][b].cpu().numpy().astype(np.float32),
        "paths": np.array([f["meta"]["path"][b] for f in frames]),
    }
    if all("pre_fetched" in f["meta"] for f in frames):
        out["depth"] = np.stack([np.asarray(f["meta"]["pre_fetched"]["depth"][b]) for f in frames]).astype(np.uint16)
        out["mask"] = np.stack([np.asarray(f["meta"]["pre_fetched"]["mask"][b]) for f in frames]).astype(bool)
        if all(k in f["meta"]["pre_fetched"] for f in frames for k in DET_KEYS):
            for k in DET_KEYS:
                out[k] = np.stack([np.asarray(f["meta"]["pre_fetched"][k][b]) for f in frames]).astype(_DET_DTYPES[k])
        if "coord" in frames[0]["meta"]["pre_fetched"]:
            out["coord"] = np.asarray(frames[0]["meta"]["pre_fetched"]["coord"][b]).astype(np.uint8)
        if "camera" in frames[0]["meta"]["pre_fetched"]:
            cam = frames[0]["meta"]["pre_fetched"]["camera"]
            out["camera_K"] = np.asarray(cam["K"][b], np.float64).reshape(3, 3)
            out["camera_depth_unit"] = np.float64(np.asarray(cam["depth_unit"][b], np.float64).reshape(()))
    if all("ori_path" in f["meta"] for f in frames):
        out["ori_paths"] = np.array([f["meta"]["ori_path"][b] for f in frames])
    np.savez(path, **out)


def load_trajectory_npz(path: str) -> dict:
    with np.load(path, allow_pickle=False) as z:
        missing = [k for k in _KEYS if k not in z.files]
        if missing:
            raise ValueError(f"{path}: not a trajectory file, missing {missing}")
        traj = {k: z[k] for k in _KEYS}
        for k in ("depth", "mask", "coord", "ori_paths") + DET_KEYS + CAMERA_KEYS:
            if k in z.files:
                traj[k] = z[k]
    T = traj["points"].shape[0]
    if not all(traj[k].shape[0] == T for k in ("points_mean", "labels", "nocs", "rotation", "translation", "scale", "paths")):
        raise ValueError(f"{path}: inconsistent frame counts")
    if any(k in traj for k in CAMERA_KEYS):
        if not all(k in traj for k in CAMERA_KEYS) or "depth" not in traj:
            raise ValueError(f"{path}: a trajectory's camera is camera_K (3,3) AND camera_depth_unit, beside its depth images")
        from .nocs_otf import check_camera
        check_camera(traj["camera_K"], traj["camera_depth_unit"], prefix=f"{path}: camera_")
    return traj


def stack_trajectories(trajs: list, default_camera=None) -> list:
    """B trajectory dicts of equal length T -> list over T of batched frame dicts (CPU tensors).  When a trajectory carries its camera
    (camera_K, camera_depth_unit) every frame gets meta['pre_fetched']['camera'] = {'K' (B,3,3), 'depth_unit' (B,)}; in such a MIXED stack a
    trajectory without one gets `default_camera` ({'K', 'depth_unit'}: the configuration's) or the NOCS REAL camera."""
    T = trajs[0]["points"].shape[0]
    if any(t["points"].shape != trajs[0]["points"].shape for t in trajs):
        raise ValueError("trajectories of one batch must share the frame count and the number of points")
    P = trajs[0]["rotation"].shape[1]
    frames = []
    for i in range(T):
        def cat(key, dtype=torch.float32):
            return torch.from_numpy(np.stack([t[key][i] for t in trajs])).to(dtype)
        poses = [{"rotation": cat("rotation")[:, p].contiguous(), "translation": cat("translation")[:, p].contiguous(),
                  "scale": cat("scale")[:, p].contiguous()} for p in range(P)]
        meta = {"path": [str(t["paths"][i]) for t in trajs], "nocs2camera": poses, "points_mean": cat("points_mean"),
                "nocs_corners": torch.from_numpy(np.stack([t["nocs_corners"] for t in trajs])).float()}
        if all("depth" in t and "mask" in t for t in trajs):
            _one_image_size([t["depth"].shape for t in trajs], "stack_trajectories")
            meta["pre_fetched"] = {"depth": torch.from_numpy(np.stack([t["depth"][i].astype(np.int32) for t in trajs])),
                                   "mask": torch.from_numpy(np.stack([t["mask"][i] for t in trajs]))}
            if all(k in t for t in trajs for k in DET_KEYS):
                meta["pre_fetched"].update(pad_detections([{k: t[k][i] for k in DET_KEYS} for t in trajs]))
            if i == 0 and all("coord" in t for t in trajs):
                meta["pre_fetched"]["coord"] = torch.from_numpy(np.stack([np.asarray(t["coord"], np.uint8) for t in trajs]))
            if any("camera_K" in t for t in trajs):
                cams = [(np.asarray(t["camera_K"], np.float64), float(t["camera_depth_unit"])) if "camera_K" in t else _default_camera(default_camera)
                        for t in trajs]
                meta["pre_fetched"]["camera"] = {"K": torch.from_numpy(np.stack([c[0] for c in cams])),
                                                 "depth_unit": torch.tensor([c[1] for c in cams], dtype=torch.float64)}
        if all("ori_paths" in t for t in trajs):
            meta["ori_path"] = [str(t["ori_paths"][i]) for t in trajs]
        frames.append({"points": cat("points"), "labels": cat("labels", torch.int64), "nocs": cat("nocs"), "meta": meta})
    return frames


def concat_frame_batches(batches: list, default_camera=None) -> list:
    """[list over T of frame dicts with batch b_k] (equal T, N, P) -> one list over T with batch sum(b_k): the batch
    dimension of every tensor concatenated, path lists chained.  Used by the harness to build a batch out of
    independently generated / loaded trajectories, so that a trajectory's content does not depend on which rank or
    batch it lands in.  Cameras (meta['pre_fetched']['camera']) are carried; where only some batches have one the others' trajectories
    get `default_camera` or the NOCS REAL camera, as in stack_trajectories."""
    if len(batches) == 1:
        return batches[0]
    T = len(batches[0])
    if any(len(b) != T for b in batches):
        raise ValueError("trajectories of one batch must share the frame count")
    out = []
    for i in range(T):
        frames = [b[i] for b in batches]
        P = len(frames[0]["meta"]["nocs2camera"])
        meta = {"path": [p for f in frames for p in f["meta"]["path"]],
                "nocs2camera": [{k: torch.cat([f["meta"]["nocs2camera"][p][k] for f in frames]) for k in frames[0]["meta"]["nocs2camera"][p]}
                                for p in range(P)],
                "points_mean": torch.cat([f["meta"]["points_mean"] for f in frames]),
                "nocs_corners": torch.cat([f["meta"]["nocs_corners"] for f in frames])}
        if all("pre_fetched" in f["meta"] for f in frames):
            _one_image_size([tuple(torch.as_tensor(f["meta"]["pre_fetched"]["depth"]).shape) for f in frames], "concat_frame_batches")
            meta["pre_fetched"] = {k: torch.cat([torch.as_tensor(f["meta"]["pre_fetched"][k]) for f in frames]) for k in ("depth", "mask")}
            if any("camera" in f["meta"]["pre_fetched"] for f in frames):
                Ks, units = [], []
                for f in frames:
                    cam, b = f["meta"]["pre_fetched"].get("camera"), len(f["meta"]["path"])
                    K0, u0 = _default_camera(default_camera)
                    Ks.append(torch.as_tensor(cam["K"]).double().reshape(b, 3, 3) if cam is not None else torch.from_numpy(K0).expand(b, 3, 3))
                    units.append(torch.as_tensor(cam["depth_unit"]).double().reshape(b) if cam is not None else torch.full((b,), u0, dtype=torch.float64))
                meta["pre_fetched"]["camera"] = {"K": torch.cat(Ks), "depth_unit": torch.cat(units)}
            if all(k in f["meta"]["pre_fetched"] for f in frames for k in DET_KEYS):
                meta["pre_fetched"].update(pad_detections([{k: f["meta"]["pre_fetched"][k] for k in DET_KEYS} for f in frames], batched=True))
            if all("coord" in f["meta"]["pre_fetched"] for f in frames):
                meta["pre_fetched"]["coord"] = torch.cat([torch.as_tensor(f["meta"]["pre_fetched"]["coord"]) for f in frames])
        if all("ori_path" in f["meta"] for f in frames):
            meta["ori_path"] = [p for f in frames for p in f["meta"]["ori_path"]]
        out.append({"points": torch.cat([f["points"] for f in frames]), "labels": torch.cat([f["labels"] for f in frames]),
                    "nocs": torch.cat([f["nocs"] for f in frames]), "meta": meta})
    return out


def pad_detections(items: list, batched: bool = False, slots: int | None = None) -> dict:
    """Detections of one frame from several sources -> one batch: the K axis padded to the largest K (or `slots`) with empty slots
    (box 0, class -1, mask 0; det_count says how many are real).  items: dicts of det_boxes (K,4), det_class (K,), det_count (),
    det_masks (K,H,W) -- or, `batched`, of (b,K,4), (b,K), (b,), (b,K,H,W) -- arrays or tensors -> dict of CPU tensors (B, ...)."""
    arrs = [{k: np.asarray(it[k]) if not torch.is_tensor(it[k]) else it[k].cpu().numpy() for k in DET_KEYS} for it in items]
    if not batched:
        arrs = [{k: a[k][None] for k in DET_KEYS} for a in arrs]
    K = max([a["det_boxes"].shape[1] for a in arrs] + [int(slots or 0)])
    H, W = arrs[0]["det_masks"].shape[-2:]
    out = {"det_boxes": [], "det_class": [], "det_count": [], "det_masks": []}
    for a in arrs:
        b, k = a["det_boxes"].shape[:2]
        boxes = np.zeros((b, K, 4), np.int32)
        cls = np.full((b, K), -1, np.int32)
        masks = np.zeros((b, K, H, W), np.uint8)
        boxes[:, :k], cls[:, :k], masks[:, :k] = a["det_boxes"], a["det_class"], a["det_masks"]
        out["det_boxes"].append(boxes)
        out["det_class"].append(cls)
        out["det_masks"].append(masks)
        out["det_count"].append(np.asarray(a["det_count"], np.int32).reshape(b))
    return {k: torch.from_numpy(np.concatenate(v)) for k, v in out.items()}


def load_nocs2d_result(nocs2d_path: str, scene: str, frame: str, slots: int | None = None) -> dict:
    """One frame's detections from the reference's detector result file `results_test_{scene}_{frame}.pkl` under `nocs2d_path`
    (nocs_data_process.py:206-214; keys pred_class_ids (n,), pred_bboxes (n,4) [y1,x1,y2,x2], pred_masks (H,W,n)) -> det_boxes (K,4) int32,
    det_class (K,) int32, det_count () int32 = n, det_masks (K,H,W) uint8 with K = max(n, slots, 1): the slots past n are empty."""
    import pickle
    from os.path import join as pjoin
    with open(pjoin(nocs2d_path, f"results_test_{scene}_{frame}.pkl"), "rb") as f:
        res = pickle.load(f)
    cls = np.asarray(res["pred_class_ids"]).reshape(-1)
    n = cls.shape[0]
    masks = np.asarray(res["pred_masks"])
    if masks.ndim != 3 or masks.shape[2] != n or np.asarray(res["pred_bboxes"]).reshape(-1, 4).shape[0] != n:
        raise ValueError(f"{nocs2d_path}: results_test_{scene}_{frame}.pkl: {n} class ids, boxes {np.asarray(res['pred_bboxes']).shape}, masks {masks.shape}")
    K = max(n, int(slots or 0), 1)
    out = {"det_boxes": np.zeros((K, 4), np.int32), "det_class": np.full((K,), -1, np.int32), "det_count": np.int32(n),
           "det_masks": np.zeros((K,) + masks.shape[:2], np.uint8)}
    out["det_boxes"][:n] = np.asarray(res["pred_bboxes"]).reshape(n, 4)
    out["det_class"][:n] = cls
    out["det_masks"][:n] = np.moveaxis(masks != 0, 2, 0)
    return out


def attach_nocs2d_detections(frames: list, nocs2d_path: str, slots: int | None = None) -> list:
    """Batched frame dicts with meta['ori_path'] (".../<scene>/<frame>_depth.png", the reference's depth path: scene = its directory,
    frame = the first four characters of its name) and meta['pre_fetched'] -> the same frames carrying their detections from
    `nocs2d_path` (load_nocs2d_result per trajectory and frame, padded to one K per frame)."""
    for f in frames:
        if "ori_path" not in f["meta"] or "pre_fetched" not in f["meta"]:
            raise ValueError("detections are attached by the frames' depth paths (meta['ori_path']) to their depth / mask (meta['pre_fetched'])")
        items = []
        for path in f["meta"]["ori_path"]:
            scene, name = str(path).split("/")[-2:]
            items.append(load_nocs2d_result(nocs2d_path, scene, name[:4], slots))
        f["meta"]["pre_fetched"].update(pad_detections(items, slots=slots))
    return frames
