"""The tracking loop: `EvalTrackModel` (and its `BaseModel`) on the MI355X path.

Mirrors the contract of the reference's network/models/model.py: `BaseModel` (l.27-104) and
`EvalTrackModel` (l.311-600): `set_data(data)`, `test(save, no_eval, epoch)`, attributes
`pred_dict = {'poses': [pose]*T, 'npcs_pred': [None, {...}]*}` and `loss_dict`.
`data` is a list over frames of dicts
  {'points' (B,3,N), 'labels' (B,N), 'nocs' (B,3,N),
   'meta': {'path': [str]*B, 'nocs2camera': [{'rotation' (B,3,3), 'translation' (B,3,1), 'scale' (B,)}]*P,
            'points_mean' (B,3,1), 'nocs_corners' (B,P,2,3)}}.
Frame i consumes the pose predicted for frame i-1 (strictly sequential, model.py:408-478);
trajectories of one batch are independent, which is what shards over GPUs (parallel.py).

The on-the-fly depth crop of `nocs_otf` (model.py:425-452) runs on the device from pre-fetched depth / mask tensors
(captra_amd/nocs_otf.py; reading the images from disk is the data loader's); compute_loss carries the reference's
segmentation, NOCS and box-IoU figures (loss.py, bbox_utils.py).
"""
from __future__ import annotations

import contextlib
import logging
import pickle
from copy import deepcopy
from os.path import join as pjoin

import os

import numpy as np
import torch
import torch.nn as nn

from . import fused
from . import graph as G
from . import track_options as O
from .networks import CoordNet, PartCanonNet, _canonicalize
from .nocs_otf import DET_KEYS
from .pose_utils.part_dof_utils import add_noise_to_part_dof, consume_noise_draws, eval_part_full, part_model_batch_to_part
from .utils import Timer, add_dict, cvt_torch, divide_dict, ensure_dirs, get_ith_from_batch


def write_result_pickles(experiment_dir: str, records) -> None:
    """records: [(file name, per-trajectory result dict)] -> <experiment_dir>/results/data/<instance>_<track>.pkl
    (reference model.py:503-509)."""
    save_path = pjoin(experiment_dir, "results", "data")
    ensure_dirs([save_path])
    for name, rec in records:
        with open(pjoin(save_path, name), "wb") as f:
            pickle.dump(rec, f)


class BaseModel(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.num_parts = int(cfg["num_parts"])
        self.num_joints = int(cfg["num_joints"])
        self.device = cfg["device"]
        self.network_type = cfg["network"]["type"]
        raw = cfg["pose_perturb"]
        self.pose_perturb_cfg = {"type": raw["type"], "scale": raw["s"], "translation": raw["t"],
                                 "rotation": float(np.deg2rad(raw["r"]))}
        self.sym = cfg["obj_sym"]
        self.cfg = cfg
        self.feed_dict = {}
        self.pred_dict = {}
        self.loss_dict = {}
        self.per_diff_dict = {}

    def record_per_diff(self, data, per_diff):
        for i, path in enumerate(data["meta"]["path"]):
            instance, track_num, frame_i = path.split(".")[-2].split("/")[-3:]
            self.per_diff_dict.setdefault(f"{instance}_{track_num}_{frame_i}", {}).update(get_ith_from_batch(per_diff, i))


OTF_FIRST_BOUND = 5                 # the first frame's stride bound, in units of N (5 N = the longest list the fast path takes)
OTF_DEFER = os.environ.get("CAPTRA_OTF_DEFER", "1") != "0"     # nocs_otf: no round trip for the crops' member counts either (A/B: 0 = the synchronous stage)


class _OtfCheck:
    """The deferred verdict of one frame's sync-free re-crop: the device word [rare-path instance met, longest candidate list]
    (captra_amd/nocs_otf.py) on its way to pinned host memory behind the crop launch.  `read()` -- called when the NEXT frame is
    about to be enqueued -- waits for that copy (work enqueued a frame ago: the host's only wait, and the GPU never waits for the
    host) and returns (rare, longest)."""
    _pinned: list = []

    def __init__(self, info):
        self.host = _OtfCheck._pinned.pop() if _OtfCheck._pinned else torch.empty(4, dtype=torch.int32).pin_memory()
        self.host.copy_(info, non_blocking=True)
        self.event = torch.cuda.Event()
        self.event.record()

    def read(self):
        self.event.synchronize()
        rare, longest = int(self.host[0]), int(self.host[1])
        _OtfCheck._pinned.append(self.host)
        return bool(rare), longest


def _otf_bound(longest: int, n: int) -> int:
    """The sampler's padded stride for the next frame: the last frame's longest candidate list + 3 %, in steps of 1024, within
    [N, 5 N] (a list that outgrows it is a rare-path instance: the frame runs again on the synchronous stage).  Tight on purpose: the
    pruned sampler keeps a cloud's buckets in registers up to 16384 points and spills slots to LDS beyond (fps_pruned.hip), and a
    tracked object's crop changes by a few points per frame."""
    return int(min(5 * n, max(n, -(-(longest + longest // 32) // 1024) * 1024)))


OTF_POSE_ON_DEVICE = os.environ.get("CAPTRA_OTF_POSE_ON_DEVICE", "1") != "0"   # nocs_otf: the crop box from the device-resident pose (A/B: 0 = via the host)
_OTF_LANE_STREAMS: dict = {}      # device index -> the two lane streams of EvalTrackModel._otf_lane_frames


def _frame_names(frame):
    return [p.split(".")[-2].split("/")[-1] for p in frame["meta"]["path"]]


class EvalTrackModel(BaseModel):
    def __init__(self, cfg):
        super().__init__(cfg)
        self.net = PartCanonNet(cfg)
        self.npcs_net = CoordNet(cfg)
        self.tree = cfg["obj_tree"]
        self.root = [p for p in range(len(self.tree)) if self.tree[p] == -1][0]
        self.gt_init = cfg["init_frame"]["gt"]
        # the opt-in features, each parsed once (track_options.py says what each one is); None = off: no launch, no tensor, no pickle entry
        self.fit_init = bool(cfg["init_frame"].get("fit", False))          # the first pose fitted to frame 0's NOCS map
        self.fit_init_cfg = O.init_fit_cfg(cfg)
        self.fit_init_yaxis = O.yaxis_only(cfg, cfg["init_frame"], "init_frame/yaxis_only")
        self.image_fit = O.image_fit_cfg(cfg)                              # the first pose fitted to frame 0's images
        self._fit_fallback_logged = False
        self.guard = O.guard_cfg(cfg)                                      # every step's pose checked, a lost part re-fitted
        self._warn_full_rotation_test(cfg)
        self.st_fit = self.net.st_fit = O.st_fit_cfg(cfg)                  # every step's scale / translation by RANSAC
        self.rot_pool = self.net.rot_pool = O.rot_pool_cfg(cfg)            # every step's rotation from the votes' consensus
        self.motion = O.motion_cfg(cfg)                                    # every step starts from a constant-velocity prediction
        self.size = self.net.size = O.size_cfg(cfg)                        # every step holds the part's running scale
        self.box = O.box_cfg(cfg)                                          # every step holds the part's box (NOCS extents)
        self.nocs_otf = bool(cfg.get("nocs_otf", False))
        self.otf_thin = O.otf_thin_cfg(cfg)                                # the re-crop's over-long lists thinned on the device
        self._otf_thin_rec = {}             # frame -> {first trajectory of a slice: its thinned flags (b,) int32 on the device}
        self.depth_filter = O.depth_filter_cfg(cfg)                        # flying pixels out of every uploaded depth image
        # the camera model: the configuration's camera, and per batch (set_data) the trajectories' cameras as PERSISTENT device tensors
        # -- `camera` = (table (C,19) float64, cam_of (B,) int32), what the *_cam entry points read in every frame -- and on the host
        # for the pickle; None = no camera anywhere: the plain entry points, no tensor
        self.camera_cfg = O.camera_cfg(cfg)
        self.camera = None
        self._camera_host = None
        self.radius = cfg["data_radius"]
        self.det_category = cfg["obj_category"]          # nocs2d_label: the class id the frame's detections are matched against
        self._det_missing_logged = False
        self.track_cfg = cfg["track_cfg"]
        self.npcs_feed_dict = []
        self.timer = Timer(True)
        self.time_dict = {"npcs_net": 0.0, "rot_all": 0.0}
        # single-part objects: RotationNet canonicalises with the very pose CoordNet used, so both nets see
        # the same cloud and FPS / ball query / 3-NN run once per frame instead of twice
        self.share_geometry = True
        self.overlap_geometry = os.environ.get("CAPTRA_OVERLAP_GEOM", "1") != "0"   # the shared geometry's two levels side by side
        self.overlap_nets = True     # CoordinateNet and RotationNet side by side on two streams (one part: they share the cloud)
        # STREAMED level-1 sampling (backbones.precompute_geometry_streamed): the 4096 -> 512 sampler as this many launches on a
        # stream of its own, the networks' first level walking the centres as they are picked; 0 / 1 = the sampler, then the
        # networks.  Same picks, same neighbour lists, same bits.
        self.sampler_chunks = int(cfg.get("sampler_chunks", os.environ.get("CAPTRA_SAMPLER_CHUNKS", "0")))
        # bf16 mode, one part: the first level of BOTH networks inside the sampler's launch (csrc/sa_bf16.hip level-1 stream kernel:
        # sampler workgroups publish their picks, the other workgroups run ball query + shared MLPs of the published centres).
        # Same picks, lists and features, bit for bit (tests/test_l1_stream_gpu.py); cfg['l1_stream'] = False / CAPTRA_L1_STREAM=0: off
        self.l1_stream = bool(cfg.get("l1_stream", True))
        # replay one captured hipGraph per frame instead of launching the ~140 kernels of a step one by one
        # (captra_amd/graph.py); opt-in: `--hipgraph` of captra_amd.track / cfg['hipgraph'].  Same kernels, same bits.
        self.use_graph = bool(cfg.get("hipgraph", False))
        # Box IoUs and predicted NOCS corners of the evaluation on the GPU (captra_amd/csrc/box_iou.hip) instead of the host numpy
        # protocol; opt-in: `--eval_device` of captra_amd.track / cfg['eval_device'].  IoUs agree within the grid's resolution
        # (DESIGN.md), corners bit for bit.
        self.eval_device = bool(cfg.get("eval_device", False))
        # arithmetic of the shared MLPs for THIS model (None = whatever the calling thread has set, default exact fp32);
        # "bf16" = BASELINE.json configs[2].  Entered around every step (fused.use_mlp_dtype): no process-wide switch.
        self.mlp_dtype = cfg.get("mlp_dtype")
        # multi-GPU harness hooks (captra_amd/track.py): `frame_hook(i, pose)` is called with every frame's pose (B,P,...)
        # as soon as it is enqueued -- the per-frame all-gather of pose records starts there and runs under the next
        # frame's kernels; `result_sink(list of (file name, per-trajectory result dict))` receives what `_save` would
        # write (rank 0 writes the pickles of every rank's trajectories).  Both None = the single-process behaviour.
        self.frame_hook = None
        self.result_sink = None
        # nocs_otf at batch >= 32 as two lanes half a frame apart (_otf_lane_frames): bit-identical results, 9.5 -> 7.9 ms per
        # 32-trajectory step (3370 -> 4060 frames/s).  On by default (cfg['otf_lanes'] = False turns it off): with the lane
        # streams created once per process the first eight model objects of a process all get the fast placement; what a
        # later one may get (both lanes on one hardware queue, ~13 ms) is in DESIGN.md section 5
        self.otf_lanes = bool(cfg.get("otf_lanes", True))
        self._graph = None
        self._graph_key = None

    def _warn_full_rotation_test(self, cfg):
        """Once per model object: a symmetric category judged by the full-rotation test."""
        uses = [name for name, on, yaxis in (("track_cfg/guard", self.guard is not None, self.guard is not None and self.guard.get("yaxis_only", False)),
                                             ("init_frame/fit", self.fit_init or self.image_fit is not None, self.fit_init_yaxis)) if on and not yaxis]
        if cfg["obj_sym"] and uses:
            logging.getLogger(__name__).warning(
                "%s on a symmetric category (%s) with the full-rotation inlier test in use: the tracked in-plane angle carries no "
                "information there; %s selects the axis-only test", " and ".join(uses), cfg["obj_category"],
                " / ".join(u.replace("/fit", "") + "/yaxis_only: True" for u in uses))

    # ---- host -> device ------------------------------------------------------------------------
    def _gt_part(self, frame):
        return part_model_batch_to_part(cvt_torch(frame["meta"]["nocs2camera"], self.device), self.num_parts, self.device)

    def _convert_pose_frame(self, frame, first):
        out = {"meta": frame["meta"], "gt_part": self._gt_part(frame)}
        if first:
            for key in ("points", "nocs"):
                if key in frame:
                    out[key] = frame[key].float().to(self.device)
        else:
            out["points"] = frame["points"].float().to(self.device)
            out["points_mean"] = frame["meta"]["points_mean"].float().to(self.device)
            if "nocs" in frame:
                out["npcs"] = frame["nocs"].float().to(self.device)
        if "labels" in frame:
            out["labels"] = frame["labels"].long().to(self.device)
        pre = frame["meta"].get("pre_fetched")
        if pre is not None:      # nocs_otf: the frame's depth image and instance mask live on the device
            out["pre_fetched"] = {"depth": torch.as_tensor(pre["depth"]).to(self.device).int(),
                                  "mask": torch.as_tensor(pre["mask"]).to(self.device).bool()}
            if self.depth_filter is not None:
                # flying pixels out of the uploaded image, all trajectories in one launch; the counts stay on the device
                from .nocs_otf import depth_support_filter
                out["pre_fetched"]["depth"], out["depth_filter_removed"] = depth_support_filter(out["pre_fetched"]["depth"].contiguous(),
                                                                                                **self.depth_filter)
            if first and self.image_fit is not None and "coord" in pre:
                out["pre_fetched"]["coord"] = torch.as_tensor(pre["coord"]).to(self.device).to(torch.uint8).contiguous()
            if self.track_cfg["nocs2d_label"] and all(k in pre for k in DET_KEYS):
                # the frame's 2D detections (boxes, classes, count, masks): the re-crop selects among them on the device
                out["pre_fetched"].update({k: torch.as_tensor(pre[k]).to(self.device).to(torch.uint8 if k == "det_masks" else torch.int32).contiguous()
                                           for k in DET_KEYS})
            # the re-crop derives ground-truth NOCS from the root part's ground-truth pose: keep it on the host (float64,
            # the values of the float32 device copy), so that the loop does not fetch it back from the device every frame
            root = frame["meta"]["nocs2camera"][self.root]
            out["gt_root_host"] = {k: np.asarray(torch.as_tensor(root[k]).float().double().cpu().numpy()) for k in ("rotation", "translation", "scale")}
            out["gt_root_dev"] = {k: torch.from_numpy(v).to(self.device) for k, v in out["gt_root_host"].items()}   # (and on the device: no upload per frame)
        return out

    def _convert_npcs_frame(self, frame):
        out = {"meta": frame["meta"], "points_mean": frame["meta"]["points_mean"].float().to(self.device)}
        for key in ("points", "nocs"):
            if key in frame:
                out[key] = frame[key].float().to(self.device)
        if "labels" in frame:
            out["labels"] = frame["labels"].long().to(self.device)
        return out

    def _set_cameras(self, data):
        """The batch's cameras (track_options.trajectory_cameras: frame 0's own, then the configuration's, then none) onto the device,
        once; a later frame whose camera differs from frame 0's is an error -- a camera belongs to a trajectory."""
        self.camera = self._camera_host = None
        pres = [f["meta"].get("pre_fetched") for f in data]
        if not pres or pres[0] is None or not (self.nocs_otf or self.image_fit is not None):
            return
        depth = pres[0]["depth"]
        if isinstance(depth, (list, tuple)):
            sizes = sorted({tuple(np.shape(d)[-2:]) for d in depth})
            if len(sizes) > 1:
                raise ValueError(f"the images of one batch share their size H x W; this batch has {sizes} (several image sizes in one batch are "
                                 "outside the camera model: batch the trajectories by image size)")
        B = len(depth)
        cams = O.trajectory_cameras(pres[0].get("camera"), self.camera_cfg, B)
        for i, pre in enumerate(pres[1:], 1):
            if pre is None or pre.get("camera") is None:
                continue                    # (a later frame need not repeat it)
            # (compared by bytes, not parsed again: a camera that equals frame 0's is as valid as frame 0's)
            same = pres[0].get("camera") is not None and all(
                pre["camera"].get(k) is pres[0]["camera"][k] or (pre["camera"].get(k) is not None and
                    np.asarray(torch.as_tensor(pre["camera"][k]).cpu().numpy(), np.float64).tobytes() == cams[k].tobytes()) for k in ("K", "depth_unit"))
            if not same:
                raise ValueError(f"frame {i}'s camera (meta['pre_fetched']['camera']) differs from frame 0's: a camera belongs to a trajectory "
                                 "and is constant over its frames")
        if cams is None:
            return
        from .nocs_otf import camera_table
        self.camera = camera_table(cams["K"], cams["depth_unit"], self.device)
        self._camera_host = cams

    def set_data(self, data):
        self._set_cameras(data)
        self.feed_dict = [self._convert_pose_frame(f, i == 0) for i, f in enumerate(data)]
        self.npcs_feed_dict = [self._convert_npcs_frame(f) for f in data]

    # ---- the loop ------------------------------------------------------------------------------
    def _initial_pose(self):
        part = self._annotated_initial_pose()
        self._image_fit_rec = None
        if self.image_fit is not None:
            return self._image_fitted_initial_pose(part)
        return self._fitted_initial_pose(part) if self.fit_init else part

    def _annotated_initial_pose(self):
        gt_part = self.feed_dict[0]["gt_part"]
        if self.gt_init:
            return gt_part
        part = add_noise_to_part_dof(gt_part, self.pose_perturb_cfg)
        if "crop_pose" in self.feed_dict[0]["meta"]:
            crop = part_model_batch_to_part(cvt_torch(self.feed_dict[0]["meta"]["crop_pose"], self.device),
                                            self.num_parts, self.device)
            part["translation"], part["scale"] = crop["translation"], crop["scale"]
        return part

    def _fitted_initial_pose(self, fallback):
        """init_frame/fit: all B x P first poses from frame 0's NOCS map (B,3,N), labels (B,N) and points (B,3,N) + points_mean in
        one launch; a part whose fit is invalid (fewer than three members or inliers) keeps `fallback`."""
        from .pose_utils.pose_fit import part_fit_ransac_cn
        first = self.feed_dict[0]
        missing = [k for k in ("nocs", "labels", "points") if k not in first]
        if missing:
            raise KeyError(f"init_frame/fit needs frame 0's {missing} (NOCS map, instance labels, points)")
        nocs = first["nocs"].float()
        B, P, N = nocs.shape[0], self.num_parts, nocs.shape[-1]
        src = (nocs if nocs.dim() == 4 else nocs.unsqueeze(1).expand(B, P, 3, N)).contiguous()
        mean = first["meta"]["points_mean"].float().to(self.device)
        rot, scale, trans, valid, _ = part_fit_ransac_cn(first["labels"].int().contiguous(), src, first["points"].float().contiguous(),
                                                         num_hyps=self.fit_init_cfg["num_hyps"], inlier_th=self.fit_init_cfg["inlier_th"],
                                                         seed=self.fit_init_cfg["seed"], target_mean=mean, yaxis_only=self.fit_init_yaxis)
        return self._valid_fits("init_frame/fit", rot, scale, trans, valid, fallback)

    def _valid_fits(self, option, rot, scale, trans, valid, fallback):
        """The first poses of `option`'s fit, `fallback` where a fit is not valid (said once per model object)."""
        if not self._fit_fallback_logged and not bool(valid.all()):
            self._fit_fallback_logged = True
            logging.getLogger(__name__).warning("%s: %d of %d first-pose fits are invalid; those parts start from the "
                                                "annotated pose", option, int((~valid).sum()), valid.numel())
        return {"rotation": torch.where(valid[..., None, None], rot, fallback["rotation"]),
                "scale": torch.where(valid, scale, fallback["scale"]),
                "translation": torch.where(valid[..., None, None], trans, fallback["translation"])}

    def _image_fitted_initial_pose(self, fallback):
        """init_frame/image_fit: all B first poses from frame 0's depth image, mask and coordinate image (the depth filter, when
        configured, has filtered the image in set_data) in two launches -- the correspondences (captra_image_members), the RANSAC
        fit -- with nothing visiting the host; a fit that is not valid keeps `fallback`.  The record, (B,) int32 each on the device:
        members, used, holes (the kernel's counts), inliers and valid (the fit's)."""
        from .nocs_otf import image_members
        from .pose_utils.pose_fit import part_fit_ransac_cn
        pre = self.feed_dict[0].get("pre_fetched") or {}
        missing = [k for k in ("depth", "mask", "coord") if k not in pre]
        if missing:
            raise KeyError(f"init_frame/image_fit needs frame 0's {missing} (meta['pre_fetched']: depth image, instance mask, NOCS "
                           "coordinate image)")
        cfg = self.image_fit
        mem = image_members(pre["depth"].contiguous(), pre["mask"].contiguous(), pre["coord"], cap=cfg["cap"], border=cfg["border"],
                            negate_z=cfg["negate_z"], cameras=self.camera)
        rot, scale, trans, valid, info = part_fit_ransac_cn(mem["labels"], mem["src"], mem["tgt"], num_hyps=self.fit_init_cfg["num_hyps"],
                                                            inlier_th=self.fit_init_cfg["inlier_th"], seed=self.fit_init_cfg["seed"],
                                                            yaxis_only=self.fit_init_yaxis)
        counts = mem["counts"]
        self._image_fit_rec = {"members": counts[:, 0].contiguous(), "used": counts[:, 1].contiguous(), "holes": counts[:, 2].contiguous(),
                               "inliers": info["num_inliers"][:, 0].contiguous(), "valid": valid[:, 0].int()}
        return self._valid_fits("init_frame/image_fit", rot, scale, trans, valid, fallback)

    @contextlib.contextmanager
    def _step_context(self, points, allow_split_k=True):
        """What every launch of a step over the clouds `points` (B,3,N) runs under: this model's MLP arithmetic and the split-k
        limit that goes with B.  allow_split_k=False: a lane of a larger batch, which must compute what the whole batch computes
        at any size, so it never takes the few-trajectory form."""
        with fused.use_mlp_dtype(self.mlp_dtype):
            few = fused.split_k_rule(len(points), allow_few=allow_split_k) if not self.training and points.is_cuda else 0
            with fused.split_k(few):
                yield

    def track_step(self, input, npcs_input, last_pose, allow_split_k=True):
        """One frame for all B trajectories: CoordNet -> labels -> RotationNet -> pose fit [-> guard] [-> motion model].  input['b0']: the index
        of the first trajectory within the whole batch when `input` is a lane of one (the guard's draws; default 0).
        track_cfg/motion: `last_pose` carries the prediction the step starts from (a dict without one is a track's start) and the
        returned dict the next one; the four phases take the dict as it travels and read their start pose out of it."""
        last_pose = O.entering(last_pose, self)      # (track_cfg/size: likewise the size state; a dict without one is a track's start)
        with self._step_context(input["points"], allow_split_k):
            self._step_begin(input, npcs_input, last_pose)
            join = self._fork_rotation_net(input, npcs_input, last_pose) if self._overlap_nets(input) else None
            if join is None and "_cloud" not in npcs_input and self._l1_stream_on(npcs_input):
                # networks one after the other (no fork): the shared prefix with the level-1 stream kernel all the same --
                # CoordinateNet takes it from `_cloud`, RotationNet from CoordinateNet's
                self._step_prep(input, npcs_input, last_pose)
            npcs_pred = self._step_coord(npcs_input)
            if join is not None:
                join()
            return npcs_pred, self._step_post(input, npcs_input, npcs_pred, last_pose)

    # ---- the step in four phases (what `track_step` composes; captra_amd.graph.TrackStepGraph(split=True) captures each as a
    # hipGraph of its own and replays [prep] -> [rot || coord] -> [post] on two EXPLICIT streams) ---------------------------
    def _step_begin(self, input, npcs_input, last_pose):
        last_pose = O.start_pose(last_pose)
        # (a view when it is contiguous -- one part: the clones are three copy kernels per step and nothing writes into them)
        npcs_input["canon_pose"] = {k: (v if v.is_contiguous() else v.clone()) for k, v in
                                    ((k, last_pose[k][:, self.root]) for k in ("rotation", "translation", "scale"))}
        npcs_input["init_part"] = last_pose
        # `_cloud` = (canonicalised cloud (B,3,N), the same (B,N,3), its geometry): the step's one hand-over of the shared prefix
        npcs_input.pop("_cloud", None)
        input.pop("_raw", None)

    def _step_prep(self, input, npcs_input, last_pose, level1_only=False, side=None) -> bool:
        """The part both networks wait for: CoordinateNet's canonicalised cloud and its geometry (sampling, neighbour lists,
        interpolation weights).  False when the cloud does not fit the one-launch sampler (no side-by-side schedule then)."""
        coord_bb = self.npcs_net.backbone
        # bf16 mode, one part: both networks' first level inside the sampler's launch (the level-1 stream kernel)
        stream = self._l1_stream_on(npcs_input)
        cam = _canonicalize(npcs_input["points"], npcs_input["points_mean"], npcs_input["canon_pose"], want_planes=stream)
        stream_level1 = None
        if stream:
            # RotationNet's backbone sees the bare coordinates, CoordinateNet's the coordinates as features too (use_xyz_feat).
            # CAPTRA_L1_NETS=rot (A/B): RotationNet's level only, CoordinateNet's three scales as launches of its own branch -- measured
            # equal at 32 trajectories (1.27 ms per step either way: the step is bound by the chip's work, not by the sampler's latency)
            nets = [(self.net.regress_net.encoder, None)]
            if os.environ.get("CAPTRA_L1_NETS", "both") == "both":
                nets.append((coord_bb, cam[0]))
            stream_level1 = (cam[0], cam[2], nets)
        geom = coord_bb.precompute_geometry(cam[1], level1_only=level1_only, side=side, stream_level1=stream_level1)
        if geom is None:
            return False
        npcs_input["_cloud"] = (cam[0], cam[1], geom)
        scratch = geom.stream_scratch
        if scratch is not None:
            # STICKY give-up word: the scratch is a fresh (eager) or re-zeroed (replayed) buffer every step, so its flag says
            # something about ONE launch; this one-word OR -- a launch of the step like any other, captured and replayed with it --
            # keeps every step's verdict until check_l1_stream() reads it (before results are written, and by the bench)
            self._l1_scratch = scratch
            sticky = getattr(self, "_l1_sticky", None)
            if (sticky is None or sticky.device != scratch.device) and not torch.cuda.is_current_stream_capturing():
                # (never created inside a capture: its zero fill would be replayed with the step; the loops run a step eagerly first)
                sticky = self._l1_sticky = torch.zeros(1, dtype=torch.int32, device=scratch.device)
            if sticky is not None and sticky.device == scratch.device:
                sticky.bitwise_or_(scratch.view(torch.int32)[-15:-14])
        return True

    def _l1_stream_on(self, npcs_input) -> bool:
        """bf16 mode, one part: both networks' first level inside the sampler's launch (the level-1 stream kernel)."""
        pts = npcs_input["points"]
        return (self.l1_stream and self.num_parts == 1 and self.share_geometry and fused.USE_L1_STREAM and fused.mlp_dtype() == "bf16"
                and not self.training and pts.is_cuda and pts.shape[2] <= 4096 and pts.shape[0] <= fused.L1_STREAM_MAX_CLOUDS
                and not (self.track_cfg["gt_label"] or self.track_cfg["nocs2d_label"]))

    def check_l1_stream(self) -> None:
        """Raises when a consumer of ANY level-1 stream launch since the last check gave up waiting for its sampler (bounded spins;
        synchronises): the sticky word every step ORs its flag into, then the last launch's own flag."""
        sticky = getattr(self, "_l1_sticky", None)
        scratch = getattr(self, "_l1_scratch", None)
        bad = (sticky is not None and bool(sticky.item())) or (scratch is not None and fused.sa1_stream_gave_up(scratch))
        if sticky is not None:
            sticky.zero_()
        if bad:
            raise RuntimeError("level-1 stream kernel: a consumer workgroup gave up waiting for the sampler in a step of this run; "
                               "its outputs (and every pose after it) are incomplete")

    def _step_rot(self, input, npcs_input, last_pose):
        """RotationNet up to its heads' raw per-point output (needs nothing of CoordinateNet's but, for one part, its geometry)."""
        P = self.num_parts
        last_pose = O.start_pose(last_pose)
        cam_cn, cam_n3, geom = npcs_input["_cloud"]
        if P == 1 and self.share_geometry:            # one part: RotationNet's cloud IS CoordinateNet's
            return self.net.regress_net.raw_point_rtvec(cam_cn, cam_n3=cam_n3, geom=geom)
        # every part's cloud canonicalised with that part's previous pose
        canon = {k: last_pose[k].reshape((-1,) + last_pose[k].shape[2:]) for k in ("rotation", "translation", "scale")}
        rcam = _canonicalize(input["points"], input["points_mean"], canon, num_parts=P)
        return self.net.regress_net.raw_point_rtvec(rcam[0], cam_n3=rcam[1])

    def _step_coord(self, npcs_input):
        return self.npcs_net(npcs_input)

    def _step_post(self, input, npcs_input, npcs_pred, last_pose):
        entered, last_pose = last_pose, O.start_pose(last_pose)
        pred_npcs = npcs_pred["nocs"].reshape(len(npcs_pred["nocs"]), self.num_parts, 3, -1)
        input["state"] = {"part": last_pose}
        lab32 = npcs_pred.pop("_labels_i32", None)   # CoordinateNet's fused read-out: the int32 labels of THIS prediction
        if lab32 is not None and not (self.track_cfg["gt_label"] or self.track_cfg["nocs2d_label"]):
            input["pred_labels_i32"] = lab32             # what the one-launch rotation read-out and pose fit take
            input["pred_labels"] = lab32 if self._overlap_nets(input) else lab32.long()
        else:
            input.pop("pred_labels_i32", None)
            input["pred_labels"] = torch.argmax(npcs_pred["seg"], dim=-2)
        input["pred_nocs"] = pred_npcs
        input["pred_label_conf"] = npcs_pred["seg"][:, 0]
        if self.track_cfg["gt_label"] or self.track_cfg["nocs2d_label"]:
            input["pred_labels"] = npcs_input["labels"]
        input.pop("_cloud", None)
        cloud = npcs_pred.pop("_cloud", None)        # CoordinateNet's cloud with the geometry its backbone used
        if self.share_geometry and self.num_parts == 1 and cloud is not None:
            input["_cloud"] = cloud
        out = self.net(input, test_mode=True)
        pose = out["part"]
        for name in ("st_fit", "rot_pool", "size"):
            if getattr(self, name) is not None:
                # the option's record joins CoordinateNet's maps (`st_*`, `rot_*`, `size_*`), so it travels with them through every batch form
                O.put_record(npcs_pred, name, out[name])
        # track_cfg/size: the fit returned the new size state beside the (held) pose; the guard judges that pose and its re-fit
        # replaces it, scale included, without touching the state; the motion model never touches the scale
        size_state = {k: pose[k] for k in O.SIZE_KEYS} if self.size is not None else None
        if self.guard is not None:
            pose = self._guard_step(input, npcs_pred, pose)
        # track_cfg/box: behind the guard (its verdict decides whether the frame counts), beside the motion model: neither reads the other
        box_hist = self._box_step(input, npcs_pred, entered) if self.box is not None else None
        if self.motion is not None:
            pose = self._motion_step(npcs_pred, entered, pose)
        if size_state is not None:
            pose = {**{k: v for k, v in pose.items() if k not in size_state}, **size_state}
        return pose if box_hist is None else {**{k: v for k, v in pose.items() if k != O.BOX_KEY}, O.BOX_KEY: box_hist}

    def _box_step(self, input, npcs_pred, entered):
        """The held box behind the guard, on the labels the fit used and the per-part NOCS maps: the frame's coordinates into the
        histograms that entered the step (`entered`: box_hist); its record joins CoordinateNet's maps (`box_*`); -> the new histograms."""
        from .pose_utils.pose_fit import part_box_hist
        x = self.box
        labels = input.get("pred_labels_i32")
        if labels is None:
            labels = input["pred_labels"].int().contiguous()
        verdict = npcs_pred["guard_verdict"] if self.guard is not None else None
        new, info = part_box_hist(labels, input["pred_nocs"].float().contiguous(), entered[O.BOX_KEY], bins=x["bins"], radial=x["radial"],
                                  quantile_permille=x["quantile_permille"], min_points=x["min_points"], verdict=verdict)
        O.put_record(npcs_pred, "box", info)
        return new

    def _motion_step(self, npcs_pred, entered, pose):
        """The motion model behind the fit and the guard: the pose the NEXT step starts from, out of the result that entered this
        step (`entered`: rotation / translation / measured) and this step's; its record joins CoordinateNet's maps (`motion_*`);
        -> the step's pose with next_rotation / next_translation / measured beside its three keys."""
        from .pose_utils.pose_fit import pose_extrapolate
        m = self.motion
        verdict = npcs_pred["guard_verdict"] if self.guard is not None else None
        rot, trans, measured, info = pose_extrapolate(entered["rotation"], entered["translation"], pose["rotation"], pose["translation"],
                                                      entered["measured"], bool(self.sym), m["max_angle"], m["max_shift"], gain=m["gain"],
                                                      verdict=verdict)
        O.put_record(npcs_pred, "motion", {**info, "rotation": rot, "translation": trans})
        return {"rotation": pose["rotation"], "scale": pose["scale"], "translation": pose["translation"],
                "next_rotation": rot, "next_translation": trans, "measured": measured}

    def _guard_step(self, input, npcs_pred, pose):
        """The guard behind the pose fit, on the labels the fit used; its record joins CoordinateNet's maps (`guard_*`), so it
        travels with them through every batch form; -> the step's pose (the re-fit where a lost part was recovered)."""
        from .pose_utils.pose_fit import part_fit_guard_cn
        g = self.guard
        labels = input.get("pred_labels_i32")
        if labels is None:
            labels = input["pred_labels"].int().contiguous()
        pose, info = part_fit_guard_cn(labels, input["pred_nocs"].float().contiguous(), input["points"].float().contiguous(),
                                       input["points_mean"], pose, inlier_th=g["inlier_th"], lost_below=g["lost_below"],
                                       min_members=g["min_members"], refit=g["refit"], num_hyps=g["num_hyps"], seed=g["seed"],
                                       b0=int(input.get("b0", 0)), yaxis_only=g.get("yaxis_only", False))
        O.put_record(npcs_pred, "guard", info)
        return pose

    # ---- the two networks side by side -------------------------------------------------------------------------------
    def _overlap_nets(self, input) -> bool:
        """The two backbones do not depend on each other (RotationNet needs CoordNet's labels only for its read-out): they
        run on two streams = two branches of the captured graph, each filling the other's latency-bound stretches and
        launch ramps / tails.  1.37 -> 1.18 ms per frame at one trajectory, 6.56 -> 6.40 ms per step at 32."""
        return (self.overlap_nets
                and not self.training and input["points"].is_cuda and fused.USE_ROT_READOUT
                and not (self.track_cfg["gt_label"] or self.track_cfg["nocs2d_label"]) and not self.net.return_point_rotation)

    def _fork_rotation_net(self, input, npcs_input, last_pose):
        small = len(input["points"]) <= 2      # one or two trajectories: every kernel is latency-bound, overlap all that can be (no gain from 4 up)
        dev = input["points"].device
        if getattr(self, "_side", None) is None:
            self._side = torch.cuda.Stream(device=dev)
        side = self._side
        main = torch.cuda.current_stream(dev)
        gstream = None
        if self.sampler_chunks > 1 and self.num_parts == 1 and self.share_geometry:
            # the geometry on a stream of its own, both networks forked right behind the canonicalisation: their first level
            # waits for the sampler's parts one by one, their second level for the rest of the geometry
            if getattr(self, "_gstream", None) is None:
                self._gstream = torch.cuda.Stream(device=dev)
            cam = _canonicalize(npcs_input["points"], npcs_input["points_mean"], npcs_input["canon_pose"])
            geom = self.npcs_net.backbone.precompute_geometry_streamed(cam[1], self.sampler_chunks, self._gstream, consumers=(side,),
                                                                       backbones=(self.net.regress_net.encoder,))
            if geom is not None:
                npcs_input["_cloud"] = (cam[0], cam[1], geom)
                gstream = self._gstream
        if gstream is None and not self._step_prep(input, npcs_input, last_pose, level1_only=small, side=side if self.overlap_geometry else None):
            return None
        side.wait_stream(main)
        with torch.cuda.stream(side):
            raw = self._step_rot(input, npcs_input, last_pose)

        def join():
            main.wait_stream(side)
            if gstream is not None:
                main.wait_stream(gstream)
            raw.record_stream(main)
            input["_raw"] = raw
        return join

    def _graph_usable(self, input) -> bool:
        return (self.use_graph and not self.training and input["points"].is_cuda
                and not (self.track_cfg["gt_label"] or self.track_cfg["nocs2d_label"]))

    def _cached(self, key, build):
        """The captured object of this batch form (`self._graph`: a TrackStepGraph, a TrackLanes, or the re-crop lanes' list of
        TrackStepGraph), built when there is none, when it was captured for another `key`, or when a weight under it changed."""
        g = self._graph
        if g is None or self._graph_key != key or any(x.stale() for x in (g if isinstance(g, list) else [g])):
            self._graph, self._graph_key = build(), key
        return self._graph

    def _graph_step(self, input, last_pose):
        """One frame through the captured graph (captured on first use for this batch shape); outputs are cloned out
        of the graph's static buffers."""
        points, mean = input["points"], input["points_mean"]
        graph = self._cached((tuple(points.shape), str(points.device)), lambda: G.TrackStepGraph(self, points, mean, last_pose))   # (the whole batch: b0 = 0)
        return graph.replay_cloned(points, mean, last_pose)

    def _lanes_usable(self, input) -> bool:
        """From 32 trajectories on the captured step runs as two free-running lanes (graph.TrackLanes; +2.8 % frames/s,
        -1 % at 8 and 16).  Not with the on-the-fly re-crop: it reads the previous pose on the host every frame."""
        B = input["points"].shape[0]
        return self._graph_usable(input) and not self.nocs_otf and B >= 32 and B % 2 == 0

    def _recrop_slice(self, i, input, last_pose, sl, defer=None):
        """nocs_otf (reference model.py:425-452) for the trajectories `sl` of frame i: re-crop around the pose predicted for
        frame i-1 -- on the device (captra_amd/nocs_otf.py: one crop launch + one ragged sampling launch).  `last_pose` holds
        those trajectories only.  -> (points (b,3,N) mean-subtracted, labels (b,N), nocs (b,3,N)).  With the pose on the device the
        stage's one host round trip is the crops' member counts; `defer` (an int: upper bound of the candidate lists' length) takes
        that one away too (nocs_otf.full_data_batch_arrays) and appends the device word [rare-path instance met, longest list] to
        the result -- the caller reads it a frame late (_OtfCheck) and runs the frame again without `defer` when it is set."""
        from .nocs_otf import full_data_batch_arrays, to_host
        last_pose = O.start_pose(last_pose)        # (track_cfg/motion: the crop follows the prediction)
        pre = input.get("pre_fetched")
        if pre is None:
            raise ValueError("nocs_otf=True needs the frame's depth and mask tensors (meta['pre_fetched']): reading depth.png / "
                             "mask.png from disk (cv2) is outside this build")
        npcs = self.npcs_feed_dict[i]
        N = input["points"].shape[2]
        b = last_pose["scale"].shape[0]
        gt = input.get("gt_root_host")
        if gt is None:
            gt = {k: to_host(v[:, self.root].double().contiguous()) for k, v in input["gt_part"].items()}
        gt = {k: v[sl] for k, v in gt.items()}
        depth, mask = pre["depth"][sl], pre["mask"][sl]
        det = self._detections(pre, sl)
        gt64 = {"rotation": np.asarray(gt["rotation"], np.float64).reshape(b, 3, 3),
                "translation": np.asarray(gt["translation"], np.float64).reshape(b, 3),
                "scale": np.asarray(gt["scale"], np.float64).reshape(b)}
        gtd = input.get("gt_root_dev")
        gtd = None if gtd is None else {k: v[sl] for k, v in gtd.items()}
        trans_d, scale_d = last_pose["translation"][:, self.root].reshape(b, 3), last_pose["scale"][:, self.root].reshape(b)
        # track_cfg/otf_thin: keyed by the trajectory's place in the whole batch and the frame, so that a lane draws what the whole
        # batch draws and a replayed frame what its first run drew
        thin = None if self.otf_thin is None else (self.otf_thin["seed"], i, sl.start or 0)
        # the camera model: the table whole, cam_of sliced with the lane exactly as the depth images are
        cameras = None if self.camera is None else (self.camera[0], self.camera[1][sl])
        if (OTF_POSE_ON_DEVICE or det is not None) and depth.is_cuda and trans_d.dtype == torch.float32 and scale_d.dtype == torch.float32:
            # the crop's box / centre / radius derived on the device from the pose (captra_crop_box): no round trip for the pose
            # (the detector route exists in this form only: its selection is captra_crop_box_det)
            full = full_data_batch_arrays(depth, mask, None, None, gt64, N, stacked=True, pose_dev=(trans_d, scale_d, float(self.radius)), gt_dev=gtd,
                                          defer=defer, mean=npcs["points_mean"][sl], det=det, thin=thin, cameras=cameras)
            if thin is not None:
                self._otf_thin_rec.setdefault(i, {})[sl.start or 0] = full["_thinned"]     # (a replay of the frame puts its own in place)
            if defer is not None:
                return full["points_cn"], full["labels"], full["nocs_cn"], full["_info"]
        elif thin is not None:
            raise ValueError("track_cfg/otf_thin/device thins the re-crop's lists on the device: it needs the frames and an fp32 pose there "
                             "(CUDA tensors, CAPTRA_OTF_POSE_ON_DEVICE not 0)")
        elif det is not None:
            raise ValueError("track_cfg/nocs2d_label with detections in the frame: the selection runs on the device from an fp32 pose")
        else:
            defer = None
            cs = to_host(torch.cat([trans_d, scale_d.reshape(b, 1)], dim=1).double())
            full = full_data_batch_arrays(depth, mask, cs[:, :3], self.radius * cs[:, 3], gt64, N, stacked=True, cameras=cameras)
        points = (full["points"].float() - npcs["points_mean"][sl].reshape(b, 1, 3)).transpose(1, 2).contiguous()
        return points, full["labels"].contiguous(), full["nocs"].float().transpose(1, 2).contiguous()

    def _detections(self, pre, sl):
        """The detector route's inputs for the trajectories `sl` (reference model.py:437-439 -> nocs_data_process.py:206-229), or None:
        taken when track_cfg/nocs2d_label is set AND the frame carries its detections (meta['pre_fetched'] det_*).  With the flag set
        and no detections the pre-fetched mask is used, as before -- said once per model object."""
        if not self.track_cfg["nocs2d_label"]:
            return None
        if not all(k in pre for k in DET_KEYS):
            if not self._det_missing_logged:
                self._det_missing_logged = True
                logging.getLogger(__name__).warning("track_cfg/nocs2d_label is set but the frames carry no detections (meta['pre_fetched'] %s): "
                                                    "the re-crop uses the pre-fetched instance mask", " / ".join(DET_KEYS))
            return None
        try:
            category = int(self.det_category)
        except (TypeError, ValueError):
            raise ValueError(f"track_cfg/nocs2d_label: the detections' class ids are integers, category {self.det_category!r} is not one") from None
        det = {k: pre[k][sl] for k in DET_KEYS}
        det["category"] = category
        return det

    def _recrop(self, i, input, last_pose, defer=None):
        """The whole batch of frame i re-cropped in place (input / npcs feed dicts); -> the deferred check's device word or None."""
        npcs = self.npcs_feed_dict[i]
        res = self._recrop_slice(i, input, last_pose, slice(None), defer=defer)
        input["points"], input["labels"], npcs["nocs"] = res[:3]
        npcs["points"], npcs["labels"] = input["points"], input["labels"]
        return res[3] if len(res) > 3 else None

    def _otf_defer_usable(self, input) -> bool:
        """The re-crop without its round trip: pose on the device, no per-frame hook that publishes a frame's pose at once (the
        distributed harness's exchange: a frame that is run again a frame later would already be out)."""
        return (OTF_DEFER and OTF_POSE_ON_DEVICE and self.nocs_otf and input["points"].is_cuda and not self.training
                and self.frame_hook is None)

    # ---- nocs_otf at batch >= 32: two lanes of trajectories, half a frame apart ------------------------------------------
    def _otf_lanes_usable(self, input) -> bool:
        """The re-crop's sampler (<= 20480 -> 4096 points: 4095 dependent rounds, ONE workgroup per trajectory) leaves
        240 of the 256 CUs idle for 2.8 ms of a 10.8 ms step.  With the batch split into two lanes on two streams, started
        half a cycle apart, one lane samples while the other runs its networks.  The host stays single-threaded: it serves
        lane 0's frame i+1 as soon as lane 0's pose i is back (lane 1's frame i is executing meanwhile), then lane 1's."""
        B = input["points"].shape[0]
        return (self.nocs_otf and input["points"].is_cuda and not self.training and B >= 32 and B % 2 == 0
                and not (self.track_cfg["gt_label"] or self.track_cfg["nocs2d_label"]))

    def _otf_lane_frames(self, pose0):
        """The frame closures of `forward` for the two re-crop lanes (`_otf_lanes_usable`): each lane re-crops its half of the
        batch and runs its step on a stream of its own; `commit` assembles the batch-wide tensors on the caller's stream."""
        feed = self.feed_dict
        B = feed[1]["points"].shape[0]
        half = B // 2
        slices = [slice(0, half), slice(half, B)]
        dev = feed[1]["points"].device
        cur = torch.cuda.current_stream(dev)
        if G.SPLIT_OTF_LANES:
            pairs = G.lane_streams(dev, 2)       # process-wide explicit streams: see captra_amd/graph.py SPLIT_OTF_LANES
            streams, sides = [m_ for m_, _ in pairs], [s_ for _, s_ in pairs]
        else:
            if getattr(self, "_otf_streams", None) is None:
                key = (dev.index if dev.index is not None else torch.cuda.current_device())
                if key not in _OTF_LANE_STREAMS:
                    _OTF_LANE_STREAMS[key] = [torch.cuda.Stream(device=dev) for _ in slices]
                self._otf_streams = _OTF_LANE_STREAMS[key]
            streams, sides = self._otf_streams, [None, None]
        graphs = None
        if self._graph_usable(feed[1]):
            graphs = self._cached(("otf", tuple(feed[1]["points"].shape), str(dev)), lambda: [
                G.TrackStepGraph(self, feed[1]["points"][s].contiguous(), feed[1]["points_mean"][s].contiguous(),
                                 {k: v[s].contiguous() for k, v in pose0.items()}, split_side=side, allow_split_k=False, b0=s.start) for s, side in zip(slices, sides)])
        lane_pose = [{k: v[s].clone() for k, v in pose0.items()} for s in slices]
        for st in streams:
            st.wait_stream(cur)
        state = {"sampled": None}      # recorded on a lane's stream when its re-crop (crop + sampling launch) of the current frame is enqueued

        def run_frame(i, poses_in, bounds):
            """Frame i of both lanes from the poses entering it; bounds[l] = the sync-free re-crop's stride bound of lane l or None
            (the synchronous stage).  -> ((parts, events), poses out, deferred checks)."""
            input = feed[i]
            parts, done, poses_out, checks = [], [], [], []
            for l, s in enumerate(slices):
                with torch.cuda.stream(streams[l]):
                    if state["sampled"] is not None:
                        # the other lane's sampling of ITS current frame is over before this lane starts to sample: the two
                        # samplers never share the chip (each runs under the other lane's networks), whatever phase the lanes
                        # would drift into by themselves.  A GPU-side wait: the host goes on enqueuing.
                        if bounds[l] is not None:
                            streams[l].wait_event(state["sampled"])
                        else:
                            state["sampled"].synchronize()
                    res = self._recrop_slice(i, input, poses_in[l], s, defer=bounds[l])
                    pts, labels, nocs = res[:3]
                    if len(res) > 3 and res[3] is not None:
                        checks.append(_OtfCheck(res[3]))
                    state["sampled"] = torch.cuda.Event()
                    state["sampled"].record(streams[l])
                    mean = input["points_mean"][s]
                    if graphs is not None:
                        cur_npcs, pose = graphs[l].replay_cloned(pts, mean, poses_in[l])
                    else:
                        cur_npcs, pose = self.track_step(*G.step_inputs(pts, mean, labels, b0=s.start), poses_in[l])
                        cur_npcs = {k: v for k, v in cur_npcs.items() if torch.is_tensor(v)}
                    poses_out.append(pose)
                    ev = torch.cuda.Event()
                    ev.record(streams[l])
                parts.append((pts, labels, nocs, pose, cur_npcs))
                done.append(ev)
            return (parts, done), poses_out, checks

        def commit(i, result):
            """The frame's batch-wide tensors, assembled on the caller's stream (GPU-side waits: the lanes do not stop)."""
            parts, done = result
            input, npcs_in = feed[i], self.npcs_feed_dict[i]
            for ev in done:
                cur.wait_event(ev)
            for part in parts:
                for x in part[:3]:
                    x.record_stream(cur)
                for d in part[3:]:
                    for v in d.values():
                        v.record_stream(cur)
            input["points"] = torch.cat([p[0] for p in parts])
            input["labels"] = torch.cat([p[1] for p in parts])
            npcs_in["nocs"] = torch.cat([p[2] for p in parts])
            npcs_in["points"], npcs_in["labels"] = input["points"], input["labels"]
            pose = {k: torch.cat([p[3][k] for p in parts]) for k in parts[0][3]}
            return {k: torch.cat([p[4][k] for p in parts]) for k in parts[0][4]}, pose

        def join():
            for st in streams:
                cur.wait_stream(st)

        first = OTF_FIRST_BOUND * feed[1]["points"].shape[2] if self._otf_defer_usable(feed[1]) else None
        return run_frame, commit, lane_pose, [first] * len(slices), join

    def _lane_frames(self, pose0):
        """The frame closures of `forward` for pre-cropped clouds from 32 trajectories on (`_lanes_usable`): graph.TrackLanes hand
        their poses over themselves, the caller's stream only copies the frame's records out.  Never a deferred check."""
        feed = self.feed_dict
        points, mean = feed[1]["points"], feed[1]["points_mean"]
        had = self._graph
        lanes = self._cached(("lanes", tuple(points.shape), str(points.device)),
                             lambda: G.TrackLanes(self, points, mean, pose0, lanes=2, keep_npcs=True))
        if lanes is had:
            lanes.set_pose(pose0)          # (a new TrackLanes starts from the pose it was built with)

        def run_frame(i, poses_in, bounds):
            return lanes.step(feed[i]["points"], feed[i]["points_mean"], sync_inputs=(i == 1)), None, []

        def commit(i, slot):
            pose, npcs = lanes.gather(slot, npcs=True)
            return {k: v.clone() for k, v in npcs.items()}, {k: v.clone() for k, v in pose.items()}

        return run_frame, commit, None, [None], None

    def _batch_frames(self, pose0):
        """The frame closures of `forward` for the whole batch on the caller's stream: re-cropped in place (nocs_otf), then one
        captured graph or the eager step.  Not a lane: the few-trajectory split-k form stays allowed, and a frame costs no
        concatenation and no event (the one-trajectory latency would pay for them)."""
        feed = self.feed_dict

        def run_frame(i, pose_in, bounds):
            lp = {k: v.clone() for k, v in pose_in.items()}
            info = self._recrop(i, feed[i], lp, defer=bounds[0]) if self.nocs_otf else None
            if self._graph_usable(feed[i]):
                out = self._graph_step(feed[i], lp)
            else:
                out = self.track_step(feed[i], self.npcs_feed_dict[i], lp)
            return out, out[1], ([] if info is None else [_OtfCheck(info)])

        first = OTF_FIRST_BOUND * feed[1]["points"].shape[2] if self._otf_defer_usable(feed[1]) else None
        return run_frame, (lambda i, out: out), pose0, [first], None

    def forward(self, save=False):
        """The frame loop.  A batch form hands in `run_frame(i, poses_in, bounds) -> (result, poses_out, checks)`, which enqueues
        frame i from the poses entering it (bounds[l]: the sync-free re-crop's stride bound of lane l, None = the synchronous
        stage; checks: the `_OtfCheck` of every sync-free crop), and `commit(i, result) -> (npcs_pred, pose)`, the frame's
        batch-wide records on the caller's stream."""
        feed = self.feed_dict
        pred_poses, npcs_pred = [self._initial_pose()], [None]
        records = {name: {} for name in O.STEP_RECORDS if getattr(self, name) is not None}     # option that is on -> {frame: its record}
        self._otf_thin_rec = {}
        if self.frame_hook is not None:
            self.frame_hook(0, pred_poses[0])
        self.timer.tick()
        if len(feed) > 1:
            if self._otf_lanes_usable(feed[1]) and self.otf_lanes:
                frames = self._otf_lane_frames
            elif self._lanes_usable(feed[1]):
                frames = self._lane_frames
            else:
                frames = self._batch_frames
            with torch.no_grad():
                # (track_cfg/motion: the travelling dict carries the prediction beside the pose; frame 0's is a track's start)
                # (track_cfg/size: likewise the size state)
                run_frame, commit, poses, bounds, join = frames(O.entering(pred_poses[0], self))
                commit = O.commit_with_records(commit, records)
                pending = None                  # (frame, poses that entered it, its deferred checks)

                def settle():
                    """The pending frame's verdicts, read a frame late: a rare-path instance -> that frame once more on the
                    synchronous stage, in place of its first run (-> []); else the lanes' longest candidate lists."""
                    nonlocal pending, poses
                    if pending is None:
                        return []
                    (pi, pin, checks), pending = pending, None
                    verdicts = [c.read() for c in checks]
                    if not any(rare for rare, _ in verdicts):
                        return [longest for _, longest in verdicts]
                    result, poses, _ = run_frame(pi, pin, [None] * len(bounds))
                    npcs_pred[pi], pred_poses[pi] = commit(pi, result)
                    if self.otf_thin is not None:
                        # a bound outgrown is outgrown ONCE: the next frame's bound follows the verdicts' longest lists
                        return [longest for _, longest in verdicts]
                    return []

                for i in range(1, len(feed)):
                    longest = settle()
                    if longest:
                        bounds = [_otf_bound(n, feed[i]["points"].shape[2]) for n in longest]
                    # the reference draws (and discards) a perturbed pose every frame (model.py:414); draw it too so that seeded runs
                    # consume the generator identically -- AFTER a replay of the previous frame (its thinning permutations come out of
                    # the same numpy generator and precede this frame's draw in the reference's order)
                    consume_noise_draws(feed[i - 1]["gt_part"], self.pose_perturb_cfg)
                    poses_in = poses
                    result, poses, checks = run_frame(i, poses_in, bounds)
                    npcs, pose = commit(i, result)
                    npcs_pred.append(npcs)
                    pred_poses.append(pose)
                    if checks:
                        pending = (i, poses_in, checks)
                    if self.frame_hook is not None:
                        self.frame_hook(i, pose)
                settle()
                if join is not None:
                    join()
        self.pred_dict = {"poses": pred_poses, "npcs_pred": npcs_pred}
        # the options' records (track_options.py), each only when its option is on: a step's, the host loop's two, frame 0's one
        for name, record in records.items():
            self.pred_dict[name] = [None] + [record[i] for i in range(1, len(feed))]
        if self.otf_thin is not None and self.nocs_otf:
            rec = self._otf_thin_rec        # (a lane wrote its slice of the frame: the slices in batch order)
            self.pred_dict["otf_thin"] = [None] + [next(iter(rec[i].values())) if len(rec[i]) == 1 else torch.cat([rec[i][k] for k in sorted(rec[i])])
                                                   for i in range(1, len(feed))]
        if self.depth_filter is not None:
            self.pred_dict["depth_filter"] = [f.get("depth_filter_removed") for f in feed]       # (None: a frame without depth)
        if self.image_fit is not None:
            self.pred_dict["image_fit"] = self._image_fit_rec
        if self._camera_host is not None:
            self.pred_dict["camera"] = self._camera_host
        self.check_l1_stream()
        if save:
            self._save(list(map(_frame_names, feed)))

    def _save(self, frame_nums):
        """Per-trajectory pickle {'pred': {'poses','corners'}, 'gt': {'poses','corners'}, 'frame_nums'}
        (reference model.py:482-509).  Predicted NOCS corners = `get_pred_nocs_corners` of the points' own-part predicted
        coordinates: per part the symmetric extent [-max|x|, +max|x|] (model.py:489-493) -- the same boxes compute_loss
        evaluates, so the offline IoU tables (captra_amd/eval.py) agree with the in-loop avg_iou."""
        from .loss import choose_coord_by_label
        from .pose_utils.bbox_utils import get_pred_nocs_corners, pred_nocs_corners_device
        gt_corners = self.feed_dict[0]["meta"]["nocs_corners"].cpu().numpy()
        corner_list, maps = [None], []
        for i in range(1, len(self.pred_dict["poses"])):
            pred = self.pred_dict["npcs_pred"][i]
            pred_labels = torch.max(pred["seg"], dim=-2)[1]                                        # (B,N)
            pred_nocs = choose_coord_by_label(pred["nocs"].transpose(-1, -2), pred_labels)         # (B,N,3)
            if self.eval_device:
                maps.append((pred_labels, pred_nocs))
            else:
                corner_list.append(get_pred_nocs_corners(pred_labels, pred_nocs, self.num_parts))
        if maps:
            # every frame in one launch and one read; float64 at the pickle boundary like the host function (same values, bit for bit)
            corners = pred_nocs_corners_device(torch.stack([m[0] for m in maps]), torch.stack([m[1] for m in maps]), self.num_parts)
            corner_list.extend(corners.double().cpu().numpy())
        if "box" in self.pred_dict:
            # track_cfg/box: the box held after frame i (causal) where it is established, the frame's own otherwise
            from .pose_utils.bbox_utils import held_box_corners
            for i in range(1, len(corner_list)):
                corner_list[i] = held_box_corners(corner_list[i], self.pred_dict["box"][i]["extent"].detach().cpu().numpy())
        to_np = lambda pose: {k: v.detach().cpu().numpy() for k, v in pose.items()}
        save_dict = {"pred": {"poses": [to_np(p) for p in self.pred_dict["poses"]], "corners": corner_list},
                     "gt": {"poses": [to_np(f["gt_part"]) for f in self.feed_dict], "corners": gt_corners},
                     "frame_nums": frame_nums}
        save_dict.update(O.records_to_numpy(self.pred_dict, guard_yaxis_only=self.guard is not None and self.guard.get("yaxis_only", False)))
        records = []
        for i, path in enumerate(self.feed_dict[0]["meta"]["path"]):
            instance, track_num = path.split(".")[-2].split("/")[-3:-1]
            records.append((f"{instance}_{track_num}.pkl", get_ith_from_batch(save_dict, i, to_single=False)))
        if self.result_sink is not None:
            self.result_sink(records)
        else:
            write_result_pickles(self.cfg["experiment_dir"], records)

    def compute_loss(self, test=False, per_instance=False, eval_iou=False, test_prefix=None):
        """The reference's compute_loss (model.py:511-593): per-part rdiff / tdiff / sdiff / 5deg5cm averaged over frames
        1..T-1 for the prediction and for its initialisation (= the previous frame's prediction), the segmentation and
        NOCS losses of CoordinateNet's maps when the frames carry labels / NOCS, and with `eval_iou` the three box IoUs
        (canonical boxes, posed predicted box, ground-truth box under the predicted pose; host-side numpy as in the
        reference, or with cfg['eval_device'] all frames in one call on the GPU: `_device_iou`).  Keys as in the reference, including its quirk of storing the per-frame NOCS losses under
        'frame_seg'."""
        from .loss import choose_coord_by_label, compute_miou_loss, compute_nocs_loss
        from .pose_utils.bbox_utils import eval_single_part_iou, get_pred_nocs_corners, held_box_corners
        avg_pred, avg_init, all_pred, all_init = {}, {}, {}, {}
        avg_iou, all_iou, seg_losses, all_seg, nocs_losses, all_nocs = {}, {}, [], {}, [], {}
        poses = self.pred_dict["poses"]
        gt_corners = self.feed_dict[0]["meta"]["nocs_corners"].float().cpu()                       # (B,P,2,3)
        device_frames = []              # eval_device: (frame, predicted labels, own-part NOCS) of the frames whose IoUs are still to come
        for i, pose in enumerate(poses):
            diff, per = eval_part_full(self.feed_dict[i]["gt_part"], pose, per_instance=per_instance, yaxis_only=self.sym)
            all_pred[i] = deepcopy(diff)
            if i == 0:
                continue
            add_dict(avg_pred, diff)
            if per_instance:
                self.record_per_diff(self.feed_dict[i], per)
            init_diff, _ = eval_part_full(self.feed_dict[i]["gt_part"], poses[i - 1], per_instance=False, yaxis_only=self.sym)
            add_dict(avg_init, init_diff)
            all_init[i] = deepcopy(init_diff)
            npcs_pred, npcs_feed = self.pred_dict["npcs_pred"][i], self.npcs_feed_dict[i]
            if npcs_pred is None:
                continue
            if "labels" in npcs_feed:
                all_seg[i] = compute_miou_loss(npcs_pred["seg"], npcs_feed["labels"].long(), per_instance=False)
                seg_losses.append(all_seg[i])
            pred_labels = torch.max(npcs_pred["seg"], dim=-2)[1]
            if "nocs" in npcs_feed:
                all_nocs[i] = compute_nocs_loss(npcs_pred["nocs"], npcs_feed["nocs"], labels=pred_labels, confidence=None,
                                                loss="l2", self_supervise=False, per_instance=False)
                nocs_losses.append(all_nocs[i])
            if eval_iou and self.eval_device:
                device_frames.append((i, pred_labels, choose_coord_by_label(npcs_pred["nocs"].transpose(-1, -2), pred_labels)))
            elif eval_iou:
                pred_nocs = choose_coord_by_label(npcs_pred["nocs"].transpose(-1, -2), pred_labels)                 # (B,N,3)
                pred_corners = torch.from_numpy(get_pred_nocs_corners(pred_labels, pred_nocs, self.num_parts)).float()
                if "box" in self.pred_dict:         # track_cfg/box: the held box where it is established
                    pred_corners = held_box_corners(pred_corners, self.pred_dict["box"][i]["extent"].cpu())
                iou, per_iou = eval_single_part_iou(gt_corners, pred_corners, self.feed_dict[i]["gt_part"], pose,
                                                    separate="both", nocs=self.nocs_otf, sym=self.sym)
                iou = {name: {p: float(v) for p, v in d.items()} for name, d in iou.items()}
                add_dict(avg_iou, iou)
                if per_instance:
                    self.record_per_diff(self.feed_dict[i], per_iou)
                all_iou[i] = deepcopy(iou)
        if device_frames:
            self._device_iou(device_frames, gt_corners, per_instance, avg_iou, all_iou)
        n = max(len(poses) - 1, 1)
        loss_dict = {"avg_pred": divide_dict(avg_pred, n), "avg_init": divide_dict(avg_init, n),
                     "frame_pred": all_pred, "frame_init": all_init}
        if seg_losses:
            loss_dict.update({"avg_seg": torch.mean(torch.stack(seg_losses)), "frame_seg": all_seg})
        if nocs_losses:
            loss_dict.update({"avg_nocs": torch.mean(torch.stack(nocs_losses)), "frame_seg": all_nocs})
        if eval_iou:
            loss_dict.update({"avg_iou": divide_dict(avg_iou, n), "frame_iou": all_iou})
        self.loss_dict = loss_dict

    def _device_iou(self, frames, gt_corners, per_instance, avg_iou, all_iou):
        """cfg['eval_device']: the box IoUs of all `frames` on the GPU (pose_utils/bbox_utils.py, captra_box_iou /
        captra_part_extent) -- one corner launch, one IoU call, one read -- then the same entries as the host path: batch means as
        Python floats into `avg_iou` / `all_iou`, per-instance float64 arrays into the per-instance records."""
        from .pose_utils.bbox_utils import eval_single_part_iou_device, pred_nocs_corners_device
        names, idx = ("npcs_iou", "iou", "gt_bbox_iou"), [f[0] for f in frames]
        pred_corners = pred_nocs_corners_device(torch.stack([f[1] for f in frames]), torch.stack([f[2] for f in frames]), self.num_parts)
        if "box" in self.pred_dict:             # track_cfg/box: the held box where it is established
            from .pose_utils.bbox_utils import held_box_corners
            pred_corners = held_box_corners(pred_corners, torch.stack([self.pred_dict["box"][i]["extent"] for i in idx]))
        dev = pred_corners.device
        stack = lambda ds: {k: torch.stack([d[k].to(dev) for d in ds]) for k in ("rotation", "translation", "scale")}
        res = eval_single_part_iou_device(gt_corners.to(dev), pred_corners, stack([self.feed_dict[i]["gt_part"] for i in idx]),
                                          stack([self.pred_dict["poses"][i] for i in idx]), nocs=self.nocs_otf, sym=self.sym)
        host = torch.stack([res[name] for name in names]).double().cpu().numpy()                   # (3,F,B,P): the only read
        for f, i in enumerate(idx):
            per_iou = {name: {p: host[k, f, :, p].copy() for p in range(host.shape[-1])} for k, name in enumerate(names)}
            iou = {name: {p: float(np.mean(v)) for p, v in d.items()} for name, d in per_iou.items()}
            add_dict(avg_iou, iou)
            if per_instance:
                self.record_per_diff(self.feed_dict[i], per_iou)
            all_iou[i] = deepcopy(iou)

    def test(self, save=False, no_eval=False, epoch=0):
        self.forward(save=save)
        if no_eval:
            self.loss_dict = {}
        else:
            self.compute_loss(test=True, per_instance=save, eval_iou=True, test_prefix="test")
