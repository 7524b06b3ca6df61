"""Holding the track's box inside the track loop (track_cfg: {box: {hold: True, ...}}) on the synthetic trajectories: the one launch per
step and what it reads, the histograms in the travelling pose dict as the loop's whole state, the captured step, the lanes, the
on-the-fly re-crop in its deferred and replayed forms, the guard's verdict, the size and the motion option beside it, the boxes the
pickle and the IoUs use, and the option switched off.  Nothing here asserts that the held box improves an IoU: tools/bench_box.py
measures that."""
import pickle

import numpy as np
import pytest

from tests import box_judge as J

BOX = {"hold": True, "quantile": 0.95, "bins": 64, "min_points": 16}
REC_KEYS = ("extent", "frame", "added", "total")
POSE_KEYS = ("rotation", "scale", "translation")
SHAPES = {"bottle": (4, 5), "drawers": (2, 4)}                            # tag -> (B, T)
IOU_TOL = 2e-3                                                            # tests/test_iou_gpu.py: host against device IoUs


def _box(tag, **kw):
    return {**BOX, "radial": tag == "bottle", **kw}                       # (the symmetric category takes the radial extents)


def _model(device, tag, hipgraph=False, experiment_dir="/tmp/captra_test_exp", eval_device=None, **track_cfg):
    from captra_amd import synthetic as clouds
    from captra_amd.configs import make_config
    from captra_amd.trainer import Trainer
    cat, objcfg, kind, _, _, wseed, _ = clouds.PHYSICAL_SETUPS[tag]
    cfg = make_config(cat, objcfg, experiment_dir=str(experiment_dir))
    for key, val in track_cfg.items():
        if val is not None:
            cfg["track_cfg"][key] = dict(val)
    cfg["hipgraph"] = hipgraph
    cfg["init_frame"]["gt"] = True
    if eval_device is not None:
        cfg["eval_device"] = eval_device
    trainer = Trainer(cfg)
    shapes = {k: tuple(v.shape) for k, v in trainer.model.state_dict().items()}
    trainer.model.load_state_dict(clouds.make_physical_state_dict(shapes, wseed, cfg["num_parts"], bool(cfg["obj_sym"]), kind))
    B, T = SHAPES[tag]
    return trainer, cfg, clouds.make_trajectory(kind, B, T, seed=7)


def _run(device, tag, save=False, no_eval=True, **kw):
    import torch
    trainer, cfg, data = _model(device, tag, **kw)
    torch.manual_seed(4321)
    pred, loss = trainer.test(data, save=save, no_eval=no_eval)
    return trainer.model, cfg, data, pred, loss


class _Spy:
    """Around part_box_hist as EvalTrackModel._box_step calls it: every call's arguments and results (cloned)."""

    def __init__(self):
        from captra_amd.pose_utils import pose_fit
        self.mod, self.real, self.calls = pose_fit, pose_fit.part_box_hist, []

    def __enter__(self):
        def spy(labels, src, state, **kw):
            new, info = self.real(labels, src, state, **kw)
            verdict = kw.get("verdict")
            self.calls.append(dict(labels=labels.clone(), src=src.clone(), state=state.clone(), verdict=None if verdict is None else verdict.clone(),
                                   kw={k: v for k, v in kw.items() if k != "verdict"}, new=new.clone(), info={k: v.clone() for k, v in info.items()}))
            return new, info
        self.mod.part_box_hist = spy
        return self

    def __exit__(self, *a):
        self.mod.part_box_hist = self.real


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a.cpu().numpy()), np.ascontiguousarray(b.cpu().numpy())
    assert a.dtype == b.dtype and a.shape == b.shape, what
    np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32), err_msg=str(what))


def _same_run(a, b, frames, what, records=("box",)):
    for i in range(1, frames):
        assert set(a["poses"][i]) == set(b["poses"][i]) == set(POSE_KEYS)
        for k in POSE_KEYS:
            _same_bits(a["poses"][i][k], b["poses"][i][k], f"{what} frame {i} {k}")
        for name in records:
            assert set(a[name][i]) == set(b[name][i])
            for k in a[name][i]:
                _same_bits(a[name][i][k], b[name][i][k], f"{what} frame {i} {name} {k}")


def _judge_call(call):
    """The judge on one spied call -> its outputs; the call's own are asserted equal, bit for bit."""
    import torch
    n = lambda t: None if t is None else t.cpu().numpy()          # noqa: E731
    kw = call["kw"]
    want = J.judge_batch(n(call["labels"]), n(call["src"]), n(call["state"]), n(call["verdict"]), kw["bins"], bool(kw["radial"]),
                         kw["quantile_permille"], kw["min_points"])
    assert torch.equal(call["new"].cpu(), torch.from_numpy(want["hist"]))
    for k in REC_KEYS:
        assert torch.equal(call["info"][k].cpu(), torch.from_numpy(want["frame" if k == "frame" else k])), k
    return want


# ================================================================================================ 1. one call per step, one state
@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["bottle", "drawers"])
def test_one_call_per_step_and_the_dict_is_the_state(device, tag, tmp_path, capsys):
    import torch
    from captra_amd import _lib
    from captra_amd import eval as ev
    _lib.prof_enable(True)
    _lib.prof_reset()
    try:
        with _Spy() as spy:
            model, cfg, data, pred, _ = _run(device, tag, save=True, experiment_dir=tmp_path, box=_box(tag))
        torch.cuda.synchronize()
        launches = _lib.prof_read("part_box_hist")[1]
    finally:
        _lib.prof_enable(False)
    T = len(data)
    B, P = pred["poses"][0]["scale"].shape
    assert model.box == {"quantile_permille": 950, "bins": 64, "min_points": 16, "radial": tag == "bottle"}
    assert launches == T - 1 and len(spy.calls) == T - 1 and set(pred) == {"poses", "npcs_pred", "box"}
    assert len(pred["box"]) == T and pred["box"][0] is None
    grown = 0
    for i in range(1, T):
        call, rec, npcs = spy.calls[i - 1], pred["box"][i], pred["npcs_pred"][i]
        assert set(pred["poses"][i]) == set(POSE_KEYS) and set(rec) == set(REC_KEYS) and not any(k.startswith("box_") for k in npcs)
        assert call["kw"] == {"bins": 64, "radial": tag == "bottle", "quantile_permille": 950, "min_points": 16} and call["verdict"] is None
        # what the launch read: the labels the fit used and CoordinateNet's per-part maps of this frame
        assert call["labels"].dtype == torch.int32 and torch.equal(call["labels"].long(), torch.argmax(npcs["seg"], dim=-2))
        _same_bits(call["src"], npcs["nocs"].reshape(B, P, 3, -1).float(), f"frame {i} src")
        # the state that enters a step is the one the step before left; a track starts empty
        if i == 1:
            assert call["state"].shape == (B, P, 3, 64) and call["state"].dtype == torch.int32 and not call["state"].any()
        else:
            assert torch.equal(call["state"], spy.calls[i - 2]["new"])
        want = _judge_call(call)
        for k in REC_KEYS:
            _same_bits(rec[k], call["info"][k], f"frame {i} record {k}")
        assert rec["extent"].shape == (B, P, 3) and rec["extent"].dtype == torch.float32 and rec["added"].shape == (B, P) and rec["added"].dtype == torch.int32
        grown += int(want["added"].sum())
        print(tag, "frame", i, "extent", rec["extent"].cpu().numpy().round(4).tolist(), "frame's", rec["frame"].cpu().numpy().round(4).tolist(),
              "added", rec["added"].cpu().numpy().tolist(), "total", rec["total"].cpu().numpy().tolist())
    # counted once per frame: what is held is what the frames added
    assert int(pred["box"][T - 1]["total"].sum()) == grown > 0 and bool((pred["box"][T - 1]["extent"] > 0).any())
    # the dict a step returns is the whole state: the step on it again gives the loop's bits, and counts the frame once
    feed, npcs_feed = model.feed_dict, model.npcs_feed_dict
    i = T - 2
    state = {**pred["poses"][i], "box_hist": spy.calls[i - 1]["new"]}
    with torch.no_grad():
        _, again = model.track_step(feed[i + 1], npcs_feed[i + 1], {k: v.clone() for k, v in state.items()})
    assert set(again) == set(POSE_KEYS) | {"box_hist"}
    for k in POSE_KEYS:
        _same_bits(again[k], pred["poses"][i + 1][k], f"step {i + 1} again {k}")
    assert torch.equal(again["box_hist"], spy.calls[i]["new"])
    # the pickles and the eval CLI's table
    files = sorted((tmp_path / "results" / "data").glob("*.pkl"))
    assert len(files) == B
    lines = []
    for f in files:
        with open(f, "rb") as fh:
            saved = pickle.load(fh)
        assert set(saved) == {"pred", "gt", "frame_nums", "box"} and saved["box"][0] is None and len(saved["box"]) == T
        assert all(set(r) == set(REC_KEYS) for r in saved["box"][1:]) and all(set(p) == set(POSE_KEYS) for p in saved["pred"]["poses"])
        assert saved["box"][1]["extent"].shape == (P, 3) and saved["box"][1]["extent"].dtype == np.float32
        lines += ev.box_table(f.name.rsplit(".", 1)[0], saved)
    assert len(lines) == B * P and all("half-extents" in line and "established at frame" in line for line in lines)
    capsys.readouterr()
    ev.main(["--obj_category", str(cfg["obj_category"]), "--obj_config", cfg["obj_config"], "--experiment_dir", str(tmp_path)])
    printed = capsys.readouterr().out
    assert "track_cfg/box" in printed and all(line in printed for line in lines)


# ============================================================================================================== 2. the captured step
@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["bottle", "drawers"])
def test_hipgraph_gives_the_eager_bits(device, tag):
    from captra_amd.graph import TrackStepGraph
    _, _, data, eager, _ = _run(device, tag, box=_box(tag))
    gmodel, _, _, graph, _ = _run(device, tag, hipgraph=True, box=_box(tag))
    assert isinstance(gmodel._graph, TrackStepGraph) and set(gmodel._graph.pose) == set(POSE_KEYS) | {"box_hist"}
    _same_run(eager, graph, len(data), f"hipgraph {tag}")
    T = len(data)
    assert int(graph["box"][T - 1]["total"].sum()) == sum(int(graph["box"][i]["added"].sum()) for i in range(1, T)) > 0


# ======================================================================================================================= 3. two lanes
def _manual_loop(model, data, form):
    """'eager' = track_step on each half of the batch with its b0, 'lanes' = graph.TrackLanes of two.
    -> [(travelling pose dict, record)] of frames 1.., batch-wide."""
    import torch
    from captra_amd import graph as G
    model.set_data(data)
    feed = model.feed_dict
    pose = {k: v.clone() for k, v in feed[0]["gt_part"].items()}
    B = len(feed[1]["points"])
    halves = [slice(0, B // 2), slice(B // 2, B)]
    out = []
    with torch.no_grad():
        if form == "lanes":
            lanes = G.TrackLanes(model, feed[1]["points"], feed[1]["points_mean"], pose, lanes=2, keep_npcs=True)
        for i in range(1, len(feed)):
            pts, mean = feed[i]["points"], feed[i]["points_mean"]
            if form == "lanes":
                pose, npcs = lanes.gather(lanes.step(pts, mean, sync_inputs=True), npcs=True)
            else:
                parts = [model.track_step(*G.step_inputs(pts[s].contiguous(), mean[s].contiguous(), b0=s.start),
                                          {k: v[s].contiguous() for k, v in pose.items()}, allow_split_k=False) for s in halves]
                pose = {k: torch.cat([p[1][k] for p in parts]) for k in parts[0][1]}
                npcs = {k: torch.cat([p[0][k] for p in parts]) for k in parts[0][0] if torch.is_tensor(parts[0][0][k])}
            pose = {k: v.clone() for k, v in pose.items()}
            out.append((pose, {k: npcs["box_" + k].clone() for k in REC_KEYS}))
    torch.cuda.synchronize()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["bottle", "drawers"])
def test_two_lanes_give_the_halves_bits(device, tag):
    import torch
    trainer, cfg, data = _model(device, tag, box=_box(tag))
    model = trainer.model
    with _Spy() as spy:
        eager = _manual_loop(model, data, "eager")
    assert len(spy.calls) == 2 * (len(data) - 1)
    lanes = _manual_loop(model, data, "lanes")
    total = 0
    for i, ((pa, ra), (pb, rb)) in enumerate(zip(eager, lanes)):
        assert set(pa) == set(pb) == set(POSE_KEYS) | {"box_hist"}
        for k in pa:
            _same_bits(pb[k], pa[k], f"lanes frame {i + 1} {k}")
        for k in ra:
            _same_bits(rb[k], ra[k], f"lanes frame {i + 1} record {k}")
        total += int(ra["added"].sum())
        # the travelling histograms are what the record counts: once per frame
        assert torch.equal(pb["box_hist"][:, :, 0].sum(-1).int(), rb["total"]) and int(rb["total"].sum()) == total
    assert total > 0


# ============================================================================================================ 4. the on-the-fly re-crop
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["deferred", "every_frame_rare", "lanes_every_frame_rare"])
def test_otf_loop_deferred_equals_synchronous(device, mode, monkeypatch):
    """The sync-free re-crop (deferred verdicts; with a bound every frame outgrows: every frame run again from the dict that entered
    it, histograms included) against the synchronous stage from the same start, bit for bit: a replayed frame is counted once."""
    import torch
    import captra_amd.model as M
    from captra_amd.configs import make_config
    from captra_amd.synthetic import OTF_LOOP_SETUPS, make_otf_trajectory, make_physical_state_dict
    from captra_amd.trainer import Trainer
    from tests.test_otf import _cat_trajectories
    lanes = mode.startswith("lanes")
    if mode.endswith("rare"):
        monkeypatch.setattr(M, "_otf_bound", lambda longest, n: n)
        monkeypatch.setattr(M, "OTF_FIRST_BOUND", 1)
    setups = [OTF_LOOP_SETUPS[t] for t in ("a", "b")]
    frames, wseed = setups[0][0], setups[0][2]
    cfg = make_config("1", experiment_dir="/tmp/captra_otf_box_test", nocs_otf=True, hipgraph=True)
    cfg["device"] = device
    cfg["init_frame"]["gt"] = True
    cfg["track_cfg"]["box"] = _box("bottle")
    trainer = Trainer(cfg)
    model = trainer.model
    model.load_state_dict(make_physical_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, wseed, 1, True, "nocs"))
    reps = 16 if lanes else 1

    def make():
        if not lanes:
            return make_otf_trajectory(1, frames, seed=setups[0][1])
        return _cat_trajectories([make_otf_trajectory(1, frames, seed=s[1]) for s in setups for _ in range(reps)])

    model.otf_lanes = lanes
    torch.manual_seed(setups[0][3]); np.random.seed(setups[0][3])
    pred, _ = trainer.test(make(), save=False, no_eval=True)
    clouds = [model.feed_dict[i]["points"].clone() for i in range(1, frames)]
    monkeypatch.setattr(M, "OTF_DEFER", False)
    torch.manual_seed(setups[0][3]); np.random.seed(setups[0][3])
    pred2, _ = trainer.test(make(), save=False, no_eval=True)
    for i in range(1, frames):
        assert torch.equal(clouds[i - 1], model.feed_dict[i]["points"]), f"cloud of frame {i}"
    _same_run(pred, pred2, frames, mode)
    added = sum(pred["box"][i]["added"].long() for i in range(1, frames))
    assert torch.equal(pred["box"][frames - 1]["total"].long(), added) and int(added.min()) > 0
    assert bool((pred["box"][frames - 1]["extent"] > 0).all())


# ======================================================================================================================= 5. the guard
@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["bottle", "drawers"])
def test_a_lost_frame_leaves_the_state(device, tag):
    """The guard's verdict goes into the launch: a step under a guard nothing passes (every part with enough members is `lost`) leaves
    the histograms as they entered, while its own record is still written; under the lenient guard the frame counts."""
    import torch
    guard = {"refit": False, "lost_below": 0.0}                       # an inlier fraction below 0: never lost
    trainer, cfg, data = _model(device, tag, box=_box(tag), guard=guard)
    model = trainer.model
    model.set_data(data)
    feed, npcs_feed = model.feed_dict, model.npcs_feed_dict
    pose0 = {k: v.clone() for k, v in feed[0]["gt_part"].items()}
    with torch.no_grad(), _Spy() as spy:
        npcs1, pose1 = model.track_step(feed[1], npcs_feed[1], pose0)
        pose1 = {k: v.clone() for k, v in pose1.items()}
        verdict1 = npcs1["guard_verdict"].clone()
        lenient = model.guard
        model.guard = {**lenient, "lost_below": (1, 1), "inlier_th": 1e-12}          # every inlier fraction is below 1: lost
        npcs2, pose2 = model.track_step(feed[2], npcs_feed[2], {k: v.clone() for k, v in pose1.items()})
        model.guard = lenient
        npcs3, pose3 = model.track_step(feed[2], npcs_feed[2], {k: v.clone() for k, v in pose1.items()})
    assert len(spy.calls) == 3 and all(torch.equal(c["verdict"], n["guard_verdict"]) for c, n in zip(spy.calls, (npcs1, npcs2, npcs3)))
    for call in spy.calls:
        _judge_call(call)
    v2, v3 = npcs2["guard_verdict"], npcs3["guard_verdict"]
    assert bool((verdict1 == 0).any()) and bool((v2 == 2).any()) and not bool(((v2 == 0) | (v2 == 3)).any()) and bool((v3 == 0).any())
    assert pose1["box_hist"].any() and torch.equal(pose2["box_hist"], pose1["box_hist"])
    _same_bits(npcs2["box_extent"], npcs1["box_extent"], "the held extent of a lost frame")
    _same_bits(npcs2["box_total"], npcs1["box_total"], "the held count of a lost frame")
    assert bool((npcs2["box_added"] > 0).any()) and torch.equal(npcs2["box_added"], npcs3["box_added"])
    ok = v3 == 0
    assert torch.equal(npcs3["box_total"][ok], (npcs1["box_total"] + npcs3["box_added"])[ok])
    assert torch.equal(pose3["box_hist"][~ok], pose1["box_hist"][~ok])


# ============================================================================================== 6. the size and the motion option beside it
MOTION = {"predict": True, "max_angle": 30, "max_shift": 0.2}
SIZE = {"hold": True, "max_ratio": 2.0, "min_frames": 1}


@pytest.mark.gpu
def test_size_and_motion_keep_their_records(device):
    import torch
    _, _, data, alone, _ = _run(device, "bottle", hipgraph=True, motion=MOTION, size=SIZE)
    model, _, _, both, _ = _run(device, "bottle", hipgraph=True, motion=MOTION, size=SIZE, box=_box("bottle"))
    _, _, _, box_only, _ = _run(device, "bottle", hipgraph=True, box=_box("bottle"))
    T = len(data)
    assert set(alone) == {"poses", "npcs_pred", "motion", "size"} and set(both) == {"poses", "npcs_pred", "motion", "size", "box"}
    _same_run(alone, both, T, "size and motion beside the box", records=("motion", "size"))
    assert set(model._graph.pose) == set(POSE_KEYS) | {"next_rotation", "next_translation", "measured", "size_mean", "size_n", "size_miss", "box_hist"}
    # the box reads NOCS coordinates and labels only: the other options change the pose the NEXT frame is canonicalised with, and
    # through it the maps, so only frame 1's record is that of the run with the box alone
    for k in REC_KEYS:
        _same_bits(both["box"][1][k], box_only["box"][1][k], f"frame 1 box {k}")
    assert int(both["box"][T - 1]["total"].sum()) == sum(int(both["box"][i]["added"].sum()) for i in range(1, T))
    # the travelling dict carries every option's keys through the eager step too
    feed, npcs_feed = model.feed_dict, model.npcs_feed_dict
    with torch.no_grad():
        _, pose = model.track_step(feed[1], npcs_feed[1], {k: v.clone() for k, v in both["poses"][0].items()})
    assert set(pose) == set(model._graph.pose)
    assert torch.equal(pose["box_hist"][:, :, 0].sum(-1).int(), both["box"][1]["total"])


# ============================================================================================= 7. the boxes of the pickle and of the IoUs
@pytest.mark.gpu
def test_corners_and_ious_use_the_held_box(device, tmp_path, monkeypatch):
    """min_points above one frame's members: after frame 1 nothing is established (the reference's corners), from frame 2 on the held box.
    pred['corners'] and the boxes both IoU paths evaluate are held_box_corners of the reference's corners and the record's extent."""
    import torch
    from captra_amd.loss import choose_coord_by_label
    from captra_amd.pose_utils import bbox_utils as BU
    seen = {"host": [], "device": []}
    real_host, real_dev = BU.eval_single_part_iou, BU.eval_single_part_iou_device

    def host(gt_corners, pred_corners, *a, **kw):
        seen["host"].append(pred_corners.clone())
        return real_host(gt_corners, pred_corners, *a, **kw)

    def dev(gt_corners, pred_corners, *a, **kw):
        seen["device"].append(pred_corners.clone())
        return real_dev(gt_corners, pred_corners, *a, **kw)

    monkeypatch.setattr(BU, "eval_single_part_iou", host)
    monkeypatch.setattr(BU, "eval_single_part_iou_device", dev)
    B, T = SHAPES["bottle"]
    # (the box changes no pose, so a first run tells how many members a frame has; the box's own run needs more than frame 1 has)
    _, _, _, probe, _ = _run(device, "bottle", box=_box("bottle"))
    min_points = int(probe["box"][1]["added"].max()) + 1
    model, cfg, data, pred, loss = _run(device, "bottle", save=True, no_eval=False, experiment_dir=tmp_path, box=_box("bottle", min_points=min_points))
    assert not model.eval_device and len(seen["host"]) == T - 1 and not seen["device"]
    established = [(pred["box"][i]["extent"] > 0).all(-1).cpu().numpy() for i in range(1, T)]              # (B,P) per frame
    assert not established[0].any() and established[-1].any(), [pred["box"][i]["total"].tolist() for i in range(1, T)]
    want = []
    for i in range(1, T):
        npcs = pred["npcs_pred"][i]
        labels = torch.max(npcs["seg"], dim=-2)[1]
        ref = BU.get_pred_nocs_corners(labels, choose_coord_by_label(npcs["nocs"].transpose(-1, -2), labels), model.num_parts)     # (B,P,2,3) float64
        e = pred["box"][i]["extent"].cpu().numpy().astype(np.float64)
        est = established[i - 1]
        want.append(np.where(est[..., None, None], np.stack([-e, e], axis=-2), ref))
        assert (np.abs(want[-1] - ref).max(axis=(-1, -2)) > 0)[est].all()       # (the held box is another box than the frame's maximum)
        np.testing.assert_array_equal(seen["host"][i - 1].numpy(), want[-1].astype(np.float32), err_msg=f"host IoU boxes of frame {i}")
    files = sorted((tmp_path / "results" / "data").glob("*.pkl"))
    assert len(files) == B
    for b, f in enumerate(files):
        with open(f, "rb") as fh:
            saved = pickle.load(fh)
        corners = saved["pred"]["corners"]
        assert corners[0] is None and len(corners) == T
        for i in range(1, T):
            assert corners[i].dtype == np.float64
            np.testing.assert_array_equal(corners[i], want[i - 1][b], err_msg=f"{f.name} corners of frame {i}")
    # the device path on the same run: the same boxes, IoUs within the tolerance of tests/test_iou_gpu.py
    model.eval_device = True
    model.compute_loss(test=True, per_instance=False, eval_iou=True, test_prefix="test")
    assert len(seen["device"]) == 1
    np.testing.assert_array_equal(seen["device"][0].cpu().numpy(), np.stack(want).astype(np.float32))
    for i in range(1, T):
        for name in ("npcs_iou", "iou", "gt_bbox_iou"):
            for p, v in loss["frame_iou"][i][name].items():
                got = model.loss_dict["frame_iou"][i][name][p]
                print("frame", i, name, p, "host", v, "device", got)
                assert abs(got - v) <= IOU_TOL, (i, name, p, v, got)
    # and the pickle's corners with the device path writing them
    model._save([["0", "0"]] * T)
    for b, f in enumerate(files):
        with open(f, "rb") as fh:
            again = pickle.load(fh)["pred"]["corners"]
        for i in range(1, T):
            np.testing.assert_array_equal(again[i], want[i - 1][b], err_msg=f"{f.name} device corners of frame {i}")


# =================================================================================================================== 8. option absent
@pytest.mark.gpu
def test_off_changes_nothing(device, tmp_path, monkeypatch):
    import torch
    from captra_amd import _lib
    from captra_amd.graph import TrackStepGraph
    calls, real = [], _lib.call

    def counting(name, *args):
        calls.append(name)
        return real(name, *args)

    monkeypatch.setattr(_lib, "call", counting)
    runs, corners = {}, {}
    for name, box in (("absent", None), ("false", {"hold": False, "quantile": 0.95})):
        with _Spy() as spy:
            model, cfg, data, pred, _ = _run(device, "bottle", save=True, hipgraph=True, experiment_dir=tmp_path / name, box=box)
        assert model.box is None and not spy.calls
        assert set(pred) == {"poses", "npcs_pred"} and all(set(p) == set(POSE_KEYS) for p in pred["poses"])
        assert not any(k.startswith("box_") for n in pred["npcs_pred"][1:] for k in n)
        assert isinstance(model._graph, TrackStepGraph) and set(model._graph.pose) == set(POSE_KEYS)
        with torch.no_grad():
            _, pose = model.track_step(model.feed_dict[1], model.npcs_feed_dict[1], {k: v.clone() for k, v in pred["poses"][0].items()})
        assert set(pose) == set(POSE_KEYS)
        files = sorted((tmp_path / name / "results" / "data").glob("*.pkl"))
        assert len(files) == 4
        saved = []
        for f in files:
            with open(f, "rb") as fh:
                saved.append(pickle.load(fh))
            assert set(saved[-1]) == {"pred", "gt", "frame_nums"}
        runs[name], corners[name] = pred, [s["pred"]["corners"] for s in saved]
    assert calls and "captra_part_box_hist" not in calls
    for a, b in zip(runs["absent"]["poses"], runs["false"]["poses"]):
        for k in a:
            _same_bits(a[k], b[k], k)
    # the pickle's corners are the reference's per-frame maximum, as before
    from captra_amd.loss import choose_coord_by_label
    from captra_amd.pose_utils.bbox_utils import get_pred_nocs_corners
    pred = runs["absent"]
    for i in range(1, len(pred["poses"])):
        labels = torch.max(pred["npcs_pred"][i]["seg"], dim=-2)[1]
        ref = get_pred_nocs_corners(labels, choose_coord_by_label(pred["npcs_pred"][i]["nocs"].transpose(-1, -2), labels), 1)
        for b in range(4):
            np.testing.assert_array_equal(corners["absent"][b][i], ref[b])
            np.testing.assert_array_equal(corners["false"][b][i], ref[b])
    # the positive control: the same spy sees the call when the option is on
    calls.clear()
    _run(device, "bottle", box=_box("bottle"))
    assert calls.count("captra_part_box_hist") == SHAPES["bottle"][1] - 1
