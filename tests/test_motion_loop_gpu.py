"""The motion model inside the track loop (track_cfg: {motion: {predict: True, ...}}) on the synthetic trajectories: the one launch
per step and what it reads, the travelling pose dict as the loop's whole state, the captured step, the lanes, the on-the-fly re-crop
in its deferred and replayed forms, the guard's verdicts, and the option switched off."""
import pickle

import numpy as np
import pytest

MOTION = {"predict": True, "max_angle": 30, "max_shift": 0.2}          # generous thresholds; a test setting only
REC_KEYS = ("used", "angle", "shift", "rotation", "translation")
POSE_KEYS = ("rotation", "scale", "translation")
SHAPES = {"bottle": (4, 5), "drawers": (2, 4)}                           # tag -> (B, T)


def _model(device, tag, motion, guard=None, hipgraph=False, experiment_dir="/tmp/captra_test_exp"):
    from captra_amd import synthetic as clouds
    from captra_amd.configs import make_config
    from captra_amd.trainer import Trainer
    cat, objcfg, kind, _, _, wseed, _ = clouds.PHYSICAL_SETUPS[tag]
    cfg = make_config(cat, objcfg, experiment_dir=str(experiment_dir))
    for key, val in (("motion", motion), ("guard", guard)):
        if val is not None:
            cfg["track_cfg"][key] = dict(val)
    cfg["hipgraph"] = hipgraph
    cfg["init_frame"]["gt"] = True
    trainer = Trainer(cfg)
    shapes = {k: tuple(v.shape) for k, v in trainer.model.state_dict().items()}
    trainer.model.load_state_dict(clouds.make_physical_state_dict(shapes, wseed, cfg["num_parts"], bool(cfg["obj_sym"]), kind))
    B, T = SHAPES[tag]
    return trainer, cfg, clouds.make_trajectory(kind, B, T, seed=7)


def _run(device, tag, motion, save=False, **kw):
    import torch
    trainer, cfg, data = _model(device, tag, motion, **kw)
    torch.manual_seed(4321)
    pred, _ = trainer.test(data, save=save, no_eval=True)
    return trainer.model, cfg, data, pred


class _Spy:
    """Around pose_fit.pose_extrapolate: every call's arguments (cloned) and results."""

    def __init__(self):
        from captra_amd.pose_utils import pose_fit
        self.mod, self.real, self.calls = pose_fit, pose_fit.pose_extrapolate, []

    def __enter__(self):
        def spy(rot0, trans0, rot1, trans1, measured0, sym, max_angle, max_shift, gain=1.0, verdict=None):
            res = self.real(rot0, trans0, rot1, trans1, measured0, sym, max_angle, max_shift, gain=gain, verdict=verdict)
            self.calls.append(dict(rot0=rot0.clone(), trans0=trans0.clone(), rot1=rot1.clone(), trans1=trans1.clone(), measured0=measured0.clone(),
                                   sym=sym, max_angle=max_angle, max_shift=max_shift, gain=gain, verdict=None if verdict is None else verdict.clone(),
                                   rot_next=res[0].clone(), trans_next=res[1].clone(), measured1=res[2].clone(),
                                   info={k: v.clone() for k, v in res[3].items()}))
            return res
        self.mod.pose_extrapolate = spy
        return self

    def __exit__(self, *a):
        self.mod.pose_extrapolate = self.real


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a.cpu().numpy()), np.ascontiguousarray(b.cpu().numpy())
    assert a.dtype == b.dtype and a.shape == b.shape, what
    np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32), err_msg=str(what))


def _same_run(a, b, frames, what):
    for i in range(1, frames):
        assert set(a["poses"][i]) == set(b["poses"][i]) == set(POSE_KEYS)
        for k in POSE_KEYS:
            _same_bits(a["poses"][i][k], b["poses"][i][k], f"{what} frame {i} {k}")
        for k in REC_KEYS:
            _same_bits(a["motion"][i][k], b["motion"][i][k], f"{what} frame {i} record {k}")


# ================================================================================================= 1. one launch per step, one state
@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["bottle", "drawers"])
def test_one_call_per_step_and_the_dict_is_the_state(device, tag, tmp_path):
    import torch
    with _Spy() as spy:
        model, cfg, data, pred = _run(device, tag, MOTION, save=True, experiment_dir=tmp_path)
    T = len(data)
    B, P = pred["poses"][0]["scale"].shape
    assert model.motion == {"max_angle": 30.0, "max_shift": 0.2 * float(cfg["data_radius"]), "gain": 1.0}
    assert set(pred) == {"poses", "npcs_pred", "motion"} and len(pred["motion"]) == T and pred["motion"][0] is None
    assert len(spy.calls) == T - 1
    for i in range(1, T):
        call, rec, pose = spy.calls[i - 1], pred["motion"][i], pred["poses"][i]
        assert set(pose) == set(POSE_KEYS) and set(rec) == set(REC_KEYS)
        assert not any(k.startswith("motion_") for k in pred["npcs_pred"][i])
        assert call["sym"] == bool(cfg["obj_sym"]) and call["verdict"] is None
        assert (call["max_angle"], call["max_shift"], call["gain"]) == (30.0, model.motion["max_shift"], 1.0)
        _same_bits(call["rot0"], pred["poses"][i - 1]["rotation"], f"frame {i} rot0")
        _same_bits(call["trans0"], pred["poses"][i - 1]["translation"], f"frame {i} trans0")
        _same_bits(call["rot1"], pose["rotation"], f"frame {i} rot1")
        _same_bits(call["trans1"], pose["translation"], f"frame {i} trans1")
        prev_measured = torch.zeros(B, P, dtype=torch.int32, device=call["measured0"].device) if i == 1 else spy.calls[i - 2]["measured1"]
        assert torch.equal(call["measured0"], prev_measured), f"frame {i} measured0"
        for k, v in (("rotation", call["rot_next"]), ("translation", call["trans_next"])) + tuple(call["info"].items()):
            assert rec[k].shape == v.shape and rec[k].dtype == v.dtype
            _same_bits(rec[k], v, f"frame {i} record {k}")
        assert rec["used"].dtype == torch.int32 and rec["used"].shape == (B, P) and rec["translation"].shape == (B, P, 3, 1)
        print(tag, "frame", i, "used", rec["used"].cpu().numpy().tolist(), "angle", rec["angle"].cpu().numpy().round(3).tolist(),
              "shift", rec["shift"].cpu().numpy().round(4).tolist())
    assert not pred["motion"][1]["used"].any()                      # the first pose is no motion sample: frame 1 never extrapolates
    for i in range(2, T):                                           # (no part predicted: a broken fixture, not a skip)
        assert pred["motion"][i]["used"].any(), f"frame {i}: no part was predicted"
    # the dict a step returns is the whole state: the step on it again gives the loop's bits; with the prediction overwritten by the
    # result -- the parent's start pose -- every predicted part comes out different
    feed, npcs_feed = model.feed_dict, model.npcs_feed_dict
    for i in range(1, T - 1):
        call = spy.calls[i - 1]
        state = {**pred["poses"][i], "next_rotation": call["rot_next"], "next_translation": call["trans_next"], "measured": call["measured1"]}
        with torch.no_grad():
            _, again = model.track_step(feed[i + 1], npcs_feed[i + 1], {k: v.clone() for k, v in state.items()})
            again = {k: v.clone() for k, v in again.items()}
            plain = {**state, "next_rotation": state["rotation"], "next_translation": state["translation"]}
            _, other = model.track_step(feed[i + 1], npcs_feed[i + 1], {k: v.clone() for k, v in plain.items()})
        assert set(again) == set(POSE_KEYS) | {"next_rotation", "next_translation", "measured"}
        for k in POSE_KEYS:
            _same_bits(again[k], pred["poses"][i + 1][k], f"step {i + 1} again {k}")
        _same_bits(again["next_rotation"], pred["motion"][i + 1]["rotation"], f"step {i + 1} again next_rotation")
        _same_bits(again["next_translation"], pred["motion"][i + 1]["translation"], f"step {i + 1} again next_translation")
        used = call["info"]["used"].bool()
        differs = (other["rotation"] != pred["poses"][i + 1]["rotation"]).flatten(2).any(-1) | \
                  (other["translation"] != pred["poses"][i + 1]["translation"]).flatten(2).any(-1)
        assert bool(differs[used].all()), (i, differs.cpu().numpy().tolist(), used.cpu().numpy().tolist())
    # the pickles: the record beside the parent's entries, poses with their three keys
    files = sorted((tmp_path / "results" / "data").glob("*.pkl"))
    assert len(files) == B
    with open(files[0], "rb") as f:
        saved = pickle.load(f)
    assert set(saved) == {"pred", "gt", "frame_nums", "motion"} and saved["motion"][0] is None and len(saved["motion"]) == T
    assert all(set(r) == set(REC_KEYS) for r in saved["motion"][1:]) and all(set(p) == set(POSE_KEYS) for p in saved["pred"]["poses"])


# ============================================================================================================== 2. the captured step
@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["bottle", "drawers"])
def test_hipgraph_gives_the_eager_bits(device, tag):
    from captra_amd.graph import TrackStepGraph
    _, _, data, eager = _run(device, tag, MOTION)
    gmodel, _, _, graph = _run(device, tag, MOTION, hipgraph=True)
    assert isinstance(gmodel._graph, TrackStepGraph) and set(gmodel._graph.pose) == set(POSE_KEYS) | {"next_rotation", "next_translation", "measured"}
    _same_run(eager, graph, len(data), f"hipgraph {tag}")


# ======================================================================================================================= 3. two lanes
def _manual_loop(model, data, form):
    """As in tests/test_rot_consensus_gpu.py: 'eager' = track_step on each half of the batch with its b0, 'lanes' = graph.TrackLanes of
    two.  -> [(travelling pose dict, record)] of frames 1.., batch-wide."""
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
            out.append((pose, {k: npcs["motion_" + k].clone() for k in REC_KEYS}))
    torch.cuda.synchronize()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["bottle", "drawers"])
def test_two_lanes_give_the_halves_bits(device, tag):
    trainer, cfg, data = _model(device, tag, MOTION)
    model = trainer.model
    with _Spy() as spy:
        eager = _manual_loop(model, data, "eager")
    assert len(spy.calls) == 2 * (len(data) - 1)
    lanes = _manual_loop(model, data, "lanes")
    used = 0
    for i, ((pa, ra), (pb, rb)) in enumerate(zip(eager, lanes)):
        assert set(pa) == set(pb) == set(POSE_KEYS) | {"next_rotation", "next_translation", "measured"}
        for k in pa:
            _same_bits(pb[k], pa[k], f"lanes frame {i + 1} {k}")
        for k in ra:
            _same_bits(rb[k], ra[k], f"lanes frame {i + 1} record {k}")
        _same_bits(pa["next_rotation"], ra["rotation"], f"frame {i + 1}: the record is the prediction")
        used += int(ra["used"].sum())
    assert used > 0


# ============================================================================================================ 4. the on-the-fly re-crop
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["deferred", "lanes_deferred", "every_frame_rare", "lanes_every_frame_rare"])
def test_otf_loop_follows_the_prediction(device, mode, monkeypatch):
    """The sync-free re-crop (deferred verdicts; with a bound every frame outgrows: every frame run again from the dict that entered
    it) against the synchronous stage from the same start, bit for bit with the option on, single batch and two lanes; and the crop's
    centre is the previous step's prediction."""
    import torch
    import captra_amd.model as M
    from captra_amd import nocs_otf
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
    cfg = make_config("1", experiment_dir="/tmp/captra_otf_motion_test", nocs_otf=True, hipgraph=True)
    cfg["device"] = device
    cfg["init_frame"]["gt"] = True
    cfg["track_cfg"]["motion"] = dict(MOTION)
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
    # the synchronous stage from the same start, its crop centres recorded
    monkeypatch.setattr(M, "OTF_DEFER", False)
    centres, real = [], nocs_otf.full_data_batch_arrays

    def spy(*a, **kw):
        if kw.get("pose_dev") is not None:
            centres.append(kw["pose_dev"][0].clone())
        return real(*a, **kw)
    monkeypatch.setattr(nocs_otf, "full_data_batch_arrays", spy)
    torch.manual_seed(setups[0][3]); np.random.seed(setups[0][3])
    pred2, _ = trainer.test(make(), save=False, no_eval=True)
    for i in range(1, frames):
        assert torch.equal(clouds[i - 1], model.feed_dict[i]["points"]), f"cloud of frame {i}"
    _same_run(pred, pred2, frames, mode)
    assert sum(int(pred["motion"][i]["used"].sum()) for i in range(2, frames)) > 0
    per = 2 if lanes else 1
    assert len(centres) == per * (frames - 1)
    B = pred["poses"][0]["scale"].shape[0]
    moved = False
    for i in range(1, frames):
        got = torch.cat(centres[per * (i - 1):per * i]).reshape(B, 3)
        want = (pred2["poses"][0]["translation"] if i == 1 else pred2["motion"][i - 1]["translation"])[:, model.root].reshape(B, 3)
        _same_bits(got, want, f"crop centre of frame {i}")
        moved = moved or not torch.equal(got, pred2["poses"][i - 1]["translation"][:, model.root].reshape(B, 3))
    assert moved                                                     # (somewhere the crop followed a prediction, not the last result)


# ============================================================================================================ 5. the guard's verdicts
# lost_below 1.0: a part with one outlier is lost -- every frame's verdict is 2 (monitoring) or 3 where the re-fit is accepted; the
# lenient guard (a test setting: 3 cm at the crops' 0.6 m, lost below 5 %) is the same loop with verdicts that are mostly ok
GUARDS = {"lost": {"refit": False, "lost_below": 1.0}, "refit": {"refit": True, "lost_below": 1.0},
          "lenient": {"refit": False, "lost_below": 0.05, "inlier_th": 0.05}}


@pytest.mark.gpu
@pytest.mark.parametrize("which", list(GUARDS))
@pytest.mark.parametrize("tag", ["bottle", "drawers"])
def test_guard_verdicts_gate_the_prediction(device, tag, which):
    import torch
    guard = GUARDS[which]
    with _Spy() as spy:
        model, cfg, data, pred = _run(device, tag, MOTION, guard=guard)
    assert set(pred) == {"poses", "npcs_pred", "motion", "guard"} and len(spy.calls) == len(data) - 1
    seen = set()
    for i in range(1, len(data)):
        verdict, used = pred["guard"][i]["verdict"], pred["motion"][i]["used"]
        assert torch.equal(spy.calls[i - 1]["verdict"], verdict)
        assert not used[verdict != 0].any(), f"frame {i}"
        if i > 1:
            before = pred["guard"][i - 1]["verdict"]
            assert not used[(before == 1) | (before == 2)].any(), f"frame {i}: predicted from a pose that was no measurement"
            assert torch.equal(spy.calls[i - 1]["measured0"], ((before == 0) | (before == 3)).int())
        seen.update(verdict.flatten().tolist())
        print(tag, "frame", i, "verdict", verdict.cpu().numpy().tolist(), "used", used.cpu().numpy().tolist())
    if which == "lenient":          # (a guard that finds the parts ok lets the loop predict: a fixture without is broken)
        assert 0 in seen and any(bool(pred["motion"][i]["used"].any()) for i in range(2, len(data)))
    else:
        assert seen - {0}, "the fixture met no verdict but ok"


# =================================================================================================================== 6. option absent
@pytest.mark.gpu
def test_off_changes_nothing(device):
    runs = {}
    for name, motion in (("absent", None), ("false", {"predict": False, "max_angle": 30, "max_shift": 0.2})):
        with _Spy() as spy:
            model, cfg, data, pred = _run(device, "bottle", motion)
        assert model.motion is None and not spy.calls
        assert set(pred) == {"poses", "npcs_pred"}
        assert all(set(p) == set(POSE_KEYS) for p in pred["poses"])
        assert not any(k.startswith("motion_") for n in pred["npcs_pred"][1:] for k in n)
        runs[name] = pred
    for a, b in zip(runs["absent"]["poses"], runs["false"]["poses"]):
        for k in a:
            _same_bits(a[k], b[k], k)
