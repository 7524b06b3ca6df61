"""Holding the track's size inside the track loop (track_cfg: {size: {hold: True, ...}}) on the synthetic trajectories: the one
launch per step and what it reads, the size state in the travelling pose dict as the loop's whole state, plain and robust mode, the
captured step, the lanes, the on-the-fly re-crop in its deferred and replayed forms, the guard, the motion model beside it, and the
option switched off.  Nothing here asserts that holding the size improves accuracy: tools/bench_size.py measures that."""
import pickle

import numpy as np
import pytest

from tests import size_judge as ZJ

MAX_RATIO = 2.0                                                           # a generous gate; a test setting only
SIZE = {"hold": True, "max_ratio": MAX_RATIO, "min_frames": 1}
ALL_INLIERS = 10.0            # st_fit/inlier_th (a fraction of data_radius) under which every member is an inlier: the held robust fit is then E-given on all members
ROBUST = {"ransac": True, "inlier_th": ALL_INLIERS}
REC_KEYS = ("held", "accepted", "free", "n")
POSE_KEYS = ("rotation", "scale", "translation")
STATE_KEYS = ("size_mean", "size_n", "size_miss")
SHAPES = {"bottle": (4, 5), "drawers": (2, 4)}                            # tag -> (B, T)
F32_EPS = float(np.finfo(np.float32).eps)


def _model(device, tag, hipgraph=False, experiment_dir="/tmp/captra_test_exp", **track_cfg):
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
    trainer = Trainer(cfg)
    shapes = {k: tuple(v.shape) for k, v in trainer.model.state_dict().items()}
    trainer.model.load_state_dict(clouds.make_physical_state_dict(shapes, wseed, cfg["num_parts"], bool(cfg["obj_sym"]), kind))
    B, T = SHAPES[tag]
    return trainer, cfg, clouds.make_trajectory(kind, B, T, seed=7)


def _run(device, tag, save=False, **kw):
    import torch
    trainer, cfg, data = _model(device, tag, **kw)
    torch.manual_seed(4321)
    pred, _ = trainer.test(data, save=save, no_eval=True)
    return trainer.model, cfg, data, pred


class _Spy:
    """Around part_fit_st_size_track as PartCanonNet calls it: every call's arguments and results (cloned)."""

    def __init__(self):
        from captra_amd import networks
        self.mod, self.real, self.calls = networks, networks.part_fit_st_size_track, []

    def __enter__(self):
        import torch
        clone = lambda v: v.clone() if torch.is_tensor(v) else v          # noqa: E731

        def spy(labels, src, pts, mean, rot, prev_scale, prev_trans, sym, state, **kw):
            res = self.real(labels, src, pts, mean, rot, prev_scale, prev_trans, sym, state, **kw)
            free = kw.get("free")
            self.calls.append(dict(labels=labels.clone(), src=src.clone(), pts=pts.clone(), mean=mean.clone(), rot=rot.clone(), sym=sym,
                                   prev_scale=prev_scale.clone(), prev_trans=prev_trans.clone(), state={k: v.clone() for k, v in state.items()},
                                   kw={k: clone(v) for k, v in kw.items() if k != "free"}, free=None if free is None else tuple(f.clone() for f in free),
                                   pose={k: v.clone() for k, v in res[0].items()}, new={k: v.clone() for k, v in res[1].items()},
                                   info={k: v.clone() for k, v in res[2].items()}))
            return res
        self.mod.part_fit_st_size_track = spy
        return self

    def __exit__(self, *a):
        self.mod.part_fit_st_size_track = self.real


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a.cpu().numpy()), np.ascontiguousarray(b.cpu().numpy())
    assert a.dtype == b.dtype and a.shape == b.shape, what
    np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32), err_msg=str(what))


def _same_run(a, b, frames, what, records=("size",)):
    for i in range(1, frames):
        assert set(a["poses"][i]) == set(b["poses"][i]) == set(POSE_KEYS)
        for k in POSE_KEYS:
            _same_bits(a["poses"][i][k], b["poses"][i][k], f"{what} frame {i} {k}")
        for name in records:
            for k in a[name][i]:
                _same_bits(a[name][i][k], b[name][i][k], f"{what} frame {i} {name} {k}")


def _replay_call(call, opts, tag):
    """The judge on one spied call: the decision from the state and the free fit as the kernel had them (exact; an averaged mean within
    1 fp32 ulp), and every held cell's translation against E-given on all members in float64 by the mirror rule."""
    n = lambda t: t.cpu().numpy()          # noqa: E731
    B, P = call["new"]["size_n"].shape
    info, new, pose = call["info"], call["new"], call["pose"]
    free = (n(info["free"]), n(info["free_translation"])[..., 0], n(info["free_valid"]))
    case = dict(labels=n(call["labels"]), src=n(call["src"]), tgt=n(call["pts"]), tgt_mean=n(call["mean"]).reshape(B, 3), rot=n(call["rot"]),
                sym=bool(call["sym"]), th=np.float32(1.0), ranks=np.zeros((B, P, 1, 3), np.int32))
    state = tuple(n(call["state"][k]) for k in STATE_KEYS)
    # (every member an inlier: robust mode's held fit is plain mode's)
    ref = ZJ.judge_batch(case, free, state, opts, False, given=n(new["size_mean"]))
    mir = ZJ.judge_batch(case, free, state, opts, False, dt=np.float32, given=n(new["size_mean"]))
    held_any = False
    for b in range(B):
        for p in range(P):
            d, what = ref["decision"][b, p], (tag, b, p)
            got = (int(new["size_n"][b, p]), int(new["size_miss"][b, p]), int(info["accepted"][b, p]), int(info["held"][b, p]))
            assert got == (d["n"], d["miss"], d["accepted"], d["held"]), (what, got, d)
            mean = float(new["size_mean"][b, p])
            assert (np.float32(mean) == d["mean32"]) if d["exact"] else abs(mean - d["mean"]) <= float(np.spacing(np.float32(abs(d["mean"])))), (what, mean, d)
            if not d["held"]:
                _same_bits(pose["scale"][b, p], info["free"][b, p], what)
                _same_bits(pose["translation"][b, p], info["free_translation"][b, p], what)
                assert bool(pose["valid"][b, p]) == bool(free[2][b, p])
                continue
            held_any = True
            _same_bits(pose["scale"][b, p], new["size_mean"][b, p], what)
            count = int((case["labels"][b] == p).sum())
            assert int(info["held_inliers"][b, p]) == (count if call["free"] is not None or count >= 3 else 0), what
            assert bool(pose["valid"][b, p]) == bool(ref["valid"][b, p]), what
            if not ref["valid"][b, p]:
                _same_bits(pose["translation"][b, p], info["free_translation"][b, p], what)
                continue
            t = n(pose["translation"][b, p])[:, 0]
            et, mt = np.abs(t - ref["trans"][b, p]).max(), np.abs(mir["trans"][b, p] - ref["trans"][b, p]).max()
            assert et <= max(2 * mt, 4 * F32_EPS * np.abs(ref["trans"][b, p]).max()), (what, et, mt)
    return held_any


# ============================================================================================== 1. min_frames beyond the trajectory
@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["bottle", "drawers"])
def test_never_held_is_the_option_off(device, tag):
    _, _, data, off = _run(device, tag)
    T = len(data)
    model, _, _, on = _run(device, tag, size={**SIZE, "min_frames": T + 1})
    assert model.size is not None and set(off) == {"poses", "npcs_pred"} and set(on) == {"poses", "npcs_pred", "size"}
    assert len(on["size"]) == T and on["size"][0] is None
    _same_run(off, on, T, f"never held {tag}", records=())
    for i in range(1, T):
        rec = on["size"][i]
        assert set(rec) == set(REC_KEYS) and not rec["held"].any()
        assert not any(k.startswith("size_") for k in on["npcs_pred"][i])
        _same_bits(rec["free"], on["poses"][i]["scale"], f"frame {i}: the free scale is the pose's")
    assert int(on["size"][T - 1]["n"].max()) == T - 1          # (every frame of some part went into its mean)


# ================================================================================================ 2. one call per step, one state
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["plain", "robust"])
@pytest.mark.parametrize("tag", ["bottle", "drawers"])
def test_one_call_per_step_and_the_dict_is_the_state(device, tag, mode, tmp_path, capsys):
    import torch
    from captra_amd import _lib
    from captra_amd import eval as ev
    st = ROBUST if mode == "robust" else None
    _lib.prof_enable(True)
    _lib.prof_reset()
    try:
        with _Spy() as spy:
            model, cfg, data, pred = _run(device, tag, save=True, experiment_dir=tmp_path, size=SIZE, st_fit=st)
        torch.cuda.synchronize()
        sfx = "_sym" if cfg["obj_sym"] else ""
        launches = {n: _lib.prof_read(n)[1] for n in ("part_fit_st", "part_fit_st_ransac" + sfx, "part_fit_st_size" + sfx, "part_fit_st_size_ransac" + sfx)}
    finally:
        _lib.prof_enable(False)
    T = len(data)
    # launches per run: robust mode REPLACES the robust fit's launch, plain mode follows the one-pass fit's
    assert launches == ({"part_fit_st": 0, "part_fit_st_ransac" + sfx: 0, "part_fit_st_size" + sfx: 0, "part_fit_st_size_ransac" + sfx: T - 1} if st else
                        {"part_fit_st": T - 1, "part_fit_st_ransac" + sfx: 0, "part_fit_st_size" + sfx: T - 1, "part_fit_st_size_ransac" + sfx: 0}), launches
    B, P = pred["poses"][0]["scale"].shape
    opts = {k: model.size[k] for k in ("min_frames", "max_ratio", "max_frames", "reset_after")}
    assert model.size == {"max_ratio": MAX_RATIO, "min_frames": 1, "max_frames": None, "reset_after": None, "init_frames": 0}
    assert set(pred) == {"poses", "npcs_pred", "size"} | ({"st_fit"} if st else set()) and len(spy.calls) == T - 1
    held_any = False
    for i in range(1, T):
        call, rec, pose, last = spy.calls[i - 1], pred["size"][i], pred["poses"][i], pred["poses"][i - 1]
        assert set(pose) == set(POSE_KEYS) and set(rec) == set(REC_KEYS) and (call["free"] is None) == (mode == "robust")
        # the state that enters a step is the one the step before left, bit for bit; a track starts empty
        if i == 1:
            assert not call["state"]["size_n"].any() and not call["state"]["size_miss"].any() and not call["state"]["size_mean"].any()
        else:
            for k in STATE_KEYS:
                _same_bits(call["state"][k], spy.calls[i - 2]["new"][k], f"frame {i} state {k}")
        _same_bits(call["prev_scale"], last["scale"], f"frame {i}: prev_scale is the pose's (held) scale")
        _same_bits(call["rot"], pose["rotation"], f"frame {i} rotation")
        held_any |= _replay_call(call, opts, (tag, mode, i))
        # the committed pose and the record are the call's
        held = call["info"]["held"].bool()
        _same_bits(pose["scale"], torch.where(held, call["new"]["size_mean"], call["info"]["free"]), f"frame {i} scale")
        _same_bits(pose["scale"], call["pose"]["scale"], f"frame {i} scale")
        _same_bits(pose["translation"], call["pose"]["translation"], f"frame {i} translation")
        for k in REC_KEYS:
            assert rec[k].shape == (B, P)
            _same_bits(rec[k], call["info"][k], f"frame {i} record {k}")
        assert rec["held"].dtype == torch.int32 and rec["free"].dtype == torch.float32 and torch.equal(rec["n"], call["new"]["size_n"])
        if st:
            # the robust fit's record is the FREE fit's
            assert torch.equal(pred["st_fit"][i]["valid"], call["info"]["free_valid"]) and torch.equal(pred["st_fit"][i]["inliers"], call["info"]["inliers"])
            assert call["kw"]["inlier_th"] == model.st_fit["inlier_th"] and call["kw"]["b0"] == 0
        print(tag, mode, "frame", i, "held", rec["held"].cpu().numpy().tolist(), "n", rec["n"].cpu().numpy().tolist(),
              "free", rec["free"].cpu().numpy().round(5).tolist(), "scale", pose["scale"].cpu().numpy().round(5).tolist())
    assert held_any and bool(pred["size"][T - 1]["held"].any())
    # the dict a step returns is the whole state: the step on it again gives the loop's bits
    feed, npcs_feed = model.feed_dict, model.npcs_feed_dict
    i = T - 2
    state = {**pred["poses"][i], **spy.calls[i - 1]["new"]}
    with torch.no_grad():
        _, again = model.track_step(feed[i + 1], npcs_feed[i + 1], {k: v.clone() for k, v in state.items()})
    assert set(again) == set(POSE_KEYS) | set(STATE_KEYS)
    for k in POSE_KEYS:
        _same_bits(again[k], pred["poses"][i + 1][k], f"step {i + 1} again {k}")
    for k in STATE_KEYS:
        _same_bits(again[k], spy.calls[i]["new"][k], f"step {i + 1} again {k}")
    # the pickles and the eval CLI's table
    files = sorted((tmp_path / "results" / "data").glob("*.pkl"))
    assert len(files) == B
    lines = []
    for f in files:
        with open(f, "rb") as fh:
            saved = pickle.load(fh)
        assert set(saved) == {"pred", "gt", "frame_nums", "size"} | ({"st_fit"} if st else set()) and saved["size"][0] is None and len(saved["size"]) == T
        assert all(set(r) == set(REC_KEYS) for r in saved["size"][1:]) and all(set(p) == set(POSE_KEYS) for p in saved["pred"]["poses"])
        lines += ev.size_table(f.name.rsplit(".", 1)[0], saved)
    assert len(lines) == B * P and all("held" in line and "final mean" in line for line in lines)
    capsys.readouterr()
    ev.main(["--obj_category", str(cfg["obj_category"]), "--obj_config", cfg["obj_config"], "--experiment_dir", str(tmp_path)])
    printed = capsys.readouterr().out
    assert "track_cfg/size" in printed and all(line in printed for line in lines)


# ============================================================================================================== 3. the captured step
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["plain", "robust"])
@pytest.mark.parametrize("tag", ["bottle", "drawers"])
def test_hipgraph_gives_the_eager_bits(device, tag, mode):
    from captra_amd.graph import TrackStepGraph
    st = {"ransac": True} if mode == "robust" else None
    _, _, data, eager = _run(device, tag, size=SIZE, st_fit=st)
    gmodel, _, _, graph = _run(device, tag, hipgraph=True, size=SIZE, st_fit=st)
    assert isinstance(gmodel._graph, TrackStepGraph) and set(gmodel._graph.pose) == set(POSE_KEYS) | set(STATE_KEYS)
    _same_run(eager, graph, len(data), f"hipgraph {tag} {mode}", records=("size", "st_fit") if st else ("size",))
    assert bool(eager["size"][len(data) - 1]["held"].any())


# ======================================================================================================================= 4. two lanes
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
            assert [g.b0 for g in lanes.graphs] == [0, B // 2]
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
            out.append((pose, {k: npcs["size_" + k].clone() for k in REC_KEYS}))
    torch.cuda.synchronize()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["bottle", "drawers"])
def test_two_lanes_give_the_halves_bits(device, tag):
    """Robust mode with the default inlier distance: the second lane's draws are keyed by its b0, for the free and the held fit alike."""
    trainer, cfg, data = _model(device, tag, size=SIZE, st_fit={"ransac": True})
    model = trainer.model
    with _Spy() as spy:
        eager = _manual_loop(model, data, "eager")
    assert len(spy.calls) == 2 * (len(data) - 1) and [c["kw"]["b0"] for c in spy.calls[:2]] == [0, SHAPES[tag][0] // 2]
    lanes = _manual_loop(model, data, "lanes")
    held = 0
    for i, ((pa, ra), (pb, rb)) in enumerate(zip(eager, lanes)):
        assert set(pa) == set(pb) == set(POSE_KEYS) | set(STATE_KEYS)
        for k in pa:
            _same_bits(pb[k], pa[k], f"lanes frame {i + 1} {k}")
        for k in ra:
            _same_bits(rb[k], ra[k], f"lanes frame {i + 1} record {k}")
        held += int(ra["held"].sum())
    assert held > 0


# ============================================================================================================ 5. the on-the-fly re-crop
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["deferred", "every_frame_rare", "lanes_every_frame_rare"])
def test_otf_loop_deferred_equals_synchronous(device, mode, monkeypatch):
    """The sync-free re-crop (deferred verdicts; with a bound every frame outgrows: every frame run again from the dict that entered
    it, size state included) against the synchronous stage from the same start, bit for bit; the crop's radius follows the HELD scale."""
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
    cfg = make_config("1", experiment_dir="/tmp/captra_otf_size_test", nocs_otf=True, hipgraph=True)
    cfg["device"] = device
    cfg["init_frame"]["gt"] = True
    cfg["track_cfg"]["size"] = dict(SIZE)
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
    scales, real = [], nocs_otf.full_data_batch_arrays

    def spy(*a, **kw):
        if kw.get("pose_dev") is not None:
            scales.append(kw["pose_dev"][1].clone())
        return real(*a, **kw)
    monkeypatch.setattr(nocs_otf, "full_data_batch_arrays", spy)
    torch.manual_seed(setups[0][3]); np.random.seed(setups[0][3])
    pred2, _ = trainer.test(make(), save=False, no_eval=True)
    for i in range(1, frames):
        assert torch.equal(clouds[i - 1], model.feed_dict[i]["points"]), f"cloud of frame {i}"
    _same_run(pred, pred2, frames, mode)
    assert sum(int(pred["size"][i]["held"].sum()) for i in range(1, frames)) > 0
    per = 2 if lanes else 1
    assert len(scales) == per * (frames - 1)
    B = pred["poses"][0]["scale"].shape[0]
    for i in range(1, frames):
        got = torch.cat(scales[per * (i - 1):per * i]).reshape(B)
        _same_bits(got, pred2["poses"][i - 1]["scale"][:, model.root].reshape(B), f"crop scale of frame {i}")


# ======================================================================================================================= 6. the guard
@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["bottle", "drawers"])
def test_guard_judges_the_held_pose(device, tag):
    """Guard (monitoring) behind the held fit: the poses are those of the run without the guard, and the guard's record is
    part_fit_guard_cn's on each frame's maps and THAT pose."""
    import torch
    from captra_amd.pose_utils.pose_fit import part_fit_guard_cn
    guard = {"refit": False, "lost_below": 0.5}
    _, _, _, alone = _run(device, tag, size=SIZE)
    model, cfg, data, both = _run(device, tag, size=SIZE, guard=guard)
    assert set(both) == {"poses", "npcs_pred", "size", "guard"}
    _same_run(alone, both, len(data), f"guard {tag}")
    B, P = both["poses"][0]["scale"].shape
    g = model.guard
    for i in range(1, len(data)):
        npcs = both["npcs_pred"][i]
        labels = torch.argmax(npcs["seg"], dim=-2).int().contiguous()
        src = npcs["nocs"].reshape(B, P, 3, -1).float().contiguous()
        pts, mean = data[i]["points"].float().to(src.device).contiguous(), data[i]["meta"]["points_mean"].float().to(src.device)
        _, info = part_fit_guard_cn(labels, src, pts, mean, both["poses"][i], inlier_th=g["inlier_th"], lost_below=g["lost_below"],
                                    min_members=g["min_members"], refit=False, num_hyps=g["num_hyps"], seed=g["seed"])
        for k in ("count", "inliers", "rms", "verdict"):
            np.testing.assert_array_equal(both["guard"][i][k].cpu().numpy(), info[k].cpu().numpy(), err_msg=f"frame {i} {k}")
    assert bool(both["size"][len(data) - 1]["held"].any())


# ================================================================================================================ 7. the motion model
MOTION = {"predict": True, "max_angle": 30, "max_shift": 0.2}


@pytest.mark.gpu
def test_motion_and_size_travel_together(device):
    import torch
    _, _, data, alone = _run(device, "bottle", motion=MOTION)
    T = len(data)
    # nothing held: the motion model's records (and the poses) are those of the run without the size option
    model, _, _, both = _run(device, "bottle", motion=MOTION, size={**SIZE, "min_frames": T + 1})
    assert set(both) == {"poses", "npcs_pred", "motion", "size"}
    _same_run(alone, both, T, "motion beside size", records=("motion",))
    # held: the travelling dict carries both options' keys, and the scale the motion model never touches is the held one
    model, _, _, held = _run(device, "bottle", motion=MOTION, size=SIZE)
    feed, npcs_feed = model.feed_dict, model.npcs_feed_dict
    with torch.no_grad():
        _, pose = model.track_step(feed[1], npcs_feed[1], {k: v.clone() for k, v in held["poses"][0].items()})
        pose = {k: v.clone() for k, v in pose.items()}
        _, pose2 = model.track_step(feed[2], npcs_feed[2], pose)
    assert set(pose) == set(pose2) == set(POSE_KEYS) | {"next_rotation", "next_translation", "measured"} | set(STATE_KEYS)
    for k in POSE_KEYS:
        _same_bits(pose2[k], held["poses"][2][k], f"frame 2 {k}")
    _same_bits(pose2["next_rotation"], held["motion"][2]["rotation"], "frame 2 prediction")
    assert torch.equal(pose2["size_n"], held["size"][2]["n"]) and bool(held["size"][2]["held"].any())
    h = held["size"][2]["held"].bool()
    _same_bits(pose2["scale"][h], pose2["size_mean"][h], "the held scale")


# =================================================================================================================== 8. option absent
@pytest.mark.gpu
def test_off_changes_nothing(device, tmp_path):
    import torch
    from captra_amd.graph import TrackStepGraph
    runs = {}
    for name, size in (("absent", None), ("false", {"hold": False, "max_ratio": MAX_RATIO})):
        with _Spy() as spy:
            model, cfg, data, pred = _run(device, "bottle", save=True, hipgraph=True, experiment_dir=tmp_path / name, size=size)
        assert model.size is None and model.net.size is None and not spy.calls
        assert set(pred) == {"poses", "npcs_pred"} and all(set(p) == set(POSE_KEYS) for p in pred["poses"])
        assert not any(k.startswith("size_") for n in pred["npcs_pred"][1:] for k in n)
        assert isinstance(model._graph, TrackStepGraph) and set(model._graph.pose) == set(POSE_KEYS)
        with torch.no_grad():
            _, pose = model.track_step(model.feed_dict[1], model.npcs_feed_dict[1], {k: v.clone() for k, v in pred["poses"][0].items()})
        assert set(pose) == set(POSE_KEYS)
        files = sorted((tmp_path / name / "results" / "data").glob("*.pkl"))
        assert len(files) == 4
        with open(files[0], "rb") as f:
            assert set(pickle.load(f)) == {"pred", "gt", "frame_nums"}
        runs[name] = pred
    for a, b in zip(runs["absent"]["poses"], runs["false"]["poses"]):
        for k in a:
            _same_bits(a[k], b[k], k)
