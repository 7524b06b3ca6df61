"""captra_part_fit_guard (csrc/pose_guard.hip) through the C ABI against the float64 judge of tests/guard_judge.py, and the guard
inside EvalTrackModel's step (track_cfg: {guard: {...}}) in the eager, captured and two-lane forms.

The fixtures are the ones tests/test_guard_cpu.py proves decidable (no residual within 10 % of the threshold, no tie in the lost
rule, no re-fit whose acceptance could turn on a rounding): count, inliers and verdict are exact, rms is at most twice as far
from float64 as the float32 mirror (floor 4 fp32 ulps: the rule of tests/test_pose_readout_gpu.py), and every pose output is
compared bit for bit -- with captra_part_fit_ransac where a part was recovered, with the input everywhere else."""
import pickle

import numpy as np
import pytest

from tests import guard_judge as G
from tests.test_guard_cpu import CHECK_B, CHECK_N, CHECK_P, D, L, LOST_BELOW, REFIT_CASES
from tests.test_pose_readout_gpu import F32_EPS

_CASES = {}


def _cached(key, build):
    if key not in _CASES:
        _CASES[key] = build()
    return _CASES[key]


def _dev(a, device):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _abi(case, device, refit, b0=0, seed=0, num_hyps=64, min_members=4, null_pose=False, shape=None, ratio=(L, D)):
    """The C ABI on sentinel-filled outputs -> (err, dict of numpy outputs)."""
    import torch
    from captra_amd import _lib as Lb
    B, P, _, N = case["src"].shape
    d = {k: _dev(case[k], device) for k in ("labels", "src", "tgt", "tgt_mean", "rot", "scale", "trans")}
    i32 = lambda: torch.full((B, P), -7, dtype=torch.int32, device=device)          # noqa: E731
    out = dict(count=i32(), inliers=i32(), verdict=i32(), rms=torch.full((B, P), float("nan"), device=device),
               rot=torch.full((B, P, 3, 3), float("nan"), device=device), scale=torch.full((B, P), float("nan"), device=device),
               trans=torch.full((B, P, 3), float("nan"), device=device))
    po = (None, None, None) if null_pose else (out["rot"], out["scale"], out["trans"])
    b_, p_, n_, h_ = shape if shape is not None else (B, P, N, num_hyps)
    with torch.cuda.device(device):
        err = Lb.lib().captra_part_fit_guard(b_, p_, n_, b0, Lb.ptr(d["labels"]), Lb.ptr(d["src"]), Lb.ptr(d["tgt"]), Lb.ptr(d["tgt_mean"]),
                                             Lb.ptr(d["rot"]), Lb.ptr(d["scale"]), Lb.ptr(d["trans"]), float(case["th"]), ratio[0], ratio[1],
                                             min_members, refit, h_, seed, Lb.ptr(out["count"]), Lb.ptr(out["inliers"]), Lb.ptr(out["rms"]),
                                             Lb.ptr(out["verdict"]), Lb.ptr(po[0]), Lb.ptr(po[1]), Lb.ptr(po[2]), Lb.stream_ptr())
    torch.cuda.synchronize(device)
    return err, {k: v.cpu().numpy() for k, v in out.items()}


def _ransac(case, device, seed=0, num_hyps=64):
    """captra_part_fit_ransac on the same inputs, drawing in the kernel."""
    from captra_amd.pose_utils.pose_fit import part_fit_ransac_cn
    rot, scale, trans, valid, info = part_fit_ransac_cn(_dev(case["labels"], device), _dev(case["src"], device), _dev(case["tgt"], device),
                                                        num_hyps=num_hyps, inlier_th=float(case["th"]), seed=seed,
                                                        target_mean=_dev(case["tgt_mean"], device))
    return dict(rot=rot.cpu().numpy(), scale=scale.cpu().numpy(), trans=trans[..., 0].cpu().numpy(), valid=valid.cpu().numpy(),
                num_inliers=info["num_inliers"].cpu().numpy())


def _check_record(got, ref, mir, name):
    for k in ("count", "inliers", "verdict"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=f"{name} {k}")
    assert np.isfinite(got["rms"]).all(), name
    err, merr = np.abs(got["rms"].astype(np.float64) - ref["rms"]), np.abs(mir["rms"].astype(np.float64) - ref["rms"])
    print(f"{name}: rms err kernel {err.max():.2e} mirror {merr.max():.2e}")
    assert (err <= np.maximum(2 * merr, 4 * F32_EPS * np.abs(ref["rms"]))).all(), (name, err, merr)
    assert (got["rms"][ref["inliers"] == 0] == 0).all(), name


def _same_bits(a, b, msg):
    np.testing.assert_array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32),
                                  err_msg=msg)


@pytest.mark.gpu
@pytest.mark.parametrize("N", CHECK_N)
@pytest.mark.parametrize("P", CHECK_P)
@pytest.mark.parametrize("B", CHECK_B)
def test_guard_check_vs_judge(device, B, P, N):
    """With and without pts_mean; parts of 0, 2, 3, 4 and N members, labels outside [0, P), NaN / Inf in non-member points and in
    one member, a pose with scale 0: exact count / inliers / verdict, rms within the bound, the pose handed through bit for bit,
    NULL pose outputs accepted."""
    for with_mean in (False, True):
        case, ref, mir = _cached(("check", B, P, N, with_mean), lambda: (lambda c: (c, G.preconditions(c, L, D), G.judge(c, L, D, dt=np.float32)))(
            G.check_case(B, P, N, with_mean)))
        err, got = _abi(case, device, refit=0)
        assert err == 0
        _check_record(got, ref, mir, f"B={B} P={P} N={N} mean={with_mean}")
        for k in ("rot", "scale", "trans"):
            _same_bits(got[k], case[k], k)
        err, null = _abi(case, device, refit=0, null_pose=True)
        assert err == 0 and np.isnan(null["rot"]).all()
        for k in ("count", "inliers", "verdict", "rms"):
            np.testing.assert_array_equal(null[k], got[k])


@pytest.mark.gpu
@pytest.mark.parametrize("B,P,N,b0,cseed", REFIT_CASES)
def test_guard_refit_vs_judge_and_ransac(device, B, P, N, b0, cseed):
    """ok / lost -> recovered / lost with the re-fit rejected, by the judge that draws with b0 + b; a recovered pose is
    captra_part_fit_ransac's bit for bit (for b0 = 5: on the batch padded with five empty trajectories in front, so that its
    b is the guard's b0 + b), every other pose the input's; refit = 0: the same verdicts without 3."""
    case = _cached(("refit", B, P, N, cseed), lambda: G.refit_case(B, P, N, cseed))
    ref = _cached(("refit-ref", B, P, N, cseed, b0), lambda: G.preconditions(case, L, D, refit=True, b0=b0))
    mir = G.judge(case, L, D, refit=True, b0=b0, dt=np.float32)
    err, got = _abi(case, device, refit=1, b0=b0)
    assert err == 0
    _check_record(got, ref, mir, f"refit B={B} P={P} N={N} b0={b0}")
    padded = dict(case)
    if b0:
        pad = lambda a, fill: np.concatenate([np.full((b0,) + a.shape[1:], fill, a.dtype), a])          # noqa: E731
        padded.update(labels=pad(case["labels"], -1), src=pad(case["src"], 0), tgt=pad(case["tgt"], 0), tgt_mean=pad(case["tgt_mean"], 0))
    direct = _ransac(padded, device)
    rec = ref["verdict"] == G.RECOVERED
    assert rec.any() or P * B < 2
    for b in range(B):
        for p in range(P):
            if rec[b, p]:
                assert direct["valid"][b0 + b, p] and direct["num_inliers"][b0 + b, p] > got["inliers"][b, p]
                want = {k: direct[k][b0 + b, p] for k in ("rot", "scale", "trans")}
            else:
                want = {k: case[k][b, p] for k in ("rot", "scale", "trans")}
            for k in want:
                _same_bits(got[k][b, p], want[k], f"{k} ({b},{p}) verdict {ref['verdict'][b, p]}")
    assert np.isfinite(got["rot"]).all() and np.isfinite(got["scale"]).all() and np.isfinite(got["trans"]).all()
    err, off = _abi(case, device, refit=0, b0=b0, null_pose=True)
    assert err == 0
    np.testing.assert_array_equal(off["verdict"], np.where(rec, G.LOST, ref["verdict"]))
    for k in ("count", "inliers", "rms"):
        np.testing.assert_array_equal(off[k], got[k])


@pytest.mark.gpu
def test_guard_refused_arguments(device):
    """Shapes beyond the RANSAC kernel's, a negative b0, a zero denominator, refit = 2, refit = 1 without pose outputs: -1, nothing written."""
    case = G.check_case(3, 4, 255, False)
    bad = [dict(shape=(3, 9, 255, 64)), dict(shape=(3, 4, 255, 0)), dict(shape=(3, 4, 255, 257)), dict(shape=(3, 4, 16385, 64)),
           dict(shape=(3, 4, 0, 64)), dict(b0=-1), dict(ratio=(1, 0)), dict(ratio=(-1, 2)), dict(refit=2), dict(refit=1, null_pose=True)]
    for kw in bad:
        err, got = _abi(case, device, **{"refit": 0, **kw})
        assert err == -1, kw
        assert (got["verdict"] == -7).all() and np.isnan(got["rms"]).all() and np.isnan(got["rot"]).all(), kw


@pytest.mark.gpu
def test_part_fit_guard_wrapper(device):
    """part_fit_guard_cn gives the ABI's bits; refit=False hands the pose dict through untouched."""
    import torch
    from captra_amd.pose_utils.pose_fit import part_fit_guard_cn
    B, P, N, b0, cseed = REFIT_CASES[1]
    case = _cached(("refit", B, P, N, cseed), lambda: G.refit_case(B, P, N, cseed))
    pose = {"rotation": _dev(case["rot"], device), "scale": _dev(case["scale"], device), "translation": _dev(case["trans"], device).unsqueeze(-1)}
    args = (_dev(case["labels"], device), _dev(case["src"], device), _dev(case["tgt"], device), _dev(case["tgt_mean"], device), pose)
    for refit in (False, True):
        err, got = _abi(case, device, refit=int(refit), b0=b0)
        assert err == 0
        out, info = part_fit_guard_cn(*args, inlier_th=float(case["th"]), lost_below=LOST_BELOW, refit=refit, b0=b0)
        assert (out is pose) == (not refit)
        assert out["translation"].shape == (B, P, 3, 1) and info["verdict"].dtype == torch.int32
        for k in ("count", "inliers", "rms", "verdict"):
            np.testing.assert_array_equal(info[k].cpu().numpy(), got[k])
        for k, g in (("rotation", "rot"), ("scale", "scale")):
            _same_bits(out[k].cpu().numpy(), got[g], k)
        _same_bits(out["translation"][..., 0].cpu().numpy(), got["trans"], "translation")


# ------------------------------------------------------------------------------------------------------------------- the model
def _model(device, guard, batch, frames, tag="bottle", hipgraph=False, experiment_dir="/tmp/captra_test_exp"):
    from captra_amd import synthetic as clouds
    from captra_amd.configs import make_config
    from captra_amd.trainer import Trainer
    cat, objcfg, kind, _, _, wseed, _ = clouds.PHYSICAL_SETUPS[tag]
    cfg = make_config(cat, objcfg, experiment_dir=str(experiment_dir))
    if guard is not None:
        cfg["track_cfg"]["guard"] = dict(guard)
    cfg["hipgraph"] = hipgraph
    trainer = Trainer(cfg)
    shapes = {k: tuple(v.shape) for k, v in trainer.model.state_dict().items()}
    trainer.model.load_state_dict(clouds.make_physical_state_dict(shapes, wseed, cfg["num_parts"], bool(cfg["obj_sym"]), kind))
    return trainer, cfg, clouds.make_trajectory(kind, batch, frames, seed=7)


def _run(device, guard, batch, frames, hipgraph=False, tag="bottle"):
    import torch
    trainer, cfg, data = _model(device, guard, batch, frames, tag=tag, hipgraph=hipgraph)
    torch.manual_seed(4321)
    pred, _ = trainer.test(data, save=False, no_eval=True)
    return trainer.model, cfg, data, pred


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _direct_record(model, pred, data, i, pose, b0=0):
    """part_fit_guard_cn on frame i's saved maps and the pose `pose`."""
    import torch
    from captra_amd.pose_utils.pose_fit import part_fit_guard_cn
    npcs = pred["npcs_pred"][i]
    B, P = pose["scale"].shape
    g = model.guard
    labels = torch.argmax(npcs["seg"], dim=-2).int().contiguous()
    src = npcs["nocs"].reshape(B, P, 3, -1).float().contiguous()
    dev = src.device
    return part_fit_guard_cn(labels, src, data[i]["points"].float().to(dev).contiguous(), data[i]["meta"]["points_mean"].float().to(dev), pose,
                             inlier_th=g["inlier_th"], lost_below=g["lost_below"], min_members=g["min_members"], refit=g["refit"],
                             num_hyps=g["num_hyps"], seed=g["seed"], b0=b0)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["eager", "hipgraph", "lanes"])
def test_monitoring_changes_no_pose_and_records_every_frame(device, form):
    """refit: False in the eager (B = 2), captured (B = 2) and two-lane (B = 32) forms, 2 tracked frames: poses and maps bit-identical to the
    guard-off run, pred_dict['guard'] = [None, record, record], each record what part_fit_guard_cn gives on that frame's saved
    maps and pose."""
    from captra_amd.graph import TrackLanes, TrackStepGraph
    B, hipgraph = (32, True) if form == "lanes" else (2, form == "hipgraph")
    _, _, _, off = _run(device, None, B, 3, hipgraph)
    model, _, data, on = _run(device, {"refit": False, "lost_below": 0.5}, B, 3, hipgraph)
    if form != "eager":
        assert isinstance(model._graph, TrackLanes if form == "lanes" else TrackStepGraph)
    assert "guard" not in off and len(on["guard"]) == 3 and on["guard"][0] is None
    for i, (a, b) in enumerate(zip(off["poses"], on["poses"])):
        for k in a:
            np.testing.assert_array_equal(a[k].cpu().numpy(), b[k].cpu().numpy(), err_msg=f"frame {i} {k}")
    for i in (1, 2):
        assert set(on["npcs_pred"][i]) == set(off["npcs_pred"][i])
        _, info = _direct_record(model, on, data, i, on["poses"][i])
        for k in ("count", "inliers", "rms", "verdict"):
            assert on["guard"][i][k].shape == (B, 1)
            np.testing.assert_array_equal(on["guard"][i][k].cpu().numpy(), info[k].cpu().numpy(), err_msg=f"frame {i} {k}")
        print(form, i, "verdicts", np.bincount(on["guard"][i]["verdict"].cpu().numpy().ravel(), minlength=4).tolist())


# The re-fit tests need parts that ARE recovered, or they would compare a pose with itself.  What the synthetic networks give is not
# under the tests' control, the guard's settings are: the guard-off run's saved maps and poses say, through direct calls of
# part_fit_guard_cn, what each candidate setting WILL do in the guarded run (frame 1 enters both runs with the same pose), and the
# first candidate that recovers a part where the test needs one is run.  No candidate -> the test fails.
REFIT_SETTINGS = ((0.005, 64), (0.002, 64), (0.005, 2), (0.002, 2), (0.01, 2), (0.001, 64), (0.001, 2), (0.02, 64))    # (inlier_th, num_hyps)


def _maps(npcs, points, mean, B, P, sl=slice(None)):
    import torch
    labels = torch.argmax(npcs["seg"], dim=-2).int()[sl].contiguous()
    src = npcs["nocs"].reshape(B, P, 3, -1).float()[sl].contiguous()
    return labels, src, points.float().to(src.device)[sl].contiguous(), mean.float().to(src.device)[sl].contiguous()


def _search(maps, pose, radius, need, b0s=(0,)):
    """The first of REFIT_SETTINGS for which `need(results)` holds; results = [(pose out, info) for b0 in b0s] of the direct call."""
    from captra_amd.pose_utils.pose_fit import part_fit_guard_cn
    for th, H in REFIT_SETTINGS:
        res = [part_fit_guard_cn(*maps, pose, inlier_th=th * radius, lost_below=1.0, refit=True, num_hyps=H, seed=0, b0=b0) for b0 in b0s]
        print("setting", th, H, "verdicts", [np.bincount(r[1]["verdict"].cpu().numpy().ravel(), minlength=4).tolist() for r in res])
        if need(res):
            return {"refit": True, "lost_below": 1.0, "inlier_th": th, "num_hyps": H}, res
    raise AssertionError("no setting of REFIT_SETTINGS recovers a part where this test needs one")


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["bottle", "drawers"])
def test_refit_step_is_where_recovered_ransac_else_step(device, tag):
    """refit: True, one track_step from frame 0's annotated pose, guard off and on.  lost_below = 1 sends every part that has an
    outlier into the re-fit; at least one part is recovered, and the final pose is where(verdict == 3, captra_part_fit_ransac on
    the step's own maps, guard-off pose), bit for bit."""
    import torch
    from captra_amd.pose_utils.pose_fit import part_fit_ransac_cn

    def step(g):
        trainer, cfg, data = _model(device, g, 2, 2, tag=tag)
        model = trainer.model
        model.set_data(data)
        with torch.no_grad():
            npcs, pose = model.track_step(model.feed_dict[1], model.npcs_feed_dict[1], {k: v.clone() for k, v in model.feed_dict[0]["gt_part"].items()})
        return model, cfg, {k: v for k, v in npcs.items() if torch.is_tensor(v)}, pose

    model0, cfg, npcs0, off = step(None)
    B, P = off["scale"].shape
    feed = model0.feed_dict[1]
    maps = _maps(npcs0, feed["points"], feed["points_mean"], B, P)
    guard, _ = _search(maps, off, float(cfg["data_radius"]), lambda res: bool((res[0][1]["verdict"] == 3).any()))
    model, _, npcs, on = step(guard)
    verdict = npcs["guard_verdict"]
    rec = verdict == 3
    assert bool(rec.any()), verdict
    rot, scale, trans, valid, info = part_fit_ransac_cn(maps[0], maps[1], maps[2], num_hyps=model.guard["num_hyps"], inlier_th=model.guard["inlier_th"],
                                                        seed=model.guard["seed"], target_mean=maps[3])
    print(tag, "verdicts", verdict.cpu().numpy().tolist(), "inliers", npcs["guard_inliers"].cpu().numpy().tolist(), "of", npcs["guard_count"].cpu().numpy().tolist(),
          "ransac", info["num_inliers"].cpu().numpy().tolist())
    assert bool((valid & (info["num_inliers"] > npcs["guard_inliers"]))[rec].all())
    want = {"rotation": torch.where(rec[..., None, None], rot, off["rotation"]), "scale": torch.where(rec, scale, off["scale"]),
            "translation": torch.where(rec[..., None, None], trans, off["translation"])}
    assert not torch.equal(want["rotation"], off["rotation"])               # (a recovered part's pose IS another pose)
    for k in want:
        _same_bits(on[k].cpu().numpy(), want[k].cpu().numpy(), k)
    for k in ("seg", "nocs"):
        np.testing.assert_array_equal(npcs[k].cpu().numpy(), npcs0[k].cpu().numpy())


@pytest.mark.gpu
def test_lanes_draw_what_the_whole_batch_draws(device):
    """B = 32, refit: True with lost_below = 1: the whole batch in the eager loop and the two captured lanes (the second one's
    b0 = 16) give equal records and equal poses -- under a setting for which the second lane recovers a part in frame 1 AND a
    direct call on the second lane's data with b0 = 0 instead of 16 returns other bits, so a lane that lost its b0 on the way
    from step_inputs to the kernel could not pass."""
    import torch
    from captra_amd.graph import TrackLanes
    _, cfg, data, off = _run(device, None, 32, 3, hipgraph=False)
    lane1 = slice(16, 32)
    maps = _maps(off["npcs_pred"][1], data[1]["points"], data[1]["meta"]["points_mean"], 32, 1, lane1)
    pose1 = {k: v[lane1].contiguous() for k, v in off["poses"][1].items()}

    def need(res):
        (p16, i16), (p0, i0) = res
        return bool((i16["verdict"] == 3).any()) and any(not torch.equal(p16[k], p0[k]) for k in p16)
    guard, ((p16, i16), (p0, _)) = _search(maps, pose1, float(cfg["data_radius"]), need, b0s=(16, 0))
    _, _, _, whole = _run(device, guard, 32, 3, hipgraph=False)
    model, _, _, lanes = _run(device, guard, 32, 3, hipgraph=True)
    assert isinstance(model._graph, TrackLanes) and [g.b0 for g in model._graph.graphs] == [0, 16]
    assert bool((whole["guard"][1]["verdict"][lane1] == 3).any())
    for i in (1, 2):
        for k in ("count", "inliers", "rms", "verdict"):
            np.testing.assert_array_equal(whole["guard"][i][k].cpu().numpy(), lanes["guard"][i][k].cpu().numpy(), err_msg=f"frame {i} {k}")
        for k in whole["poses"][i]:
            np.testing.assert_array_equal(whole["poses"][i][k].cpu().numpy(), lanes["poses"][i][k].cpu().numpy(), err_msg=f"frame {i} {k}")
        print("frame", i, "verdicts", np.bincount(whole["guard"][i]["verdict"].cpu().numpy().ravel(), minlength=4).tolist())
    # frame 1 of the second lane IS the direct call with b0 = 16, and is NOT the one with b0 = 0
    np.testing.assert_array_equal(lanes["guard"][1]["verdict"][lane1].cpu().numpy(), i16["verdict"].cpu().numpy())
    for k in p16:
        _same_bits(lanes["poses"][1][k][lane1].cpu().numpy(), p16[k].cpu().numpy(), f"lane 1 {k} vs the direct call with b0 = 16")
    assert any(not torch.equal(lanes["poses"][1][k][lane1], p0[k]) for k in p0)


@pytest.mark.gpu
def test_pickles_carry_the_record_only_when_on(device, tmp_path, capsys):
    """The result pickles: 'guard' = per frame None / {'count','inliers','rms','verdict'} of shape (P,) when the guard is on, the
    key set of a guard-off run otherwise; captra_amd.eval's table reads it."""
    import torch
    from captra_amd.eval import guard_table
    keys = {}
    for name, guard in (("off", None), ("on", {"refit": True, "lost_below": 0.5})):
        trainer, cfg, data = _model(device, guard, 2, 3, experiment_dir=tmp_path / name)
        torch.manual_seed(4321)
        trainer.test(data, save=True, no_eval=True)
        files = sorted((tmp_path / name / "results" / "data").glob("*.pkl"))
        assert len(files) == 2
        with open(files[0], "rb") as f:
            keys[name] = pickle.load(f)
    assert set(keys["off"]) == {"pred", "gt", "frame_nums"}
    assert set(keys["on"]) == {"pred", "gt", "frame_nums", "guard"}
    assert set(keys["on"]["pred"]) == set(keys["off"]["pred"])
    rec = keys["on"]["guard"]
    assert rec[0] is None and len(rec) == 3
    for r in rec[1:]:
        assert set(r) == {"count", "inliers", "rms", "verdict"} and all(np.asarray(v).shape == (1,) for v in r.values())
    lines = guard_table("x", keys["on"])
    assert len(lines) == 1 and "lost" in lines[0] and "recovered" in lines[0] and "too_few" in lines[0]
