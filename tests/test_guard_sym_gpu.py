"""captra_part_fit_guard_sym and captra_part_fit_ransac_sym (the axis-only inlier test of the symmetric categories: csrc/pose_solve.h,
pose_guard.hip, pose_ransac.h) through the C ABI against the float64 judge of tests/sym_judge.py, and the guard with
track_cfg: {guard: {yaxis_only: True}} inside EvalTrackModel's step on bottle in the eager, captured and two-lane forms.

The fixtures are the ones tests/test_guard_sym_cpu.py proves decidable: count, inliers, verdict, the best hypothesis and its score
are exact; rms follows the rule of tests/test_guard_gpu.py (at most twice the mirror's distance from float64, floor 4 fp32 ulps);
a pose is compared bit for bit where it is handed through or where the guard's re-fit stands beside the fit alone, and with
float64 by the rule of tests/test_pose_ransac_gpu.py (twice the mirror, floors of tests/test_pose_readout_gpu.py: that file keeps
the rule inside its `_check`, which also recomputes the full-rotation inlier set, so the rule is applied here from the same
constants)."""
import numpy as np
import pytest

from tests import sym_judge as Y
from tests.test_guard_cpu import D, L
from tests.test_guard_gpu import REFIT_SETTINGS, _check_record, _dev, _maps, _model, _run, _same_bits
from tests.test_guard_sym_cpu import REFIT_CASES, SHAPES, check_fixture, refit_fixture
from tests.test_pose_readout_gpu import DET_ATOL, F32_EPS, MATRIX_ATOL, ORTHO_ATOL

YAXIS = {"yaxis_only": True}


def _abi(case, device, refit, sym=True, b0=0, seed=0, num_hyps=64, min_members=4, null_pose=False, shape=None, ratio=(L, D), pose=None):
    """captra_part_fit_guard[_sym] on sentinel-filled outputs -> (err, dict of numpy outputs).  pose: (rot, scale, trans) in place of the case's."""
    import torch
    from captra_amd import _lib as Lb
    B, P, _, N = case["src"].shape
    src = dict(case)
    if pose is not None:
        src["rot"], src["scale"], src["trans"] = pose
    d = {k: _dev(src[k], device) for k in ("labels", "src", "tgt", "tgt_mean", "rot", "scale", "trans")}
    i32 = lambda: torch.full((B, P), -7, dtype=torch.int32, device=device)          # noqa: E731
    out = dict(count=i32(), inliers=i32(), verdict=i32(), rms=torch.full((B, P), float("nan"), device=device),
               rot=torch.full((B, P, 3, 3), float("nan"), device=device), scale=torch.full((B, P), float("nan"), device=device),
               trans=torch.full((B, P, 3), float("nan"), device=device))
    po = (None, None, None) if null_pose else (out["rot"], out["scale"], out["trans"])
    b_, p_, n_, h_ = shape if shape is not None else (B, P, N, num_hyps)
    fn = getattr(Lb.lib(), "captra_part_fit_guard_sym" if sym else "captra_part_fit_guard")
    with torch.cuda.device(device):
        err = fn(b_, p_, n_, b0, Lb.ptr(d["labels"]), Lb.ptr(d["src"]), Lb.ptr(d["tgt"]), Lb.ptr(d["tgt_mean"]), Lb.ptr(d["rot"]),
                 Lb.ptr(d["scale"]), Lb.ptr(d["trans"]), float(case["th"]), ratio[0], ratio[1], min_members, refit, h_, seed,
                 Lb.ptr(out["count"]), Lb.ptr(out["inliers"]), Lb.ptr(out["rms"]), Lb.ptr(out["verdict"]), Lb.ptr(po[0]), Lb.ptr(po[1]),
                 Lb.ptr(po[2]), Lb.stream_ptr())
    torch.cuda.synchronize(device)
    return err, {k: v.cpu().numpy() for k, v in out.items()}


def _ransac_abi(case, device, seed=0, num_hyps=64, shape=None):
    """captra_part_fit_ransac_sym drawing in the kernel, on sentinel-filled outputs."""
    import torch
    from captra_amd import _lib as Lb
    B, P, _, N = case["src"].shape
    d = {k: _dev(case[k], device) for k in ("labels", "src", "tgt", "tgt_mean")}
    out = dict(rot=torch.full((B, P, 3, 3), float("nan"), device=device), scale=torch.full((B, P), float("nan"), device=device),
               trans=torch.full((B, P, 3), float("nan"), device=device), valid=torch.full((B, P), -7, dtype=torch.int32, device=device),
               best=torch.full((B, P), -7, dtype=torch.int32, device=device), num_inliers=torch.full((B, P), -7, dtype=torch.int32, device=device))
    b_, p_, n_, h_ = shape if shape is not None else (B, P, N, num_hyps)
    with torch.cuda.device(device):
        err = Lb.lib().captra_part_fit_ransac_sym(b_, p_, n_, h_, float(case["th"]), Lb.ptr(d["labels"]), Lb.ptr(d["src"]), Lb.ptr(d["tgt"]), 0,
                                                  Lb.ptr(d["tgt_mean"]), None, seed, Lb.ptr(out["rot"]), Lb.ptr(out["scale"]), Lb.ptr(out["trans"]),
                                                  Lb.ptr(out["valid"]), Lb.ptr(out["best"]), Lb.ptr(out["num_inliers"]), None, Lb.stream_ptr())
    torch.cuda.synchronize(device)
    return err, {k: v.cpu().numpy() for k, v in out.items()}


def _padded(case, b0):
    """The batch with b0 empty trajectories in front: its b is the guard's b0 + b."""
    if not b0:
        return case
    pad = lambda a, fill: np.concatenate([np.full((b0,) + a.shape[1:], fill, a.dtype), a])          # noqa: E731
    return dict(case, labels=pad(case["labels"], -1), src=pad(case["src"], 0), tgt=pad(case["tgt"], 0), tgt_mean=pad(case["tgt_mean"], 0))


@pytest.mark.gpu
@pytest.mark.parametrize("B,P,N,b0", SHAPES)
def test_sym_check_vs_judge(device, B, P, N, b0):
    """1. With and without pts_mean; parts of 0, 2, 3, 4 and N members, labels outside [0, P), NaN / Inf in non-members and in one
    member, a pose with scale 0: exact count / inliers / verdict, rms within the bound, the pose handed through bit for bit, NULL
    pose outputs accepted."""
    for with_mean in (False, True):
        case, ref, mir = check_fixture(B, P, N, with_mean)
        err, got = _abi(case, device, refit=0, b0=b0)
        assert err == 0
        _check_record(got, ref, mir, f"sym B={B} P={P} N={N} mean={with_mean}")
        for k in ("rot", "scale", "trans"):
            _same_bits(got[k], case[k], k)
        err, null = _abi(case, device, refit=0, b0=b0, null_pose=True)
        assert err == 0 and np.isnan(null["rot"]).all()
        for k in ("count", "inliers", "verdict", "rms"):
            np.testing.assert_array_equal(null[k], got[k])


@pytest.mark.gpu
@pytest.mark.parametrize("B,P,N,b0,cseed,first", REFIT_CASES)
def test_decisive_pair_and_invariance(device, B, P, N, b0, cseed, first):
    """2. On the same buffers the full-rotation entry calls every phi-rotated TRUE pose lost, the axis-only entry calls it ok with
    exactly the true inliers.  3. A second pose, rotated by another R_y and rounded again, gives identical count / inliers / verdict."""
    case, ref, _ = refit_fixture(B, P, N, b0, cseed, first)
    true = np.array([[case["modes"][b, p] == "true" for p in range(P)] for b in range(B)])
    err, old = _abi(case, device, refit=0, sym=False)
    err2, new = _abi(case, device, refit=0)
    assert err == 0 and err2 == 0
    if true.any():
        print("true parts: members", new["count"][true].tolist(), "full-rotation inliers", old["inliers"][true].tolist(), "axis-only", new["inliers"][true].tolist())
        assert (old["verdict"][true] == Y.LOST).all()
        assert (new["verdict"][true] == Y.OK).all()
        np.testing.assert_array_equal(new["inliers"][true], case["n_true"][true])
    rng = np.random.default_rng(B * 1000 + N)
    rot2 = np.stack([[(case["rot"][b, p].astype(np.float64) @ Y.rot_y(rng.uniform(0.5, 2.5))).astype(np.float32) for p in range(P)] for b in range(B)])
    assert not np.array_equal(rot2, case["rot"])
    err, again = _abi(case, device, refit=0, pose=(rot2, case["scale"], case["trans"]))
    assert err == 0
    for k in ("count", "inliers", "verdict"):
        np.testing.assert_array_equal(again[k], new[k], err_msg=k)


@pytest.mark.gpu
@pytest.mark.parametrize("B,P,N,b0,cseed,first", REFIT_CASES)
def test_sym_refit_vs_judge_and_ransac(device, B, P, N, b0, cseed, first):
    """4. Verdicts by the judge that draws with b0 + b; a recovered pose is captra_part_fit_ransac_sym's bit for bit (for b0 = 5 on
    the batch padded in front), every other pose the input's; refit = 0: the same verdicts with lost in place of recovered."""
    case, ref, mir = refit_fixture(B, P, N, b0, cseed, first)
    err, got = _abi(case, device, refit=1, b0=b0)
    assert err == 0
    _check_record(got, ref, mir, f"sym refit B={B} P={P} N={N} b0={b0} first={first}")
    err, direct = _ransac_abi(_padded(case, b0), device)
    assert err == 0
    rec = ref["verdict"] == Y.RECOVERED
    for b in range(B):
        for p in range(P):
            if rec[b, p]:
                assert direct["valid"][b0 + b, p] == 1 and direct["num_inliers"][b0 + b, p] > got["inliers"][b, p]
                want = {k: direct[k][b0 + b, p] for k in ("rot", "scale", "trans")}
            else:
                want = {k: case[k][b, p] for k in ("rot", "scale", "trans")}
            for k in want:
                _same_bits(got[k][b, p], want[k], f"{k} ({b},{p}) verdict {ref['verdict'][b, p]}")
    assert np.isfinite(got["rot"]).all() and np.isfinite(got["scale"]).all() and np.isfinite(got["trans"]).all()
    err, off = _abi(case, device, refit=0, b0=b0, null_pose=True)
    assert err == 0
    np.testing.assert_array_equal(off["verdict"], np.where(rec, Y.LOST, ref["verdict"]))
    for k in ("count", "inliers", "rms"):
        np.testing.assert_array_equal(off[k], got[k])


@pytest.mark.gpu
@pytest.mark.parametrize("B,P,N,b0,cseed,first", REFIT_CASES)
def test_sym_first_pose_fit_vs_judge(device, B, P, N, b0, cseed, first):
    """5. captra_part_fit_ransac_sym on the recipe clouds, drawing in the kernel: the judge's best hypothesis and inlier count,
    validity, and the pose within twice the mirror's distance from float64 (floors: 4 fp32 ulps, MATRIX_ATOL)."""
    case = _padded(refit_fixture(B, P, N, b0, cseed, first)[0], b0)
    ref, pinned = Y.fit_preconditions(case)
    mir = Y.judge_fit(case, dt=np.float32)
    err, got = _ransac_abi(case, device)
    assert err == 0
    np.testing.assert_array_equal(got["valid"].astype(bool), ref["valid"])
    assert pinned or not ref["valid"].any()         # (the single part of gross outliers has nothing to pin)
    for b in range(case["src"].shape[0]):
        for p in range(P):
            tag = (b, p)
            if not ref["valid"][b, p]:
                np.testing.assert_array_equal(got["rot"][b, p], np.eye(3, dtype=np.float32), err_msg=str(tag))
                assert got["scale"][b, p] == 1.0 and (got["trans"][b, p] == 0.0).all() and got["num_inliers"][b, p] < 3, tag
                continue
            assert (b, p) in pinned and mir["valid"][b, p], tag
            assert got["best"][b, p] == ref["best"][b, p] and got["num_inliers"][b, p] == ref["num_inliers"][b, p], tag
            R = got["rot"][b, p].astype(np.float64)
            es, ms = abs(got["scale"][b, p] - ref["scale"][b, p]), abs(mir["scale"][b, p] - ref["scale"][b, p])
            et, mt = np.abs(got["trans"][b, p] - ref["trans"][b, p]).max(), np.abs(mir["trans"][b, p] - ref["trans"][b, p]).max()
            er, mr = np.abs(R - ref["rot"][b, p]).max(), np.abs(mir["rot"][b, p] - ref["rot"][b, p]).max()
            print(f"{tag}: scale err kernel {es:.2e} mirror {ms:.2e}; trans {et:.2e} / {mt:.2e}; rot {er:.2e} / {mr:.2e}")
            assert es <= max(2 * ms, 4 * F32_EPS * abs(ref["scale"][b, p])), (tag, es, ms)
            assert et <= max(2 * mt, 4 * F32_EPS * np.abs(ref["trans"][b, p]).max()), (tag, et, mt)
            assert er <= max(2 * mr, MATRIX_ATOL), (tag, er, mr)
            assert np.abs(R.T @ R - np.eye(3)).max() <= ORTHO_ATOL and abs(np.linalg.det(R) - 1.0) <= DET_ATOL, tag


@pytest.mark.gpu
def test_sym_refused_arguments(device):
    """6. What captra_part_fit_guard / captra_part_fit_ransac refuse: -1, nothing written."""
    case = check_fixture(3, 4, 4096, False)[0]
    bad = [dict(shape=(3, 9, 4096, 64)), dict(shape=(3, 4, 4096, 0)), dict(shape=(3, 4, 4096, 257)), dict(shape=(3, 4, 16385, 64)),
           dict(shape=(3, 4, 0, 64)), dict(b0=-1), dict(ratio=(1, 0)), dict(ratio=(-1, 2)), dict(refit=2), dict(refit=1, null_pose=True)]
    for kw in bad:
        err, got = _abi(case, device, **{"refit": 0, **kw})
        assert err == -1, kw
        assert (got["verdict"] == -7).all() and np.isnan(got["rms"]).all() and np.isnan(got["rot"]).all(), kw
    for shape in ((3, 9, 4096, 64), (3, 4, 4096, 0), (3, 4, 4096, 257), (3, 4, 16385, 64), (3, 4, 0, 64)):
        err, got = _ransac_abi(case, device, shape=shape)
        assert err == -1, shape
        assert np.isnan(got["rot"]).all() and (got["valid"] == -7).all() and (got["best"] == -7).all()


# ------------------------------------------------------------------------------------------------------------------- the model
def _direct_record(model, pred, data, i, pose, yaxis_only, b0=0):
    """part_fit_guard_cn on frame i's saved maps and the pose `pose`."""
    from captra_amd.pose_utils.pose_fit import part_fit_guard_cn
    B, P = pose["scale"].shape
    g = model.guard
    maps = _maps(pred["npcs_pred"][i], data[i]["points"], data[i]["meta"]["points_mean"], B, P)
    return part_fit_guard_cn(*maps, pose, inlier_th=g["inlier_th"], lost_below=g["lost_below"], min_members=g["min_members"], refit=g["refit"],
                             num_hyps=g["num_hyps"], seed=g["seed"], b0=b0, yaxis_only=yaxis_only)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["eager", "hipgraph", "lanes"])
def test_sym_monitoring_changes_no_pose_and_records_every_frame(device, form):
    """7. refit: False with yaxis_only on bottle, eager (B = 2), captured (B = 2), two-lane (B = 32), 3 frames: poses and maps
    bit-identical to the guard-off run, each record what part_fit_guard_cn(..., yaxis_only=True) gives on that frame's saved maps
    and pose (the full-rotation entry's counts are printed beside them)."""
    from captra_amd.graph import TrackLanes, TrackStepGraph
    B, hipgraph = (32, True) if form == "lanes" else (2, form == "hipgraph")
    _, _, _, off = _run(device, None, B, 3, hipgraph)
    model, _, data, on = _run(device, {"refit": False, "lost_below": 0.5, **YAXIS}, B, 3, hipgraph)
    assert model.guard["yaxis_only"] is True
    if form != "eager":
        assert isinstance(model._graph, TrackLanes if form == "lanes" else TrackStepGraph)
    assert "guard" not in off and len(on["guard"]) == 3 and on["guard"][0] is None
    for i, (a, b) in enumerate(zip(off["poses"], on["poses"])):
        for k in a:
            np.testing.assert_array_equal(a[k].cpu().numpy(), b[k].cpu().numpy(), err_msg=f"frame {i} {k}")
    for i in (1, 2):
        assert set(on["npcs_pred"][i]) == set(off["npcs_pred"][i])
        for k in ("seg", "nocs"):
            np.testing.assert_array_equal(on["npcs_pred"][i][k].cpu().numpy(), off["npcs_pred"][i][k].cpu().numpy())
        _, info = _direct_record(model, on, data, i, on["poses"][i], True)
        _, full = _direct_record(model, on, data, i, on["poses"][i], False)
        assert set(on["guard"][i]) == {"count", "inliers", "rms", "verdict"}
        for k in ("count", "inliers", "rms", "verdict"):
            assert on["guard"][i][k].shape == (B, 1)
            np.testing.assert_array_equal(on["guard"][i][k].cpu().numpy(), info[k].cpu().numpy(), err_msg=f"frame {i} {k}")
        print(form, i, "verdicts", np.bincount(on["guard"][i]["verdict"].cpu().numpy().ravel(), minlength=4).tolist(), "inliers axis-only",
              info["inliers"].cpu().numpy().ravel()[:4].tolist(), "full-rotation", full["inliers"].cpu().numpy().ravel()[:4].tolist())


def _search(maps, pose, radius, need, b0s=(0,)):
    """tests/test_guard_gpu.py's search with the axis-only test: the first of REFIT_SETTINGS for which `need(results)` holds."""
    from captra_amd.pose_utils.pose_fit import part_fit_guard_cn
    for th, H in REFIT_SETTINGS:
        res = [part_fit_guard_cn(*maps, pose, inlier_th=th * radius, lost_below=1.0, refit=True, num_hyps=H, seed=0, b0=b0, yaxis_only=True)
               for b0 in b0s]
        print("setting", th, H, "verdicts", [np.bincount(r[1]["verdict"].cpu().numpy().ravel(), minlength=4).tolist() for r in res])
        if need(res):
            return {"refit": True, "lost_below": 1.0, "inlier_th": th, "num_hyps": H, **YAXIS}, res
    raise AssertionError("no setting of REFIT_SETTINGS recovers a part where this test needs one")


@pytest.mark.gpu
def test_sym_refit_step_is_where_recovered_ransac_else_step(device):
    """7. refit: True with yaxis_only on bottle, one track_step from frame 0's annotated pose, guard off and on: at least one part is
    recovered, and the final pose is where(verdict == 3, part_fit_ransac_cn(..., yaxis_only=True), guard-off pose), bit for bit."""
    import torch
    from captra_amd.pose_utils.pose_fit import part_fit_ransac_cn

    def step(g):
        trainer, cfg, data = _model(device, g, 2, 2)
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
    rec = npcs["guard_verdict"] == 3
    assert bool(rec.any()), npcs["guard_verdict"]
    rot, scale, trans, valid, info = part_fit_ransac_cn(maps[0], maps[1], maps[2], num_hyps=model.guard["num_hyps"], inlier_th=model.guard["inlier_th"],
                                                        seed=model.guard["seed"], target_mean=maps[3], yaxis_only=True)
    print("verdicts", npcs["guard_verdict"].cpu().numpy().tolist(), "inliers", npcs["guard_inliers"].cpu().numpy().tolist(), "of",
          npcs["guard_count"].cpu().numpy().tolist(), "ransac", info["num_inliers"].cpu().numpy().tolist())
    assert bool((valid & (info["num_inliers"] > npcs["guard_inliers"]))[rec].all())
    want = {"rotation": torch.where(rec[..., None, None], rot, off["rotation"]), "scale": torch.where(rec, scale, off["scale"]),
            "translation": torch.where(rec[..., None, None], trans, off["translation"])}
    assert not torch.equal(want["rotation"], off["rotation"])
    for k in want:
        _same_bits(on[k].cpu().numpy(), want[k].cpu().numpy(), k)
    for k in ("seg", "nocs"):
        np.testing.assert_array_equal(npcs[k].cpu().numpy(), npcs0[k].cpu().numpy())


@pytest.mark.gpu
def test_sym_lanes_draw_what_the_whole_batch_draws(device):
    """7. B = 32, refit: True with yaxis_only: the whole batch in the eager loop and the two captured lanes (the second one's b0 = 16)
    give equal records and poses, under a setting for which the second lane recovers a part in frame 1 and b0 = 0 gives other bits."""
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
    np.testing.assert_array_equal(lanes["guard"][1]["verdict"][lane1].cpu().numpy(), i16["verdict"].cpu().numpy())
    for k in p16:
        _same_bits(lanes["poses"][1][k][lane1].cpu().numpy(), p16[k].cpu().numpy(), f"lane 1 {k} vs the direct call with b0 = 16")
    assert any(not torch.equal(lanes["poses"][1][k][lane1], p0[k]) for k in p0)


@pytest.mark.gpu
def test_defaults_untouched(device):
    """8. Key absent and key False on bottle: the records are the full-rotation entry's (today's), bit for bit."""
    for extra in ({}, {"yaxis_only": False}):
        model, _, data, on = _run(device, {"refit": False, "lost_below": 0.5, **extra}, 2, 3)
        assert "yaxis_only" not in model.guard
        for i in (1, 2):
            _, info = _direct_record(model, on, data, i, on["poses"][i], False)
            for k in ("count", "inliers", "rms", "verdict"):
                np.testing.assert_array_equal(on["guard"][i][k].cpu().numpy(), info[k].cpu().numpy(), err_msg=f"frame {i} {k}")


@pytest.mark.gpu
def test_pickle_says_which_test_counted(device, tmp_path):
    """The result pickle of a yaxis_only run carries one boolean in the slot of frame 0; the frames' records keep their four keys."""
    import pickle

    import torch
    from captra_amd.eval import guard_table, guard_test_name
    trainer, cfg, data = _model(device, {"refit": False, "lost_below": 0.5, **YAXIS}, 2, 3, experiment_dir=tmp_path / "on")
    torch.manual_seed(4321)
    trainer.test(data, save=True, no_eval=True)
    files = sorted((tmp_path / "on" / "results" / "data").glob("*.pkl"))
    assert len(files) == 2
    with open(files[0], "rb") as f:
        rec = pickle.load(f)["guard"]
    assert set(rec[0]) == {"yaxis_only"} and bool(rec[0]["yaxis_only"]) and len(rec) == 3
    for r in rec[1:]:
        assert set(r) == {"count", "inliers", "rms", "verdict"} and all(np.asarray(v).shape == (1,) for v in r.values())
    assert guard_test_name({"guard": rec}) == "axis-only" and len(guard_table("x", {"guard": rec})) == 1
