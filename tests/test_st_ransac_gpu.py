"""captra_part_fit_st_ransac (csrc/pose_st_ransac.hip) through the C ABI against the float64 judge of tests/st_ransac_judge.py, its
Python wrappers, and the robust fit inside the track loop (track_cfg: {st_fit: {ransac: True}}) on the synthetic trajectories.

A RANSAC result is a function of an inlier SET; the cases come with the preconditions that make that set immune to a 10 % rounding
of any residual (st_ransac_judge.check_batch), so the kernel must select exactly the judge's set, and its scale / translation are
then compared by the rule of tests/test_pose_ransac_gpu.py: at most twice as far from float64 as the float32 mirror, with a floor
of 4 fp32 ulps of the output."""
import pickle

import numpy as np
import pytest

from tests import st_ransac_judge as SJ
from tests.test_pose_readout_gpu import F32_EPS

# case seeds: 2000 + N + 2 per_part + with_mean + 10 sym unless the CPU found that seed's fixture broken (preconditions (a)-(c))
SEEDS = {(4100, False, True, False): 7105, (4096, True, False, True): 7106}
_CASES = {}


def _case(N, per_part, with_mean, sym, **kw):
    """Cases and their judge / mirror results, built once and shared (never modified)."""
    k = (N, per_part, with_mean, sym) + tuple(sorted(kw.items()))
    if k not in _CASES:
        c = SJ.batch_case(N, SEEDS.get((N, per_part, with_mean, sym), 2000 + N + 2 * per_part + with_mean + 10 * sym), per_part, with_mean, sym, **kw)
        _CASES[k] = (c, SJ.judge_batch(c), SJ.judge_batch(c, dt=np.float32))
    return _CASES[k]


def _dev(a, device):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _abi(case, device, ranks="given", seed=0, b0=0, prev=True, shape=None, sym=None):
    """The C ABI on sentinel-filled outputs -> (err, dict of numpy outputs).  ranks: 'given' = the case's, None = NULL (drawn in the
    kernel from `seed`), or an array.  shape = (b, p, n, h) overrides what the arrays say (for the refused shapes)."""
    import torch
    from captra_amd import _lib as L
    B, P, _, N = case["src"].shape
    H = case["ranks"].shape[2]
    r = case["ranks"] if isinstance(ranks, str) else ranks
    d = {k: _dev(case[k], device) for k in ("labels", "src", "tgt", "tgt_mean", "rot")}
    ps, pt = (_dev(case["prev_scale"], device), _dev(case["prev_trans"], device)) if prev else (None, None)
    rk = None if r is None else _dev(np.asarray(r, np.int32), device)
    out = dict(scale=torch.full((B, P), float("nan"), device=device), trans=torch.full((B, P, 3), float("nan"), device=device),
               valid=torch.full((B, P), -7, dtype=torch.int32, device=device), best=torch.full((B, P), -7, dtype=torch.int32, device=device),
               num_inliers=torch.full((B, P), -7, dtype=torch.int32, device=device))
    b_, p_, n_, h_ = shape if shape is not None else (B, P, N, H)
    with torch.cuda.device(device):
        err = L.lib().captra_part_fit_st_ransac(b_, p_, n_, int(case["sym"]) if sym is None else sym, b0, h_, float(case["th"]), L.ptr(d["labels"]),
                                                L.ptr(d["src"]), L.ptr(d["tgt"]), 1 if case["per_part"] else 0, L.ptr(d["tgt_mean"]),
                                                L.ptr(d["rot"]), L.ptr(ps), L.ptr(pt), L.ptr(rk), seed, L.ptr(out["scale"]),
                                                L.ptr(out["trans"]), L.ptr(out["valid"]), L.ptr(out["best"]), L.ptr(out["num_inliers"]),
                                                L.stream_ptr())
    torch.cuda.synchronize(device)
    return err, {k: v.cpu().numpy() for k, v in out.items()}


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, what
    np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32), err_msg=str(what))


def _check(got, case, ranks, ref, mir, name, prev=True):
    """Everything the issue asserts for one launch whose member ranks were `ranks`."""
    B, P = ref["valid"].shape
    np.testing.assert_array_equal(got["num_inliers"], ref["num_inliers"], err_msg=name)
    np.testing.assert_array_equal(got["valid"].astype(bool), ref["valid"], err_msg=name)
    for k in ("scale", "trans"):
        assert np.isfinite(got[k]).all(), (name, k)
    for b in range(B):
        for p in range(P):
            pts, S, T = SJ.members_of(case, b, p)
            tag = (name, b, p, len(pts))
            if len(pts) < 3:
                assert not ref["valid"][b, p] and got["best"][b, p] == 0 and got["num_inliers"][b, p] == 0, tag
            else:
                # the inlier set of the kernel's `best` (any hypothesis at the top score), recomputed in float64 from its samples
                h = int(got["best"][b, p])
                assert 0 <= h < ranks.shape[2], tag
                mask = SJ.inlier_set(case, b, p, pts[np.asarray(ranks[b, p, h]) % len(pts)])
                np.testing.assert_array_equal(mask, ref["inliers"][b, p], err_msg=str(tag))
            if not ref["valid"][b, p]:
                want_s, want_t = (case["prev_scale"][b, p], case["prev_trans"][b, p]) if prev else (np.float32(1), np.zeros(3, np.float32))
                _same_bits(got["scale"][b, p], np.float32(want_s), tag)
                _same_bits(got["trans"][b, p], want_t, tag)
                continue
            assert mir["valid"][b, p], tag
            es, ms = abs(got["scale"][b, p] - ref["scale"][b, p]), abs(mir["scale"][b, p] - ref["scale"][b, p])
            et, mt = np.abs(got["trans"][b, p] - ref["trans"][b, p]).max(), np.abs(mir["trans"][b, p] - ref["trans"][b, p]).max()
            print(f"{tag}: scale err kernel {es:.2e} mirror {ms:.2e}; trans {et:.2e} / {mt:.2e}")
            assert es <= max(2 * ms, 4 * F32_EPS * abs(ref["scale"][b, p])), (tag, es, ms)
            assert et <= max(2 * mt, 4 * F32_EPS * np.abs(ref["trans"][b, p]).max()), (tag, et, mt)


# ============================================================================================================ 1. kernel vs judge
@pytest.mark.gpu
@pytest.mark.parametrize("with_mean", [False, True])
@pytest.mark.parametrize("per_part", [False, True])
@pytest.mark.parametrize("sym", [False, True])
@pytest.mark.parametrize("N", [257, 4096, 4100])
def test_st_ransac_vs_judge(device, N, sym, per_part, with_mean):
    """B = 3, P = 3, H = 64 with the judge's triples (N = 4100: the first size whose coordinates are not staged in LDS): exact inlier
    counts and sets, validity, the pose bounds; parts of 0, 2 and 3 members and the part of gross outliers hold prev_* bit for bit,
    the part of 4 members is valid."""
    case, ref, mir = _case(N, per_part, with_mean, sym)
    err, got = _abi(case, device)
    assert err == 0
    _check(got, case, case["ranks"], ref, mir, f"N={N} sym={sym}")
    counts = [[int((case["labels"][b] == p).sum()) for p in range(3)] for b in range(3)]
    assert counts[1] == [2, 3, 4] and counts[2] == [N, 0, 0]
    v = got["valid"].astype(bool)
    assert v.tolist() == [[True, True, False], [False, False, True], [True, False, False]]
    assert got["num_inliers"][1].tolist() == [0, 3, 4]                                  # three members: found, not valid (count > 3)
    assert got["num_inliers"][0, 2] < 3 and counts[0][2] >= 3                           # gross outliers only


# ============================================================================================================== 2. kernel draws
def _slice(case, sl):
    out = dict(case)
    for k in ("labels", "src", "tgt", "tgt_mean", "rot", "prev_scale", "prev_trans", "ranks"):
        out[k] = None if case[k] is None else np.ascontiguousarray(case[k][sl])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("sym", [False, True])
@pytest.mark.parametrize("b0", [0, 7])
def test_st_ransac_kernel_draws(device, b0, sym):
    """sample_rank = NULL, seed 5: a launch on trajectories [0:1] with b0 and one on [1:3] with b0 + 1 give the bits of the launch on
    all three with b0; best / num_inliers (and everything else) are the judge's on draw_ranks(seed, b0 + b, p, ...)."""
    case, _, _ = _case(257, False, True, sym)
    B, P, H = case["ranks"].shape[:3]
    ranks = np.zeros_like(case["ranks"])
    for b in range(B):
        for p in range(P):
            c = int((case["labels"][b] == p).sum())
            if c >= 3:
                ranks[b, p] = SJ.draw_ranks(5, b0 + b, p, H, c)
    SJ.check_batch(case, ranks, pin=True)
    err, got = _abi(case, device, ranks=None, seed=5, b0=b0)
    assert err == 0
    ref, mir = SJ.judge_batch(case, ranks), SJ.judge_batch(case, ranks, dt=np.float32)
    _check(got, case, ranks, ref, mir, f"b0={b0} sym={sym}")
    np.testing.assert_array_equal(got["best"], ref["best"])
    parts = [_abi(_slice(case, sl), device, ranks=None, seed=5, b0=b0 + sl.start) for sl in (slice(0, 1), slice(1, 3))]
    assert all(e == 0 for e, _ in parts)
    for k in got:
        _same_bits(np.concatenate([g[k] for _, g in parts]), got[k], k)
    if b0:
        _, other = _abi(case, device, ranks=None, seed=5, b0=0)
        assert (other["best"] != got["best"]).any()               # (b0 reaches the draws)


# =============================================================================================== 3. prev_* = NULL, refused shapes
@pytest.mark.gpu
@pytest.mark.parametrize("sym", [False, True])
def test_st_ransac_without_prev_and_refused_shapes(device, sym):
    case, _, _ = _case(257, False, False, sym)
    ref, mir = SJ.judge_batch(case, prev=False), SJ.judge_batch(case, dt=np.float32, prev=False)
    err, got = _abi(case, device, prev=False)
    assert err == 0
    _check(got, case, case["ranks"], ref, mir, f"prev=NULL sym={sym}", prev=False)
    inv = ~got["valid"].astype(bool)
    assert inv.sum() == 5 and (got["scale"][inv] == 1.0).all() and (got["trans"][inv] == 0.0).all()
    for shape, kw in (((3, 9, 257, 64), {}), ((3, 3, 257, 257), {}), ((3, 3, 257, 0), {}), ((3, 3, 16385, 64), {}), ((3, 3, 0, 64), {}),
                      ((3, 3, 257, 64), {"sym": 2}), ((3, 3, 257, 64), {"sym": -1}), ((3, 3, 257, 64), {"b0": -1}),
                      ((3, 3, 257, 64), {"b0": 2 ** 31 - 3})):
        err, got = _abi(case, device, shape=shape, **kw)
        assert err == -1, (shape, kw)
        assert np.isnan(got["scale"]).all() and np.isnan(got["trans"]).all() and all((got[k] == -7).all() for k in ("valid", "best", "num_inliers"))
    err, got = _abi(case, device, shape=(0, 3, 257, 64))
    assert err == 0 and np.isnan(got["scale"]).all()
    err, _ = _abi(case, device, b0=2 ** 31 - 4)                     # b0 = INT_MAX - b: the largest allowed
    assert err == 0


# ================================================================================================== 4. outliers, on the device
@pytest.mark.gpu
@pytest.mark.parametrize("sym", [False, True])
def test_one_pass_fit_misses_what_the_robust_fit_finds(device, sym):
    """The case of test 1 at N = 4096 (30 % gross outliers in every recipe part): captra_part_fit_st_track on the same inputs misses the
    judge's scale by more than 10 % on the recipe parts; captra_part_fit_st_ransac is within rule 1 of it."""
    from captra_amd.pose_utils.pose_fit import part_fit_st_track
    case, ref, mir = _case(4096, False, True, sym)
    err, got = _abi(case, device)
    assert err == 0
    _check(got, case, case["ranks"], ref, mir, f"outliers sym={sym}")
    scale, _, valid = part_fit_st_track(_dev(case["labels"], device), _dev(case["src"], device), _dev(case["tgt"], device),
                                        _dev(case["tgt_mean"], device), _dev(case["rot"], device), _dev(case["prev_scale"], device),
                                        _dev(case["prev_trans"], device).unsqueeze(-1), sym)
    scale = scale.cpu().numpy()
    recipe = [(b, p) for (b, p), tin in case["true_in"].items() if len(tin) >= 40 and (b, p) != case["outlier_part"]]
    assert len(recipe) == 3
    for b, p in recipe:
        plain, robust = abs(scale[b, p] - ref["scale"][b, p]) / ref["scale"][b, p], abs(got["scale"][b, p] - ref["scale"][b, p]) / ref["scale"][b, p]
        print(f"part ({b},{p}) of {len(case['true_in'][b, p])} members: one-pass fit {plain:.3f}, robust fit {robust:.1e} from the judge's scale")
        assert bool(valid[b, p]) and plain > 0.10                     # (the robust fit: rule 1, in _check above)


# ===================================================================================================================== 5. wrappers
@pytest.mark.gpu
@pytest.mark.parametrize("sym", [False, True])
def test_st_ransac_wrappers(device, sym):
    """part_fit_st_ransac_track and part_fit_st_ransac (reference layouts, (B,P,N,3)) return the ABI's bits."""
    import torch
    from captra_amd.pose_utils.pose_fit import part_fit_st_ransac, part_fit_st_ransac_track
    case, _, _ = _case(257, False, True, sym)
    err, got = _abi(case, device)
    assert err == 0
    rk = _dev(case["ranks"], device)
    scale, trans, valid, info = part_fit_st_ransac_track(_dev(case["labels"], device), _dev(case["src"], device), _dev(case["tgt"], device),
                                                         _dev(case["tgt_mean"], device).unsqueeze(-1), _dev(case["rot"], device),
                                                         _dev(case["prev_scale"], device), _dev(case["prev_trans"], device).unsqueeze(-1), sym,
                                                         float(case["th"]), sample_rank=rk)
    assert trans.shape == (3, 3, 3, 1) and valid.dtype == torch.bool and set(info) == {"inliers", "best"}
    _same_bits(scale.cpu().numpy(), got["scale"], "scale")
    _same_bits(trans[..., 0].cpu().numpy(), got["trans"], "trans")
    np.testing.assert_array_equal(valid.cpu().numpy(), got["valid"].astype(bool))
    np.testing.assert_array_equal(info["inliers"].cpu().numpy(), got["num_inliers"])
    np.testing.assert_array_equal(info["best"].cpu().numpy(), got["best"])
    # kernel draws with b0 through the wrapper
    err, drawn = _abi(case, device, ranks=None, seed=5, b0=7)
    s2, t2, _, i2 = part_fit_st_ransac_track(_dev(case["labels"], device), _dev(case["src"], device), _dev(case["tgt"], device),
                                             _dev(case["tgt_mean"], device), _dev(case["rot"], device), _dev(case["prev_scale"], device),
                                             _dev(case["prev_trans"], device), sym, float(case["th"]), seed=5, b0=7)
    assert err == 0
    _same_bits(s2.cpu().numpy(), drawn["scale"], "scale, drawn")
    _same_bits(t2[..., 0].cpu().numpy(), drawn["trans"], "trans, drawn")
    np.testing.assert_array_equal(i2["best"].cpu().numpy(), drawn["best"])
    # the reference layouts: a target per part, no previous pose
    case, _, _ = _case(257, True, True, sym)
    err, got = _abi(case, device, prev=False)
    assert err == 0
    rot = _dev(case["rot"], device)
    model, valid = part_fit_st_ransac(_dev(case["labels"].astype(np.int64), device), _dev(case["src"].transpose(0, 1, 3, 2), device),
                                      _dev(case["tgt"].transpose(0, 1, 3, 2), device), rot, {"num_parts": 3, "sym": sym},
                                      inlier_th=float(case["th"]), sample_rank=_dev(case["ranks"], device),
                                      target_mean=_dev(case["tgt_mean"], device))
    assert model["rotation"] is rot and model["translation"].shape == (3, 3, 3, 1)
    _same_bits(model["scale"].cpu().numpy(), got["scale"], "scale, reference layout")
    _same_bits(model["translation"][..., 0].cpu().numpy(), got["trans"], "trans, reference layout")
    np.testing.assert_array_equal(valid.cpu().numpy(), got["valid"].astype(bool))


# =================================================================================================================== 6. in the loop
ALL_INLIERS = 10.0          # inlier_th as a fraction of data_radius under which every member is an inlier (6 m at the crops' 0.6 m)


def _model(device, tag, st_fit, guard=None, hipgraph=False, experiment_dir="/tmp/captra_test_exp"):
    from captra_amd import synthetic as clouds
    from captra_amd.configs import make_config
    from captra_amd.trainer import Trainer
    cat, objcfg, kind, _, _, wseed, _ = clouds.PHYSICAL_SETUPS[tag]
    cfg = make_config(cat, objcfg, experiment_dir=str(experiment_dir))
    if st_fit is not None:
        cfg["track_cfg"]["st_fit"] = dict(st_fit)
    if guard is not None:
        cfg["track_cfg"]["guard"] = dict(guard)
    cfg["hipgraph"] = hipgraph
    trainer = Trainer(cfg)
    shapes = {k: tuple(v.shape) for k, v in trainer.model.state_dict().items()}
    trainer.model.load_state_dict(clouds.make_physical_state_dict(shapes, wseed, cfg["num_parts"], bool(cfg["obj_sym"]), kind))
    B, T = {"bottle": (4, 4), "drawers": (2, 3)}[tag]
    return trainer, cfg, clouds.make_trajectory(kind, B, T, seed=7)


def _run(device, tag, st_fit, guard=None, hipgraph=False):
    import torch
    trainer, cfg, data = _model(device, tag, st_fit, guard, hipgraph)
    torch.manual_seed(4321)
    pred, _ = trainer.test(data, save=False, no_eval=True)
    return trainer.model, cfg, data, pred


def _frame_maps(pred, data, i, B, P):
    import torch
    npcs = pred["npcs_pred"][i]
    labels = torch.argmax(npcs["seg"], dim=-2).int().contiguous()
    src = npcs["nocs"].reshape(B, P, 3, -1).float().contiguous()
    return labels, src, data[i]["points"].float().to(src.device).contiguous(), data[i]["meta"]["points_mean"].float().to(src.device)


def _manual_loop(model, data, form):
    """The frames of `data` from frame 0's annotated pose, never in the few-trajectory split-k form: 'eager' = track_step on each half
    of the batch with its b0 (the two lanes one after the other, not captured), 'lanes' = graph.TrackLanes of two.
    -> [(pose, record, maps)] of frames 1.., batch-wide."""
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
            out.append((pose, {k: npcs["st_" + k].clone() for k in ("inliers", "valid")}, {k: npcs[k].clone() for k in ("seg", "nocs")}))
    torch.cuda.synchronize()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("th", [ALL_INLIERS, None], ids=["all_inliers", "default_th"])
@pytest.mark.parametrize("tag", ["bottle", "drawers"])
def test_robust_fit_in_the_loop(device, tag, th):
    """Every frame's scale / translation / record is the wrapper's on that frame's own maps, rotation and previous pose, bit for bit;
    invalid parts carry the previous values; the captured step gives the eager step's bits; so do two lanes of the batch."""
    import torch
    from captra_amd.graph import TrackStepGraph
    from captra_amd.pose_utils.pose_fit import part_fit_st_ransac_track
    st = {"ransac": True} if th is None else {"ransac": True, "inlier_th": th}
    model, cfg, data, pred = _run(device, tag, st)
    assert model.st_fit is not None and len(pred["st_fit"]) == len(data) and pred["st_fit"][0] is None
    B, P = pred["poses"][0]["scale"].shape
    assert (B, P) == {"bottle": (4, 1), "drawers": (2, 4)}[tag]
    for i in range(1, len(data)):
        rec, pose, last = pred["st_fit"][i], pred["poses"][i], pred["poses"][i - 1]
        assert set(rec) == {"inliers", "valid"} and all(v.shape == (B, P) and v.dtype == torch.int32 for v in rec.values())
        assert not any(k.startswith("st_") for k in pred["npcs_pred"][i])
        labels, src, pts, mean = _frame_maps(pred, data, i, B, P)
        scale, trans, valid, info = part_fit_st_ransac_track(labels, src, pts, mean, pose["rotation"].float().contiguous(), last["scale"],
                                                             last["translation"], bool(cfg["obj_sym"]), model.st_fit["inlier_th"],
                                                             num_hyps=model.st_fit["num_hyps"], seed=model.st_fit["seed"], b0=0)
        _same_bits(pose["scale"].cpu().numpy(), scale.cpu().numpy(), f"frame {i} scale")
        _same_bits(pose["translation"].cpu().numpy(), trans.cpu().numpy(), f"frame {i} translation")
        np.testing.assert_array_equal(rec["inliers"].cpu().numpy(), info["inliers"].cpu().numpy())
        np.testing.assert_array_equal(rec["valid"].cpu().numpy(), valid.int().cpu().numpy())
        held = ~valid
        assert torch.equal(pose["scale"][held], last["scale"][held]) and torch.equal(pose["translation"][held], last["translation"][held])
        members = (labels[:, None, :] == torch.arange(P, device=labels.device)[None, :, None]).sum(-1)
        print(tag, "frame", i, "inliers", rec["inliers"].cpu().numpy().tolist(), "of", members.cpu().numpy().tolist(), "valid", rec["valid"].cpu().numpy().tolist())
        if th is not None:
            assert bool(valid.all()) and torch.equal(rec["inliers"], members.int())
        assert all(bool(torch.isfinite(v).all()) for v in pose.values())
    # the captured step, through the model's own loop
    gmodel, _, _, gpred = _run(device, tag, st, hipgraph=True)
    assert isinstance(gmodel._graph, TrackStepGraph)
    for i in range(1, len(data)):
        for k in pred["poses"][i]:
            _same_bits(gpred["poses"][i][k].cpu().numpy(), pred["poses"][i][k].cpu().numpy(), f"hipgraph frame {i} {k}")
        for k in ("inliers", "valid"):
            np.testing.assert_array_equal(gpred["st_fit"][i][k].cpu().numpy(), pred["st_fit"][i][k].cpu().numpy())
    # two lanes of the batch (the second one's b0 = B / 2), captured and free-running, against the same halves stepped eagerly: every
    # pose and record bit for bit; and the second lane IS the wrapper on its own maps with ITS b0.  (The whole batch of four is not
    # the yardstick here: a sub-batch of one or two trajectories takes the step's latency-bound schedule (model.py:
    # _fork_rotation_net), and measured on the MI355X RotationNet's rotation of a lane of two is one ulp from the whole batch's --
    # upstream of the fit, which then fits other bits.)
    forms = {form: _manual_loop(model, data, form) for form in ("eager", "lanes")}
    for i, ((pa, ra, ma), (pb, rb, mb)) in enumerate(zip(forms["eager"], forms["lanes"])):
        for k in pa:
            _same_bits(pb[k].cpu().numpy(), pa[k].cpu().numpy(), f"lanes frame {i + 1} {k}")
        for k in ra:
            np.testing.assert_array_equal(rb[k].cpu().numpy(), ra[k].cpu().numpy(), err_msg=f"lanes frame {i + 1} {k}")
    h = B // 2
    last = {k: v.to(pb[k].device) for k, v in model.feed_dict[0]["gt_part"].items()}
    for i, (pb, rb, mb) in enumerate(forms["lanes"], start=1):
        labels = torch.argmax(mb["seg"], dim=-2).int()[h:].contiguous()
        src = mb["nocs"].reshape(B, P, 3, -1).float()[h:].contiguous()
        pts, mean = model.feed_dict[i]["points"][h:].float().contiguous(), model.feed_dict[i]["points_mean"][h:]
        scale, trans, valid, info = part_fit_st_ransac_track(labels, src, pts, mean, pb["rotation"][h:].float().contiguous(), last["scale"][h:],
                                                             last["translation"][h:], bool(cfg["obj_sym"]), model.st_fit["inlier_th"],
                                                             num_hyps=model.st_fit["num_hyps"], seed=model.st_fit["seed"], b0=h)
        _same_bits(pb["scale"][h:].cpu().numpy(), scale.cpu().numpy(), f"second lane, frame {i} scale")
        _same_bits(pb["translation"][h:].cpu().numpy(), trans.cpu().numpy(), f"second lane, frame {i} translation")
        np.testing.assert_array_equal(rb["inliers"][h:].cpu().numpy(), info["inliers"].cpu().numpy())
        np.testing.assert_array_equal(rb["valid"][h:].cpu().numpy(), valid.int().cpu().numpy())
        last = pb


@pytest.mark.gpu
def test_guard_judges_the_robust_fits_pose(device):
    """Guard (monitoring) and robust fit both on: the poses are those of the robust fit alone, and the guard's record is
    part_fit_guard_cn's on each frame's maps and THAT pose."""
    from captra_amd.pose_utils.pose_fit import part_fit_guard_cn
    guard = {"refit": False, "lost_below": 0.5, "yaxis_only": True}
    _, _, _, alone = _run(device, "bottle", {"ransac": True})
    model, cfg, data, both = _run(device, "bottle", {"ransac": True}, guard=guard)
    B, P = both["poses"][0]["scale"].shape
    g = model.guard
    for i in range(1, len(data)):
        for k in both["poses"][i]:
            _same_bits(both["poses"][i][k].cpu().numpy(), alone["poses"][i][k].cpu().numpy(), f"frame {i} {k}")
        for k in ("inliers", "valid"):
            np.testing.assert_array_equal(both["st_fit"][i][k].cpu().numpy(), alone["st_fit"][i][k].cpu().numpy())
        labels, src, pts, mean = _frame_maps(both, data, i, B, P)
        _, info = part_fit_guard_cn(labels, src, pts, mean, both["poses"][i], inlier_th=g["inlier_th"], lost_below=g["lost_below"],
                                    min_members=g["min_members"], refit=False, num_hyps=g["num_hyps"], seed=g["seed"], yaxis_only=True)
        for k in ("count", "inliers", "rms", "verdict"):
            np.testing.assert_array_equal(both["guard"][i][k].cpu().numpy(), info[k].cpu().numpy(), err_msg=f"frame {i} {k}")


@pytest.mark.gpu
def test_layer_by_layer_path_takes_the_robust_fit(device):
    """PartCanonNet.forward without the fused rotation read-out (fused.USE_ROT_READOUT off): the robust fit's record, and the pose the
    wrapper gives on the step's own maps and rotation."""
    import torch
    from captra_amd import fused
    from captra_amd.pose_utils.pose_fit import part_fit_st_ransac_track
    trainer, cfg, data = _model(device, "drawers", {"ransac": True})
    model = trainer.model
    model.set_data(data)
    last = {k: v.clone() for k, v in model.feed_dict[0]["gt_part"].items()}
    old = fused.USE_ROT_READOUT
    fused.USE_ROT_READOUT = False
    try:
        with torch.no_grad():
            npcs, pose = model.track_step(model.feed_dict[1], model.npcs_feed_dict[1], last)
    finally:
        fused.USE_ROT_READOUT = old
    B, P = pose["scale"].shape
    labels = torch.argmax(npcs["seg"], dim=-2).int().contiguous()
    src = npcs["nocs"].reshape(B, P, 3, -1).float().contiguous()
    feed = model.feed_dict[1]
    scale, trans, valid, info = part_fit_st_ransac_track(labels, src, feed["points"].float().contiguous(), feed["points_mean"],
                                                         pose["rotation"].float().contiguous(), last["scale"], last["translation"], False,
                                                         model.st_fit["inlier_th"], num_hyps=model.st_fit["num_hyps"], seed=model.st_fit["seed"])
    _same_bits(pose["scale"].cpu().numpy(), scale.cpu().numpy(), "scale")
    _same_bits(pose["translation"].cpu().numpy(), trans.cpu().numpy(), "translation")
    np.testing.assert_array_equal(npcs["st_inliers"].cpu().numpy(), info["inliers"].cpu().numpy())
    np.testing.assert_array_equal(npcs["st_valid"].cpu().numpy(), valid.int().cpu().numpy())


# ========================================================================================================== 7. off changes nothing
@pytest.mark.gpu
def test_off_changes_nothing(device, tmp_path):
    """No key and ransac: False: the same poses bit for bit, the parent's pred_dict and pickle keys, and no launch of the new
    kernel among the profiler's kernel names (the one-pass fit's is there); on: the pickles gain 'st_fit' and nothing else."""
    import torch
    from captra_amd import _lib
    runs, keys = {}, {}
    for name, st in (("absent", None), ("false", {"ransac": False, "num_hyps": 16}), ("on", {"ransac": True})):
        trainer, cfg, data = _model(device, "bottle", st, experiment_dir=tmp_path / name)
        assert (trainer.model.st_fit is not None) == (name == "on")
        torch.manual_seed(4321)
        _lib.prof_enable(True)
        _lib.prof_reset()
        try:
            pred, _ = trainer.test(data, save=True, no_eval=True)
            torch.cuda.synchronize()
            names = set(_lib.prof_names())
        finally:
            _lib.prof_enable(False)
        # (the off runs come first: the profiler keeps the names it has met while it was enabled)
        assert any("part_fit_st_ransac" in n for n in names) == (name == "on"), names
        assert name == "on" or "part_fit_st" in names, names
        files = sorted((tmp_path / name / "results" / "data").glob("*.pkl"))
        assert len(files) == 4
        with open(files[0], "rb") as f:
            keys[name] = pickle.load(f)
        runs[name] = (pred, torch.rand(3))
    for name in ("absent", "false"):
        assert set(runs[name][0]) == {"poses", "npcs_pred"} and set(keys[name]) == {"pred", "gt", "frame_nums"}
    for a, b in zip(runs["absent"][0]["poses"], runs["false"][0]["poses"]):
        for k in a:
            _same_bits(a[k].cpu().numpy(), b[k].cpu().numpy(), k)
    for a, b in zip(runs["absent"][0]["npcs_pred"][1:], runs["false"][0]["npcs_pred"][1:]):
        assert set(a) == set(b)
    assert torch.equal(runs["absent"][1], runs["false"][1])                 # the same random-number consumption
    assert set(runs["on"][0]) == {"poses", "npcs_pred", "st_fit"} and set(keys["on"]) == {"pred", "gt", "frame_nums", "st_fit"}
    rec = keys["on"]["st_fit"]
    assert rec[0] is None and len(rec) == 4
    for r in rec[1:]:
        assert set(r) == {"inliers", "valid"} and all(np.asarray(v).shape == (1,) for v in r.values())
