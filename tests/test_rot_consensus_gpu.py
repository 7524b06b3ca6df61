"""captra_rot_pool_consensus (csrc/rot_consensus.hip) through the C ABI against the float64 judge of tests/rot_consensus_judge.py, its
Python wrapper, and the consensus read-out inside the track loop (track_cfg: {rot_pool: {consensus: True, angle_th: ...}}) on the
synthetic trajectories.

The result is a function of an inlier SET; the cases come with the preconditions that make that set immune to a rounding of 10 %
of the threshold (rot_consensus_judge.check_batch), so the kernel must select exactly the judge's set, and its dR / rotation are
then compared by the rule of tests/test_pose_ransac_gpu.py: at most twice as far from float64 as the float32 mirror, with a floor
of 4 fp32 ulps of the output (F32_EPS of tests/test_pose_readout_gpu.py times the largest entry of the 3x3 output).

The part whose members' raw is all NaN: the vote of such a member is, by the read-out's own normalize3, finite -- (1,0,0) for a
symmetric category, the degenerate frame x = z = (1,0,0), y = 0 otherwise.  Without symmetry no such vote is an inlier even of
itself (trace 2 < 1 + 2 cos 15 deg): num_inliers = 0 and dR is the identity.  With symmetry every such vote agrees with every other
(d = 1), so num_inliers = count and dR is what captra_rot_pool_compose gives on the same input; the judge says the same, and the
tests below assert each of the two."""
import pickle

import numpy as np
import pytest

from tests import rot_consensus_judge as RJ
from tests.test_pose_readout_gpu import F32_EPS

H = 64
INT_MAX = 2**31 - 1
_CASES = {}


def _case(N, sym, **kw):
    """Cases and their judge / mirror results, built once and shared (never modified)."""
    k = (N, sym) + tuple(sorted(kw.items()))
    if k not in _CASES:
        c = RJ.batch_case(N, 3000 + N + 10 * sym, sym, num_hyps=H, **kw)
        _CASES[k] = (c, RJ.judge_batch(c), RJ.judge_batch(c, dt=np.float32))
    return _CASES[k]


def _dev(a, device):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _abi(case, device, ranks="given", seed=0, b0=0, shape=None, sym=None, diag=None, cos_th=None, sl=slice(None), fn="consensus"):
    """The C ABI on sentinel-filled outputs -> (err, dict of numpy outputs).  ranks: 'given' = the case's, None = NULL (drawn in the
    kernel from `seed`).  shape = (b, p, n, h) overrides what the arrays say (for the refused arguments); sl: the trajectories
    launched; fn = 'compose': captra_rot_pool_compose on the same inputs."""
    import torch
    from captra_amd import _lib as L
    P = case["ranks"].shape[1]
    labels, prev, rk = case["labels"][sl], case["prev_rot"][sl], case["ranks"][sl]
    B, N = labels.shape
    raw = case["raw"].reshape((case["ranks"].shape[0], P) + case["raw"].shape[1:])[sl]
    d = dict(labels=_dev(labels, device), raw=_dev(raw, device), prev=_dev(prev, device))
    rkd = _dev(rk, device) if isinstance(ranks, str) else None
    out = dict(rot=torch.full((B, P, 3, 3), float("nan"), device=device), delta=torch.full((B, P, 3, 3), float("nan"), device=device),
               count=torch.full((B, P), -7, dtype=torch.int32, device=device), num_inliers=torch.full((B, P), -7, dtype=torch.int32, device=device),
               best=torch.full((B, P), -7, dtype=torch.int32, device=device))
    b_, p_, n_, h_ = shape if shape is not None else (B, P, N, H)
    sym_ = int(case["sym"]) if sym is None else sym
    diag_ = int(case["diag"]) if diag is None else diag
    with torch.cuda.device(device):
        if fn == "compose":
            err = L.lib().captra_rot_pool_compose(b_, p_, n_, sym_, diag_, L.ptr(d["raw"]), L.ptr(d["labels"]), L.ptr(d["prev"]),
                                                  L.ptr(out["rot"]), L.ptr(out["delta"]), L.stream_ptr())
        else:
            c = float(RJ.cos_th_of(case["th_deg"])) if cos_th is None else cos_th
            err = L.lib().captra_rot_pool_consensus(b_, p_, n_, sym_, diag_, b0, h_, c, L.ptr(d["raw"]), L.ptr(d["labels"]), L.ptr(d["prev"]),
                                                    L.ptr(rkd), seed, L.ptr(out["rot"]), L.ptr(out["delta"]), L.ptr(out["count"]),
                                                    L.ptr(out["num_inliers"]), L.ptr(out["best"]), L.stream_ptr())
    torch.cuda.synchronize(device)
    return err, {k: v.cpu().numpy() for k, v in out.items()}


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, what
    np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32), err_msg=str(what))


def _check(got, case, ranks, ref, mir, name):
    """Everything the issue asserts for one launch whose member ranks were `ranks` (B,P,H)."""
    B, P = ref["count"].shape
    for k in ("count", "num_inliers", "best"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=f"{name} {k}")
    for k in ("rot", "delta"):
        assert np.isfinite(got[k]).all(), (name, k)
    for b in range(B):
        for p in range(P):
            pts, _ = RJ.members_of(case, b, p)
            tag = (name, b, p, len(pts))
            if len(pts):
                h = int(got["best"][b, p])
                assert 0 <= h < ranks.shape[2], tag
                np.testing.assert_array_equal(RJ.inlier_set(case, b, p, int(ranks[b, p, h])), ref["inliers"][b, p], err_msg=str(tag))
            for k in ("delta", "rot"):
                e, m = np.abs(got[k][b, p] - ref[k][b, p]).max(), np.abs(mir[k][b, p] - ref[k][b, p]).max()
                print(f"{tag}: {k} err kernel {e:.2e} mirror {m:.2e}")
                assert e <= max(2 * m, 4 * F32_EPS * np.abs(ref[k][b, p]).max()), (tag, k, e, m)


# ============================================================================================================ 1. kernel vs judge
# N = 4096 is one scoring round of the workgroup (1024 lanes x 4 points), 4100 the first N of two rounds, 16384 the limit; the
# kernel has no other regime (the votes of a round live in registers at every N)
@pytest.mark.gpu
@pytest.mark.parametrize("sym", [False, True])
@pytest.mark.parametrize("N,diag", [(257, True), (257, False), (4096, True), (4100, True), (16384, True)])
def test_consensus_vs_judge(device, N, diag, sym):
    case, ref, mir = _case(N, sym, diag=diag)
    err, got = _abi(case, device)
    assert err == 0
    _check(got, case, case["ranks"], ref, mir, f"N={N} sym={sym} diag={diag}")
    # trajectory 1: no member (default), one member, two members
    assert ref["count"][1].tolist() == [0, 1, 2] and got["num_inliers"][1].tolist() == [0, 1, 2]
    assert got["count"][2].tolist() == [N, 0, 0]
    b, p = case["nan_part"]
    _, plain = _abi(case, device, fn="compose")
    if sym:         # (module docstring) every NaN member votes (1,0,0): all agree, the plain read-out's bits
        assert got["num_inliers"][b, p] == got["count"][b, p] > 0
        _same_bits(got["delta"][b, p], plain["delta"][b, p], "NaN part, sym")
    else:
        assert got["num_inliers"][b, p] == 0 and got["count"][b, p] > 0
        _same_bits(got["delta"][b, p], np.eye(3, dtype=np.float32), "NaN part")
        _same_bits(got["rot"][b, p], case["prev_rot"][b, p] @ np.eye(3, dtype=np.float32), "NaN part rot")
    # empty parts: the default dR, exactly as the plain read-out writes it
    for (bb, pp) in ((1, 0), (2, 1), (2, 2)):
        _same_bits(got["delta"][bb, pp], plain["delta"][bb, pp], "empty part")
        _same_bits(got["rot"][bb, pp], plain["rot"][bb, pp], "empty part rot")
    # 3b: the part of one member: its dR is that vote's frame by the plain kernel
    _same_bits(got["delta"][1, 1], plain["delta"][1, 1], "one member")
    _same_bits(got["rot"][1, 1], plain["rot"][1, 1], "one member rot")


# =============================================================================================================== 2. kernel draws
@pytest.mark.gpu
@pytest.mark.parametrize("sym", [False, True])
def test_consensus_kernel_draws(device, sym):
    case, _, _ = _case(257, sym, diag=True)
    B, P = case["ranks"].shape[:2]
    bests = {}
    for b0 in (0, 7):
        ranks = np.zeros((B, P, H), np.int64)
        for b in range(B):
            for p in range(P):
                ranks[b, p] = RJ.hyp_ranks(5, b0 + b, p, H, int((case["labels"][b] == p).sum()))
        RJ.check_batch(case, ranks, pin=True)
        ref, mir = RJ.judge_batch(case, ranks), RJ.judge_batch(case, ranks, dt=np.float32)
        err, whole = _abi(case, device, ranks=None, seed=5, b0=b0)
        assert err == 0
        _check(whole, case, ranks, ref, mir, f"draws b0={b0} sym={sym}")
        e0, first = _abi(case, device, ranks=None, seed=5, b0=b0, sl=slice(0, 1))
        e1, rest = _abi(case, device, ranks=None, seed=5, b0=b0 + 1, sl=slice(1, 3))
        assert e0 == 0 and e1 == 0
        for k in whole:
            got = np.concatenate([first[k], rest[k]])
            if got.dtype == np.float32:
                _same_bits(got, whole[k], (b0, k))
            else:
                np.testing.assert_array_equal(got, whole[k], err_msg=str((b0, k)))
        bests[b0] = whole["best"]
    assert (bests[0] != bests[7]).any()


# ============================================================================================== 3. all inliers is the plain read-out
@pytest.mark.gpu
@pytest.mark.parametrize("sym", [False, True])
@pytest.mark.parametrize("N,diag", [(257, False), (4100, True)])
def test_all_inliers_is_the_plain_readout(device, N, diag, sym):
    case, ref, mir = _case(N, sym, diag=diag, outliers=False, th_deg=60.0, nan_part=None)
    err, got = _abi(case, device)
    e2, plain = _abi(case, device, fn="compose")
    assert err == 0 and e2 == 0
    np.testing.assert_array_equal(got["num_inliers"], got["count"])
    np.testing.assert_array_equal(got["count"], ref["count"])
    _same_bits(got["rot"], plain["rot"], "rot")
    _same_bits(got["delta"], plain["delta"], "delta")


# ======================================================================================================= 4. what the mean misses
@pytest.mark.gpu
@pytest.mark.parametrize("sym", [False, True])
def test_plain_mean_misses_what_the_consensus_finds(device, sym):
    case, ref, mir = _case(4096, sym, diag=True)
    err, got = _abi(case, device)
    _, plain = _abi(case, device, fn="compose")
    assert err == 0
    _check(got, case, case["ranks"], ref, mir, f"misses sym={sym}")
    for (b, p), tin in case["true_in"].items():
        if b == 1 or tin is None:
            continue
        Rt = case["R_true"][b, p]

        def off(dR):
            c = dR[:, 1] @ Rt[:, 1] if sym else (np.trace(Rt.T @ dR.astype(np.float64)) - 1) / 2
            return float(np.rad2deg(np.arccos(np.clip(c, -1, 1))))
        print(f"part {(b, p)}: plain read-out {off(plain['delta'][b, p]):.2f} deg from R_true, consensus {off(got['delta'][b, p]):.2f} deg")
        assert off(plain["delta"][b, p]) > 5.0, (b, p)


# ============================================================================================================ 5. refused arguments
@pytest.mark.gpu
def test_consensus_refused_arguments(device):
    case, _, _ = _case(257, False, diag=True)
    B, P, N = 3, 3, 257
    c15 = float(RJ.cos_th_of(15.0))
    refused = [dict(shape=(B, 0, N, H)), dict(shape=(B, 9, N, H)), dict(shape=(B, P, N, 0)), dict(shape=(B, P, N, 257)), dict(shape=(B, P, 0, H)),
               dict(shape=(B, P, 16385, H)), dict(sym=2), dict(sym=-1), dict(diag=2), dict(diag=-1), dict(b0=-1), dict(b0=INT_MAX - B + 1),
               dict(cos_th=1.0), dict(cos_th=-1.0), dict(cos_th=1.5), dict(cos_th=float("nan")), dict(shape=(-1, P, N, H))]
    for kw in refused:
        err, got = _abi(case, device, **kw)
        assert err == -1, kw
        assert np.isnan(got["rot"]).all() and np.isnan(got["delta"]).all(), kw
        assert all((got[k] == -7).all() for k in ("count", "num_inliers", "best")), kw
    err, got = _abi(case, device, shape=(0, P, N, H))
    assert err == 0 and np.isnan(got["rot"]).all() and (got["count"] == -7).all()
    err, got = _abi(case, device, b0=INT_MAX - B)
    assert err == 0 and np.isfinite(got["rot"]).all() and c15 < 1.0


# ======================================================================================================================= 6. wrapper
@pytest.mark.gpu
@pytest.mark.parametrize("sym", [False, True])
def test_consensus_wrapper(device, sym):
    from captra_amd import fused
    case, _, _ = _case(257, sym, diag=False)
    raw, labels, prev = _dev(case["raw"], device), _dev(case["labels"], device), _dev(case["prev_rot"], device)
    _, got = _abi(case, device)
    rot, delta, info = fused.rot_pool_consensus(raw, labels, prev, sym, case["th_deg"], num_hyps=H, sample_rank=_dev(case["ranks"], device),
                                                want_delta=True)
    _same_bits(rot.cpu().numpy(), got["rot"], "rot")
    _same_bits(delta.cpu().numpy(), got["delta"], "delta")
    assert set(info) == {"count", "inliers", "best"}
    for k, g in (("count", "count"), ("inliers", "num_inliers"), ("best", "best")):
        assert info[k].dtype.is_floating_point is False and info[k].shape == (3, 3)
        np.testing.assert_array_equal(info[k].cpu().numpy(), got[g])
    _, drawn = _abi(case, device, ranks=None, seed=5, b0=7)
    rot, info = fused.rot_pool_consensus(raw, labels, prev, sym, case["th_deg"], num_hyps=H, seed=5, b0=7)
    _same_bits(rot.cpu().numpy(), drawn["rot"], "rot, kernel draws")
    np.testing.assert_array_equal(info["best"].cpu().numpy(), drawn["best"])
    np.testing.assert_array_equal(info["inliers"].cpu().numpy(), drawn["num_inliers"])


# =================================================================================================================== 7. in the loop
TH_LOOP = 30.0          # degrees; a test setting only


def _model(device, tag, rot_pool, st_fit=None, guard=None, hipgraph=False, experiment_dir="/tmp/captra_test_exp"):
    from captra_amd import synthetic as clouds
    from captra_amd.configs import make_config
    from captra_amd.trainer import Trainer
    cat, objcfg, kind, _, _, wseed, _ = clouds.PHYSICAL_SETUPS[tag]
    cfg = make_config(cat, objcfg, experiment_dir=str(experiment_dir))
    for key, val in (("rot_pool", rot_pool), ("st_fit", st_fit), ("guard", guard)):
        if val is not None:
            cfg["track_cfg"][key] = dict(val)
    cfg["hipgraph"] = hipgraph
    trainer = Trainer(cfg)
    shapes = {k: tuple(v.shape) for k, v in trainer.model.state_dict().items()}
    trainer.model.load_state_dict(clouds.make_physical_state_dict(shapes, wseed, cfg["num_parts"], bool(cfg["obj_sym"]), kind))
    B, T = {"bottle": (4, 4), "drawers": (2, 3)}[tag]
    return trainer, cfg, clouds.make_trajectory(kind, B, T, seed=7)


def _run(device, tag, rot_pool, hipgraph=False, **kw):
    import torch
    trainer, cfg, data = _model(device, tag, rot_pool, hipgraph=hipgraph, **kw)
    torch.manual_seed(4321)
    pred, _ = trainer.test(data, save=False, no_eval=True)
    return trainer.model, cfg, data, pred


class _Spy:
    """Around fused.rot_pool_consensus: every call's arguments (cloned) and results."""

    def __init__(self):
        from captra_amd import fused
        self.fused, self.real, self.calls = fused, fused.rot_pool_consensus, []

    def __enter__(self):
        def spy(raw, labels, prev, sym, angle, **kw):
            res = self.real(raw, labels, prev, sym, angle, **kw)
            self.calls.append(dict(raw=raw.clone(), labels=labels.clone(), prev=prev.clone(), sym=sym, angle=angle, kw=dict(kw),
                                   rot=res[0].clone(), info={k: v.clone() for k, v in res[-1].items()}))
            return res
        self.fused.rot_pool_consensus = spy
        return self

    def __exit__(self, *a):
        self.fused.rot_pool_consensus = self.real


def _manual_loop(model, data, form):
    """As in tests/test_st_ransac_gpu.py: 'eager' = track_step on each half of the batch with its b0, 'lanes' = graph.TrackLanes of
    two.  -> [(pose, record)] of frames 1.., batch-wide."""
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
            out.append((pose, {k: npcs["rot_" + k].clone() for k in ("inliers", "count")}))
    torch.cuda.synchronize()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["bottle", "drawers"])
def test_consensus_in_the_loop(device, tag):
    """Every frame's rotation and record are those of the one call of the wrapper in that step; where every member is an inlier the
    plain read-out gives the same bits on the call's inputs; the captured step gives the eager step's bits; so do two lanes."""
    import torch
    from captra_amd import fused
    from captra_amd.graph import TrackStepGraph
    rp = {"consensus": True, "angle_th": TH_LOOP}
    with _Spy() as spy:
        model, cfg, data, pred = _run(device, tag, rp)
    assert model.rot_pool == {"angle_th": TH_LOOP, "num_hyps": 64, "seed": 0} and model.net.rot_pool is model.rot_pool
    assert len(pred["rot_pool"]) == len(data) and pred["rot_pool"][0] is None
    B, P = pred["poses"][0]["scale"].shape
    assert (B, P) == {"bottle": (4, 1), "drawers": (2, 4)}[tag]
    assert len(spy.calls) == len(data) - 1
    sym = bool(cfg["obj_sym"])
    for i in range(1, len(data)):
        call, rec, pose = spy.calls[i - 1], pred["rot_pool"][i], pred["poses"][i]
        assert call["kw"].get("b0", 0) == 0 and call["sym"] == sym and call["angle"] == TH_LOOP and call["kw"].get("sample_rank") is None
        assert set(rec) == {"inliers", "count"} and all(v.shape == (B, P) and v.dtype == torch.int32 for v in rec.values())
        assert not any(k.startswith("rot_") for k in pred["npcs_pred"][i])
        _same_bits(pose["rotation"].cpu().numpy(), call["rot"].cpu().numpy(), f"frame {i} rotation")
        assert torch.equal(rec["inliers"], call["info"]["inliers"]) and torch.equal(rec["count"], call["info"]["count"])
        labels = torch.argmax(pred["npcs_pred"][i]["seg"], dim=-2).int()
        assert torch.equal(labels, call["labels"])
        members = (labels[:, None, :] == torch.arange(P, device=labels.device)[None, :, None]).sum(-1).int()
        assert torch.equal(rec["count"], members)
        assert bool(((rec["inliers"] >= 0) & (rec["inliers"] <= rec["count"])).all())
        print(tag, "frame", i, "inliers", rec["inliers"].cpu().numpy().tolist(), "of", rec["count"].cpu().numpy().tolist())
        plain = fused.rot_pool_compose(call["raw"], call["labels"], call["prev"], sym)
        full = rec["inliers"] == rec["count"]
        assert torch.equal(plain[full], call["rot"][full])
        assert all(bool(torch.isfinite(v).all()) for v in pose.values())
    # the captured step, through the model's own loop
    gmodel, _, _, gpred = _run(device, tag, rp, hipgraph=True)
    assert isinstance(gmodel._graph, TrackStepGraph)
    for i in range(1, len(data)):
        for k in pred["poses"][i]:
            _same_bits(gpred["poses"][i][k].cpu().numpy(), pred["poses"][i][k].cpu().numpy(), f"hipgraph frame {i} {k}")
        for k in ("inliers", "count"):
            np.testing.assert_array_equal(gpred["rot_pool"][i][k].cpu().numpy(), pred["rot_pool"][i][k].cpu().numpy())
    # two lanes of the batch (the second one's b0 = B / 2) against the same halves stepped eagerly with their b0
    with _Spy() as spy:
        eager = _manual_loop(model, data, "eager")
    assert [c["kw"].get("b0", 0) for c in spy.calls] == [0, B // 2] * (len(data) - 1)
    lanes = _manual_loop(model, data, "lanes")
    for i, ((pa, ra), (pb, rb)) in enumerate(zip(eager, lanes)):
        for k in pa:
            _same_bits(pb[k].cpu().numpy(), pa[k].cpu().numpy(), f"lanes frame {i + 1} {k}")
        for k in ra:
            np.testing.assert_array_equal(rb[k].cpu().numpy(), ra[k].cpu().numpy(), err_msg=f"lanes frame {i + 1} {k}")


def _frame_maps(pred, data, i, B, P):
    import torch
    npcs = pred["npcs_pred"][i]
    labels = torch.argmax(npcs["seg"], dim=-2).int().contiguous()
    src = npcs["nocs"].reshape(B, P, 3, -1).float().contiguous()
    return labels, src, data[i]["points"].float().to(src.device).contiguous(), data[i]["meta"]["points_mean"].float().to(src.device)


@pytest.mark.gpu
def test_st_fit_and_guard_consume_the_consensus_rotation(device):
    """Consensus read-out, robust scale / translation fit and guard (monitoring) all on: the rotation is the consensus call's, the
    three records are there, and the guard's is part_fit_guard_cn's on each frame's maps and the final pose."""
    from captra_amd.pose_utils.pose_fit import part_fit_guard_cn
    guard = {"refit": False, "lost_below": 0.5, "yaxis_only": True}
    with _Spy() as spy:
        model, cfg, data, both = _run(device, "bottle", {"consensus": True, "angle_th": TH_LOOP}, st_fit={"ransac": True}, guard=guard)
    assert set(both) == {"poses", "npcs_pred", "guard", "st_fit", "rot_pool"}
    B, P = both["poses"][0]["scale"].shape
    g = model.guard
    for i in range(1, len(data)):
        _same_bits(both["poses"][i]["rotation"].cpu().numpy(), spy.calls[i - 1]["rot"].cpu().numpy(), f"frame {i} rotation")
        labels, src, pts, mean = _frame_maps(both, data, i, B, P)
        _, info = part_fit_guard_cn(labels, src, pts, mean, both["poses"][i], inlier_th=g["inlier_th"], lost_below=g["lost_below"],
                                    min_members=g["min_members"], refit=False, num_hyps=g["num_hyps"], seed=g["seed"], yaxis_only=True)
        for k in ("count", "inliers", "rms", "verdict"):
            np.testing.assert_array_equal(both["guard"][i][k].cpu().numpy(), info[k].cpu().numpy(), err_msg=f"frame {i} {k}")
        np.testing.assert_array_equal(both["rot_pool"][i]["count"].cpu().numpy(), info["count"].cpu().numpy())


@pytest.mark.gpu
def test_layer_by_layer_path_takes_the_consensus(device):
    """PartCanonNet.forward without the fused rotation read-out (fused.USE_ROT_READOUT off): the record, and the rotation the wrapper
    gives on raw_diag's output (the spy's `raw` is what the path handed over: (B*P,R,N), the diagonal heads only)."""
    import torch
    from captra_amd import fused
    trainer, cfg, data = _model(device, "drawers", {"consensus": True, "angle_th": TH_LOOP})
    model = trainer.model
    model.set_data(data)
    last = {k: v.clone() for k, v in model.feed_dict[0]["gt_part"].items()}
    old = fused.USE_ROT_READOUT
    fused.USE_ROT_READOUT = False
    try:
        with torch.no_grad(), _Spy() as spy:
            npcs, pose = model.track_step(model.feed_dict[1], model.npcs_feed_dict[1], last)
    finally:
        fused.USE_ROT_READOUT = old
    assert len(spy.calls) == 1
    call = spy.calls[0]
    B, P = pose["scale"].shape
    assert call["raw"].dim() == 3 and call["raw"].shape[:2] == (B * P, 6)
    labels = torch.argmax(npcs["seg"], dim=-2).int().contiguous()
    assert torch.equal(labels, call["labels"])
    rot, info = fused.rot_pool_consensus(call["raw"], labels, last["rotation"].float().contiguous(), False, TH_LOOP, num_hyps=64, seed=0, b0=0)
    _same_bits(pose["rotation"].cpu().numpy(), rot.cpu().numpy(), "rotation")
    np.testing.assert_array_equal(npcs["rot_inliers"].cpu().numpy(), info["inliers"].cpu().numpy())
    np.testing.assert_array_equal(npcs["rot_count"].cpu().numpy(), info["count"].cpu().numpy())


# ========================================================================================================== 8. off changes nothing
@pytest.mark.gpu
def test_off_changes_nothing(device, tmp_path):
    """No key and consensus: False: the same poses bit for bit, the parent's pred_dict and pickle keys, the same random-number
    consumption and no launch of the new kernel among the profiler's kernel names (the plain read-out's is there); on: the pickles
    gain 'rot_pool' and nothing else, and the plain read-out is no longer launched."""
    import torch
    from captra_amd import _lib
    runs, keys = {}, {}
    for name, rp in (("absent", None), ("false", {"consensus": False, "num_hyps": 16}), ("on", {"consensus": True, "angle_th": TH_LOOP})):
        trainer, cfg, data = _model(device, "bottle", rp, experiment_dir=tmp_path / name)
        assert (trainer.model.rot_pool is not None) == (name == "on")
        torch.manual_seed(4321)
        _lib.prof_enable(True)
        _lib.prof_reset()
        try:
            pred, _ = trainer.test(data, save=True, no_eval=True)
            torch.cuda.synchronize()
            names = set(_lib.prof_names())
            launches = {k: _lib.prof_read(k)[1] for k in ("rot_pool_compose", "rot_pool_consensus_sym")}
        finally:
            _lib.prof_enable(False)
        # (the off runs come first: the profiler keeps the names it has met while it was enabled)
        assert any("rot_pool_consensus" in n for n in names) == (name == "on"), names
        # launches since the reset: the plain read-out once per step when off, never when on
        assert launches == ({"rot_pool_compose": 0, "rot_pool_consensus_sym": 3} if name == "on" else {"rot_pool_compose": 3, "rot_pool_consensus_sym": 0}), launches
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
    assert torch.equal(runs["absent"][1], runs["on"][1])
    assert set(runs["on"][0]) == {"poses", "npcs_pred", "rot_pool"} and set(keys["on"]) == {"pred", "gt", "frame_nums", "rot_pool"}
    rec = keys["on"]["rot_pool"]
    assert rec[0] is None and len(rec) == 4
    for r in rec[1:]:
        assert set(r) == {"inliers", "count"} and all(np.asarray(v).shape == (1,) for v in r.values())
