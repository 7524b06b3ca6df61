"""captra_part_fit_ransac (csrc/pose_ransac.hip) through the C ABI against the float64 judge of tests/ransac_judge.py, and the
first-pose fit of EvalTrackModel (init_frame: {fit: True}) on the synthetic trajectories.

A RANSAC result is a function of an inlier SET; the cases come with the precondition that makes that set immune to a 10 %
rounding of any residual (ransac_judge.check_precondition), so the kernel must select exactly the judge's set and its pose is
then compared like the one-pass fit's: at most twice as far from float64 as the float32 mirror, with the floors of
tests/test_pose_readout_gpu.py (4 fp32 ulps of the output for scale and translation, MATRIX_ATOL for the rotation)."""
from pathlib import Path

import numpy as np
import pytest

from tests import ransac_judge as J
from tests.test_pose_readout_gpu import DET_ATOL, F32_EPS, MATRIX_ATOL, ORTHO_ATOL

GOLDEN = Path(__file__).resolve().parent / "golden" / "g17_pose_fit_ransac.npz"
_CASES = {}


def _case(*key, **kw):
    """Cases and their judge / mirror results, built once and shared (never modified)."""
    k = key + tuple(sorted(kw.items()))
    if k not in _CASES:
        c = J.batch_case(*key, **kw)
        args = (c["labels"], c["src"], c["tgt"], float(c["th"]), c["ranks"], c["tgt_mean"])
        _CASES[k] = (c, J.judge_batch(*args), J.judge_batch(*args, dt=np.float32))
    return _CASES[k]


def _dev(a, device):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _abi(case, device, ranks="given", seed=0, num_hyps=None, shape=None):
    """The C ABI on sentinel-filled outputs -> (err, dict of numpy outputs).  ranks: 'given' = the case's, None = NULL (drawn in the
    kernel from `seed`), or an array.  shape = (b, p, n, h) overrides what the arrays say (for the refused shapes)."""
    import torch
    from captra_amd import _lib as L
    B, P, _, N = case["src"].shape
    H = case["ranks"].shape[2] if num_hyps is None else num_hyps
    r = case["ranks"] if isinstance(ranks, str) else ranks
    d = {k: _dev(case[k], device) for k in ("labels", "src", "tgt", "tgt_mean")}
    rk = None if r is None else _dev(np.asarray(r, np.int32), device)
    out = dict(rot=torch.full((B, P, 3, 3), float("nan"), device=device), scale=torch.full((B, P), float("nan"), device=device),
               trans=torch.full((B, P, 3), float("nan"), device=device), valid=torch.full((B, P), -7, dtype=torch.int32, device=device),
               best=torch.full((B, P), -7, dtype=torch.int32, device=device), num_inliers=torch.full((B, P), -7, dtype=torch.int32, device=device),
               samples=torch.full((B, P, H, 3), -7, dtype=torch.int32, device=device))
    b_, p_, n_, h_ = shape if shape is not None else (B, P, N, H)
    with torch.cuda.device(device):
        err = L.lib().captra_part_fit_ransac(b_, p_, n_, h_, float(case["th"]), L.ptr(d["labels"]), L.ptr(d["src"]), L.ptr(d["tgt"]),
                                             1 if case["per_part"] else 0, L.ptr(d["tgt_mean"]), L.ptr(rk), seed, L.ptr(out["rot"]),
                                             L.ptr(out["scale"]), L.ptr(out["trans"]), L.ptr(out["valid"]), L.ptr(out["best"]),
                                             L.ptr(out["num_inliers"]), L.ptr(out["samples"]), L.stream_ptr())
    torch.cuda.synchronize(device)
    return err, {k: v.cpu().numpy() for k, v in out.items()}


def _check(got, case, ranks, ref, mir, name):
    """Everything the issue asserts for one launch whose member ranks were `ranks`."""
    B, P = ref["valid"].shape
    np.testing.assert_array_equal(got["num_inliers"], ref["num_inliers"], err_msg=name)
    np.testing.assert_array_equal(got["valid"].astype(bool), ref["valid"], err_msg=name)
    for k in ("rot", "scale", "trans"):
        assert np.isfinite(got[k]).all(), (name, k)
    for b in range(B):
        for p in range(P):
            pts, S, T = J.members_of(case, b, p)
            tag = (name, b, p, len(pts))
            if len(pts) < 3:
                assert not ref["valid"][b, p] and (got["samples"][b, p] == -1).all() and got["best"][b, p] == 0, tag
            else:
                np.testing.assert_array_equal(got["samples"][b, p], pts[np.asarray(ranks[b, p]) % len(pts)], err_msg=str(tag))
                # the inlier set of the kernel's `best` (any hypothesis at the top score), recomputed in float64 from its samples
                h = int(got["best"][b, p])
                assert 0 <= h < got["samples"].shape[2], tag
                tgt = case["tgt"][b, p] if case["per_part"] else case["tgt"][b]
                if case["tgt_mean"] is not None:
                    tgt = (tgt + case["tgt_mean"][b][:, None]).astype(np.float32)
                mask = J.inlier_set(case["labels"][b] == p, case["src"][b, p], tgt, float(case["th"]), got["samples"][b, p, h])
                np.testing.assert_array_equal(mask, ref["inliers"][b, p], err_msg=str(tag))
            if not ref["valid"][b, p]:
                np.testing.assert_array_equal(got["rot"][b, p], np.eye(3, dtype=np.float32), err_msg=str(tag))
                assert got["scale"][b, p] == 1.0 and (got["trans"][b, p] == 0.0).all(), tag
                continue
            assert mir["valid"][b, p], tag
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
@pytest.mark.parametrize("with_mean", [False, True])
@pytest.mark.parametrize("per_part", [False, True])
@pytest.mark.parametrize("N", [257, 4096])
def test_ransac_vs_judge(device, N, per_part, with_mean):
    """B = 3, P = 3, H = 64 with the judge's triples: exact inlier counts and sets, validity, pose bounds; parts of 0 and 2
    members and the part of gross outliers are invalid with identity / 1 / 0, the part of exactly 3 members is valid."""
    case, ref, mir = _case(N, 1000 + N + 2 * per_part + with_mean, per_part, with_mean)
    err, got = _abi(case, device)
    assert err == 0
    _check(got, case, case["ranks"], ref, mir, f"N={N}")
    counts = [[int((case["labels"][b] == p).sum()) for p in range(3)] for b in range(3)]
    assert counts[1] == [2, 3, 4] and counts[2] == [N, 0, 0]
    v = got["valid"].astype(bool)
    assert not v[1, 0] and v[1, 1] and v[1, 2] and v[2, 0] and not v[2, 1] and not v[2, 2]
    assert not v[0, 2] and got["num_inliers"][0, 2] < 3 and counts[0][2] >= 3          # gross outliers only


@pytest.mark.gpu
def test_ransac_largest_shape(device):
    """P = 1, N = 16384, H = 256: the member list alone sits in LDS, the coordinates are re-read from global memory."""
    case, ref, mir = _case(16384, 16384, False, True, num_hyps=256, B=1, P=1)
    err, got = _abi(case, device)
    assert err == 0
    _check(got, case, case["ranks"], ref, mir, "N=16384")
    assert got["valid"][0, 0] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("N", [257, 4096])
def test_ransac_kernel_draws(device, N):
    """sample_rank = NULL: the samples are the numpy generator's for two seeds, every triple is three distinct members, the same
    seed gives the same bits, and the pose is within the same bounds of the judge run on those triples."""
    case, _, _ = _case(N, 1000 + N + 1, False, True)
    B, P, H = case["ranks"].shape[:3]
    first = None
    for seed in (11, 12):
        ranks = np.zeros_like(case["ranks"])
        for b in range(B):
            for p in range(P):
                c = int((case["labels"][b] == p).sum())
                if c >= 3:
                    ranks[b, p] = J.draw_ranks(seed, b, p, H, c)
        J.check_batch(case, ranks)
        err, got = _abi(case, device, ranks=None, seed=seed)
        assert err == 0
        args = (case["labels"], case["src"], case["tgt"], float(case["th"]), ranks, case["tgt_mean"])
        _check(got, case, ranks, J.judge_batch(*args), J.judge_batch(*args, dt=np.float32), f"N={N} seed={seed}")
        for b in range(B):
            for p in range(P):
                if (case["labels"][b] == p).sum() >= 3:
                    s = got["samples"][b, p]
                    assert (case["labels"][b][s] == p).all()
                    assert (s[:, 0] != s[:, 1]).all() and (s[:, 0] != s[:, 2]).all() and (s[:, 1] != s[:, 2]).all()
        err, again = _abi(case, device, ranks=None, seed=seed)
        assert err == 0
        for k in got:
            np.testing.assert_array_equal(got[k], again[k])
        if first is not None:
            assert (got["samples"] != first["samples"]).any()
        first = got


@pytest.mark.gpu
def test_ransac_g17_through_the_kernel(device):
    """The reference's own fit (golden G17) within the project's 1e-4, its None case invalid."""
    z = np.load(GOLDEN)
    for i in range(int(z["num_cases"])):
        S, T = z[f"src{i}"], z[f"tgt{i}"]
        K = len(S)
        case = dict(labels=np.zeros((1, K), np.int32), src=np.ascontiguousarray(S.T[None, None]), tgt=np.ascontiguousarray(T.T[None]),
                    tgt_mean=None, th=np.float32(z[f"th{i}"]), ranks=z[f"triples{i}"][None, None].astype(np.int32), per_part=False)
        err, got = _abi(case, device)
        assert err == 0
        if int(z[f"none{i}"]):
            assert got["valid"][0, 0] == 0 and got["num_inliers"][0, 0] < 3
            continue
        assert got["valid"][0, 0] == 1
        np.testing.assert_allclose(got["rot"][0, 0], z[f"rot{i}"], atol=1e-4, rtol=0)
        np.testing.assert_allclose(got["scale"][0, 0], z[f"scale{i}"], atol=1e-4, rtol=0)
        np.testing.assert_allclose(got["trans"][0, 0], z[f"trans{i}"], atol=1e-4, rtol=0)


@pytest.mark.gpu
def test_ransac_refused_shapes(device):
    """P = 9, H = 0, H = 257, N = 16385 (and N = 0): -1 and nothing is written."""
    case, _, _ = _case(257, 1257, False, False)
    for shape in ((3, 9, 257, 64), (3, 3, 257, 0), (3, 3, 257, 257), (3, 3, 16385, 64), (3, 3, 0, 64)):
        err, got = _abi(case, device, shape=shape)
        assert err == -1, shape
        assert np.isnan(got["rot"]).all() and (got["valid"] == -7).all() and (got["samples"] == -7).all()


@pytest.mark.gpu
def test_part_fit_ransac_wrappers(device):
    """The reference-layout wrapper and the channel-major one give the ABI's bits."""
    import torch
    from captra_amd.pose_utils.pose_fit import part_fit_ransac, part_fit_ransac_cn
    case, _, _ = _case(257, 1257 + 3, True, True)
    err, got = _abi(case, device)
    assert err == 0
    rk = _dev(case["ranks"], device)
    rot, scale, trans, valid, info = part_fit_ransac_cn(_dev(case["labels"], device), _dev(case["src"], device), _dev(case["tgt"], device),
                                                        inlier_th=float(case["th"]), sample_rank=rk, target_mean=_dev(case["tgt_mean"], device),
                                                        tgt_per_part=True, want_samples=True)
    model, valid2, info2 = part_fit_ransac(_dev(case["labels"].astype(np.int64), device), _dev(case["src"].transpose(0, 1, 3, 2), device),
                                           _dev(case["tgt"].transpose(0, 1, 3, 2), device), {"num_parts": 3}, inlier_th=float(case["th"]),
                                           sample_rank=rk, target_mean=_dev(case["tgt_mean"], device))
    assert trans.shape == (3, 3, 3, 1) and valid.dtype == torch.bool
    for a, b, c in ((rot, model["rotation"], got["rot"]), (scale, model["scale"], got["scale"]), (trans[..., 0], model["translation"][..., 0], got["trans"]),
                    (valid, valid2, got["valid"].astype(bool)), (info["best"], info2["best"], got["best"]),
                    (info["num_inliers"], info2["num_inliers"], got["num_inliers"])):
        np.testing.assert_array_equal(a.cpu().numpy(), c)
        np.testing.assert_array_equal(b.cpu().numpy(), c)
    np.testing.assert_array_equal(info["samples"].cpu().numpy(), got["samples"])


def _model(tag, device, init_frame=None, frames=3):
    from captra_amd import synthetic as clouds
    from captra_amd.configs import make_config
    from captra_amd.trainer import Trainer
    cat, objcfg, kind, _, batch, wseed, _ = clouds.PHYSICAL_SETUPS[tag]
    cfg = make_config(cat, objcfg, experiment_dir="/tmp/captra_test_exp")
    if init_frame is not None:
        cfg["init_frame"] = dict(init_frame)
    trainer = Trainer(cfg)
    shapes = {k: tuple(v.shape) for k, v in trainer.model.state_dict().items()}
    trainer.model.load_state_dict(clouds.make_physical_state_dict(shapes, wseed, cfg["num_parts"], bool(cfg["obj_sym"]), kind))
    return trainer, cfg, clouds.make_trajectory(kind, batch, frames, seed=7)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["bottle", "drawers"])
def test_initial_pose_fitted_from_frame0(device, tag):
    """init_frame: {gt: False, fit: True} at B = 2: the synthetic NOCS map is exact, every member is an inlier and the fit is
    the full-cloud Umeyama -- the float64 judge is within 1e-4 of frame 0's nocs2camera, and the model's first pose is within
    the kernel's bounds of the judge (hence needs no annotation: the fallback it was given is a perturbed pose)."""
    from captra_amd.track_options import INIT_FIT_INLIER_TH
    trainer, cfg, data = _model(tag, device, {"gt": False, "fit": True}, frames=1)
    model = trainer.model
    model.set_data(data)
    pose = {k: v.cpu().numpy() for k, v in model._initial_pose().items()}
    B, P = pose["scale"].shape
    N = data[0]["points"].shape[-1]
    labels = data[0]["labels"].numpy().astype(np.int32)
    src = np.ascontiguousarray(np.broadcast_to(data[0]["nocs"].numpy()[:, None], (B, P, 3, N)), np.float32)
    th = np.float32(INIT_FIT_INLIER_TH * cfg["data_radius"])
    ranks = np.zeros((B, P, 64, 3), np.int64)
    for b in range(B):
        for p in range(P):
            ranks[b, p] = J.draw_ranks(0, b, p, 64, int((labels[b] == p).sum()))
    args = (labels, src, data[0]["points"].numpy(), float(th), ranks, data[0]["meta"]["points_mean"].numpy().reshape(B, 3))
    ref, mir = J.judge_batch(*args), J.judge_batch(*args, dt=np.float32)
    assert ref["valid"].all()
    for p in range(P):
        gt = data[0]["meta"]["nocs2camera"][p]
        assert (ref["num_inliers"][:, p] == (labels == p).sum(1)).all()
        assert np.abs(ref["rot"][:, p] - gt["rotation"].numpy()).max() <= 1e-4
        assert np.abs(ref["scale"][:, p] - gt["scale"].numpy()).max() <= 1e-4
        assert np.abs(ref["trans"][:, p] - gt["translation"].numpy()[..., 0]).max() <= 1e-4
    for b in range(B):
        for p in range(P):
            es, ms = abs(pose["scale"][b, p] - ref["scale"][b, p]), abs(mir["scale"][b, p] - ref["scale"][b, p])
            et = np.abs(pose["translation"][b, p, :, 0] - ref["trans"][b, p]).max()
            mt = np.abs(mir["trans"][b, p] - ref["trans"][b, p]).max()
            er, mr = np.abs(pose["rotation"][b, p] - ref["rot"][b, p]).max(), np.abs(mir["rot"][b, p] - ref["rot"][b, p]).max()
            print(f"{tag} ({b},{p}): scale {es:.2e} / {ms:.2e}; trans {et:.2e} / {mt:.2e}; rot {er:.2e} / {mr:.2e}")
            assert es <= max(2 * ms, 4 * F32_EPS * abs(ref["scale"][b, p]))
            assert et <= max(2 * mt, 4 * F32_EPS * np.abs(ref["trans"][b, p]).max())
            assert er <= max(2 * mr, MATRIX_ATOL)


@pytest.mark.gpu
def test_fit_off_changes_nothing(device):
    """fit absent and fit: False: forward() returns the same bits, pose by pose, from the same seed."""
    import torch
    runs = []
    for init in (None, {"gt": False, "fit": False}):
        trainer, cfg, data = _model("bottle", device, init)
        assert not trainer.model.fit_init
        torch.manual_seed(4321)
        pred, _ = trainer.test(data, save=False, no_eval=True)
        runs.append((pred["poses"], torch.rand(3)))
    for a, b in zip(runs[0][0], runs[1][0]):
        for k in a:
            np.testing.assert_array_equal(a[k].cpu().numpy(), b[k].cpu().numpy())
    assert torch.equal(runs[0][1], runs[1][1])                    # the same random-number consumption
