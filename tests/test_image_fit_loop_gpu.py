"""The on-the-fly re-crop loop started from images alone (init_frame: {gt: False, image_fit: True}, captra_amd/model.py;
include/captra_hip.h: captra_image_members) on make_otf_trajectory(2, 3, coord=True): the first pose is the hand-made chain's bit for
bit and the judge chain's (tests/image_fit_judge.py -> tests/ransac_judge.py) within the RANSAC kernel's bounds, the loop runs on to
finite poses, the record reaches pred_dict, the pickle and the eval table, the eager and the captured loop agree, a configured depth
filter is in front of the fit, and without the option nothing is launched or recorded."""
import pickle

import numpy as np
import pytest
import torch

from tests import depth_judge as DJ
from tests import image_fit_judge as IJ
from tests import ransac_judge as RJ
from tests.test_pose_readout_gpu import F32_EPS, MATRIX_ATOL
from tests.weights import make_physical_state_dict

pytestmark = pytest.mark.gpu

FRAMES, BATCH = 3, 2
TRAJ_SEED, WEIGHT_SEED, RUN_SEED = 1, 31, 5001
FILTER = {"window": 3, "abs_mm": 10, "min_support": 12}
FILTER_RULE = dict(window=3, abs_mm=10, rel_permille=0, min_support=12)
REC_KEYS = ("members", "used", "holes", "inliers", "valid")


def _trainer(device, init_frame, depth_filter=None):
    from captra_amd.configs import make_config
    from captra_amd.trainer import Trainer
    cfg = make_config("1", experiment_dir="/tmp/captra_image_fit_test", nocs_otf=True)
    cfg["device"] = device
    cfg["init_frame"].update(init_frame)
    if depth_filter is not None:
        cfg["track_cfg"]["depth_filter"] = dict(depth_filter)
    trainer = Trainer(cfg)
    model = trainer.model
    model.load_state_dict(make_physical_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, WEIGHT_SEED, 1, True, "nocs"))
    return trainer


@pytest.fixture(scope="module")
def trainers(device):
    return {"on": _trainer(device, {"gt": False, "image_fit": True}), "off": _trainer(device, {"gt": False})}


@pytest.fixture(scope="module")
def data():
    from captra_amd.synthetic import make_otf_trajectory
    return make_otf_trajectory(BATCH, FRAMES, seed=TRAJ_SEED, coord=True)


def _run(trainer, data, hipgraph, save=False):
    model = trainer.model
    model.use_graph = hipgraph
    torch.manual_seed(RUN_SEED); np.random.seed(RUN_SEED)
    pred, _ = trainer.test(data, save=save, no_eval=True)
    poses = [{k: pred["poses"][i][k].clone() for k in ("rotation", "translation", "scale")} for i in range(len(data))]
    return poses, dict(model.pred_dict)


@pytest.fixture(scope="module")
def eager_on(trainers, data):
    return _run(trainers["on"], data, hipgraph=False)


def _by_hand(model):
    """image_members + part_fit_ransac_cn on the model's own device images of frame 0, at the model's settings."""
    from captra_amd.nocs_otf import image_members
    from captra_amd.pose_utils.pose_fit import part_fit_ransac_cn
    pre = model.feed_dict[0]["pre_fetched"]
    mem = image_members(pre["depth"].contiguous(), pre["mask"].contiguous(), pre["coord"], **{k: model.image_fit[k] for k in ("cap", "border", "negate_z")})
    fit = part_fit_ransac_cn(mem["labels"], mem["src"], mem["tgt"], num_hyps=model.fit_init_cfg["num_hyps"], inlier_th=model.fit_init_cfg["inlier_th"],
                             seed=model.fit_init_cfg["seed"])
    return mem, fit


def test_first_pose_is_the_chain_by_hand_and_the_judges(trainers, data, eager_on):
    from captra_amd.track_options import INIT_FIT_INLIER_TH
    model = trainers["on"].model
    poses, pred = eager_on
    mem, (rot, scale, trans, valid, info) = _by_hand(model)
    assert bool(valid.all())
    assert torch.equal(poses[0]["rotation"], rot) and torch.equal(poses[0]["scale"], scale) and torch.equal(poses[0]["translation"], trans)
    # the members are the judge's
    pre = data[0]["meta"]["pre_fetched"]
    ref_mem = IJ.members(pre["depth"].numpy(), pre["mask"].numpy(), pre["coord"].numpy(), IJ.kinv_of(IJ.NOCS_INTRINSICS["real"]), 16384)
    got = {k: v.cpu().numpy() for k, v in mem.items()}
    for k in ("counts", "pix", "labels", "src"):
        np.testing.assert_array_equal(got[k], ref_mem[k], err_msg=k)
    assert IJ.tgt_agrees(got["tgt"], ref_mem["tgt64"])
    # the fit of the kernel's members, judged in float64 and mirrored in float32 (tests/test_pose_ransac_gpu.py's criteria); what
    # makes the inlier set decidable here: every member is an inlier, in some hypothesis with all residuals below 0.9 th
    th = float(np.float32(INIT_FIT_INLIER_TH * float(model.cfg["data_radius"])))
    ref, ranks = IJ.fit_chain(got, th)
    mir, _ = IJ.fit_chain(got, th, dt=np.float32)
    for b in range(BATCH):
        used = int(got["counts"][b, 1])
        S, T = got["src"][b, 0][:, :used].T, got["tgt"][b][:, :used].T
        RJ.check_precondition(S, T, ranks[b, 0] % used, th, np.ones(used, bool))
        assert ref["valid"][b, 0] and mir["valid"][b, 0] and int(info["num_inliers"][b, 0]) == ref["num_inliers"][b, 0] == used
        R = poses[0]["rotation"][b, 0].double().cpu().numpy()
        s, t = float(poses[0]["scale"][b, 0]), poses[0]["translation"][b, 0, :, 0].double().cpu().numpy()
        es, ms = abs(s - ref["scale"][b, 0]), abs(mir["scale"][b, 0] - ref["scale"][b, 0])
        et, mt = np.abs(t - ref["trans"][b, 0]).max(), np.abs(mir["trans"][b, 0] - ref["trans"][b, 0]).max()
        er, mr = np.abs(R - ref["rot"][b, 0]).max(), np.abs(mir["rot"][b, 0] - ref["rot"][b, 0]).max()
        print(f"trajectory {b}: scale err kernel {es:.2e} mirror {ms:.2e}; trans {et:.2e} / {mt:.2e}; rot {er:.2e} / {mr:.2e}")
        assert es <= max(2 * ms, 4 * F32_EPS * abs(ref["scale"][b, 0]))
        assert et <= max(2 * mt, 4 * F32_EPS * np.abs(ref["trans"][b, 0]).max())
        assert er <= max(2 * mr, MATRIX_ATOL)
    # and it needs no annotation: the fallback it was given is a perturbed pose, the fit is the scene's pose
    gt = data[0]["meta"]["nocs2camera"][0]
    for b in range(BATCH):
        err = IJ.pose_errors(poses[0]["rotation"][b, 0].cpu().numpy(), float(poses[0]["scale"][b, 0]), poses[0]["translation"][b, 0].cpu().numpy(),
                             gt["rotation"][b].numpy(), float(gt["scale"][b]), gt["translation"][b].numpy())
        assert err[0] <= 0.1 and err[1] <= 0.1 and err[2] <= 1e-3, err


def test_the_loop_runs_on_and_records_the_fit(trainers, data, eager_on):
    poses, pred = eager_on
    assert len(poses) == FRAMES
    for p in poses:
        assert all(torch.isfinite(v).all() for v in p.values())
    rec = pred["image_fit"]
    assert tuple(rec) == REC_KEYS
    for k in REC_KEYS:
        assert rec[k].is_cuda and rec[k].dtype == torch.int32 and tuple(rec[k].shape) == (BATCH,), k
    pre = data[0]["meta"]["pre_fetched"]
    ref = IJ.members(pre["depth"].numpy(), pre["mask"].numpy(), pre["coord"].numpy(), IJ.kinv_of(IJ.NOCS_INTRINSICS["real"]), 16384)
    assert rec["members"].tolist() == ref["counts"][:, 0].tolist() and rec["used"].tolist() == ref["counts"][:, 1].tolist()
    assert rec["holes"].tolist() == ref["counts"][:, 2].tolist() and rec["valid"].tolist() == [1] * BATCH
    assert rec["inliers"].tolist() == rec["used"].tolist()


def test_record_reaches_the_pickle_and_the_eval_table(trainers, data, eager_on, tmp_path, capsys):
    from captra_amd import eval as ev
    model = trainers["on"].model
    model.cfg["experiment_dir"] = str(tmp_path)
    _run(trainers["on"], data, hipgraph=False, save=True)
    names = sorted(p.name for p in (tmp_path / "results" / "data").iterdir())
    assert names == [f"inst{TRAJ_SEED + b}_track0.pkl" for b in range(BATCH)]
    lines = []
    for b, name in enumerate(names):
        with open(tmp_path / "results" / "data" / name, "rb") as f:
            rec = pickle.load(f)
        assert {k: int(np.asarray(v)) for k, v in rec["image_fit"].items()} == {k: int(eager_on[1]["image_fit"][k][b]) for k in REC_KEYS}
        lines += ev.image_fit_table(name.rsplit(".", 1)[0], rec)
    capsys.readouterr()
    ev.main(["--obj_category", "1", "--experiment_dir", str(tmp_path), "--eval_device"])
    printed = capsys.readouterr().out
    assert "init_frame/image_fit" in printed and all(line in printed for line in lines)


def test_eager_and_captured_loop_agree(trainers, data, eager_on):
    graph = _run(trainers["on"], data, hipgraph=True)
    for k in ("rotation", "translation", "scale"):
        assert torch.equal(eager_on[0][0][k], graph[0][0][k]), k
    for a, b in zip(eager_on[0], graph[0]):
        assert all(torch.equal(a[k], b[k]) for k in a)
    assert all(torch.equal(eager_on[1]["image_fit"][k], graph[1]["image_fit"][k]) for k in REC_KEYS)


def test_option_absent_launches_and_records_nothing(trainers, data, eager_on, monkeypatch):
    from captra_amd import _lib
    calls, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *args: (calls.append(name), real(name, *args))[1])
    _lib.prof_reset(); _lib.prof_enable(True)
    try:
        off = _run(trainers["off"], data, hipgraph=False)
    finally:
        _lib.prof_enable(False)
    monkeypatch.setattr(_lib, "call", real)
    assert calls and "captra_image_members" not in calls and _lib.prof_read("image_members")[1] == 0
    assert trainers["off"].model.image_fit is None and "image_fit" not in off[1]
    assert "coord" not in trainers["off"].model.feed_dict[0]["pre_fetched"]             # nothing is uploaded for it either
    assert any(not torch.equal(off[0][0][k], eager_on[0][0][k]) for k in off[0][0])      # (the perturbed annotation is another pose)
    _lib.prof_reset(); _lib.prof_enable(True)
    try:
        _run(trainers["on"], data, hipgraph=False)
    finally:
        _lib.prof_enable(False)
    assert _lib.prof_read("image_members")[1] == 1                                      # (the counter does see the launch)


def test_a_configured_depth_filter_is_in_front_of_the_fit(device):
    """The scene with flying pixels along the silhouette: the record and the first pose are those of the FILTERED image."""
    from captra_amd.synthetic import make_otf_trajectory
    data = make_otf_trajectory(BATCH, 2, seed=TRAJ_SEED, flying=0.5, coord=True)
    trainer = _trainer(device, {"gt": False, "image_fit": True, "border": 1}, depth_filter=FILTER)
    poses, pred = _run(trainer, data, hipgraph=False)
    pre = data[0]["meta"]["pre_fetched"]
    kinv = IJ.kinv_of(IJ.NOCS_INTRINSICS["real"])
    filtered, removed = DJ.judge(pre["depth"].numpy(), **FILTER_RULE)
    want = IJ.members(filtered, pre["mask"].numpy(), pre["coord"].numpy(), kinv, 16384, 1)
    raw = IJ.members(pre["depth"].numpy(), pre["mask"].numpy(), pre["coord"].numpy(), kinv, 16384, 1)
    rec = pred["image_fit"]
    assert rec["members"].tolist() == want["counts"][:, 0].tolist() and rec["holes"].tolist() == want["counts"][:, 2].tolist()
    assert (want["counts"][:, 0] < raw["counts"][:, 0]).all() and (want["counts"][:, 2] > raw["counts"][:, 2]).all()
    mem, (rot, scale, trans, valid, _) = _by_hand(trainer.model)
    assert np.array_equal(mem["pix"].cpu().numpy(), want["pix"])
    assert torch.equal(poses[0]["rotation"], rot) and torch.equal(poses[0]["scale"], scale) and torch.equal(poses[0]["translation"], trans)
