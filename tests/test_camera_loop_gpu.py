"""The camera model through the on-the-fly re-crop loop (captra_amd/model.py: `camera`, meta['pre_fetched']['camera']):

  * a MIXED batch -- one trajectory's sensor counts half millimetres (its images hold twice the numbers, its depth_unit is 0.0005) --
    tracks to the plain run's poses BYTE FOR BYTE on every frame (doubling a count and halving the unit are power-of-two scalings: exact
    in float64), in every batch form: eager, one captured graph, two lanes with the deferred check; with `nocs2d_label` detections and
    with `init_frame/image_fit`.  Without the feature the camera is ignored and that trajectory's object sits at twice its distance;
  * a shifted principal point: images padded on the left and at the bottom, seen through the camera with cx + q, cy + p, give the same
    crop -- the same pixels in the same order, the points within 1e-12 m;
  * option absent: no camera tensor, no pickle entry, the plain entry points."""
import numpy as np
import pytest
import torch

from tests import camera_judge as C, otf_inputs as I

pytestmark = pytest.mark.gpu

FRAMES, BATCH = 4, 3
TRAJ_SEED, WEIGHT_SEED, RUN_SEED = 1, 31, 5001
CAMERAS = [(None, 0.001, 1), (None, 0.0005, 2), (None, 0.001, 1)]          # trajectory 1 alone counts half millimetres


@pytest.fixture(scope="module", autouse=True)
def _leave_the_allocator_as_found():
    """Set up first, so torn down last: when this module's tensors and models are gone its cached blocks go back to the driver.  Tests
    that run later in the same process (fused.pointwise_mlp2 wants its two sources within 1 GiB of each other) find the caching
    allocator as a run without this module leaves it."""
    yield
    import gc
    gc.collect()
    torch.cuda.empty_cache()


def _trainer(device, nocs2d_label=False, image_fit=False):
    from captra_amd.configs import make_config
    from captra_amd.synthetic import make_physical_state_dict
    from captra_amd.trainer import Trainer
    cfg = make_config("1", experiment_dir="/tmp/captra_camera_test", nocs_otf=True)
    cfg["device"] = device
    cfg["init_frame"].update({"gt": False, "image_fit": True} if image_fit else {"gt": True})
    cfg["track_cfg"]["nocs2d_label"] = bool(nocs2d_label)
    trainer = Trainer(cfg)
    model = trainer.model
    model.load_state_dict(make_physical_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, WEIGHT_SEED, 1, True, "nocs"))
    return trainer


def _data(cameras, det=False, coord=False, batch=BATCH, frames=FRAMES):
    from captra_amd.synthetic import make_otf_detections, make_otf_trajectory
    data = make_otf_trajectory(batch, frames, seed=TRAJ_SEED, coord=coord, cameras=cameras)
    return make_otf_detections(batch, frames, seed=TRAJ_SEED, data=data) if det else data


def _run(trainer, data, hipgraph=False, lanes=False, save=False):
    model = trainer.model
    model.use_graph, model.otf_lanes = hipgraph, lanes
    torch.manual_seed(RUN_SEED); np.random.seed(RUN_SEED)
    pred, _ = trainer.test(data, save=save, no_eval=True)
    return [{k: pred["poses"][i][k].clone() for k in ("rotation", "translation", "scale")} for i in range(len(data))], dict(model.pred_dict)


def _assert_same_poses(a, b, tag):
    assert len(a) == len(b)
    for i, (pa, pb) in enumerate(zip(a, b)):
        for k in pa:
            assert torch.equal(pa[k], pb[k]), (tag, k, i)
        assert all(torch.isfinite(v).all() for v in pa.values()), (tag, i)


@pytest.fixture(scope="module")
def det_trainer(device):
    return _trainer(device, nocs2d_label=True)


@pytest.fixture(scope="module")
def fit_trainer(device):
    return _trainer(device, image_fit=True)


@pytest.mark.parametrize("hipgraph", [False, True], ids=["eager", "hipgraph"])
def test_mixed_batch_with_detections_tracks_to_the_plain_poses(det_trainer, hipgraph):
    """3 trajectories x 4 frames, the detector route: every pose of every frame == the plain run's."""
    plain, pred_p = _run(det_trainer, _data(None, det=True), hipgraph)
    assert det_trainer.model.camera is None and "camera" not in pred_p
    mixed, pred_m = _run(det_trainer, _data(CAMERAS, det=True), hipgraph)
    table, cam_of = det_trainer.model.camera
    assert tuple(table.shape) == (2, 19) and cam_of.tolist() == [0, 1, 0] and table.is_cuda and cam_of.is_cuda
    _assert_same_poses(mixed, plain, "detections")
    assert pred_m["camera"]["depth_unit"].tolist() == [0.001, 0.0005, 0.001]


@pytest.mark.parametrize("hipgraph", [False, True], ids=["eager", "hipgraph"])
def test_mixed_batch_from_an_image_fit_tracks_to_the_plain_poses(fit_trainer, hipgraph):
    """The same with the first pose fitted from frame 0's images: the fit back-projects trajectory 1 with its own unit too."""
    plain, _ = _run(fit_trainer, _data(None, coord=True), hipgraph)
    mixed, pred = _run(fit_trainer, _data(CAMERAS, coord=True), hipgraph)
    _assert_same_poses(mixed, plain, "image fit")
    assert pred["image_fit"]["valid"].tolist() == [1] * BATCH


def test_an_ignored_camera_would_show(fit_trainer):
    """What the comparison above is worth: the scaled trajectory WITHOUT its camera (the frames as a build without the feature reads them)
    starts from another pose -- the object at twice its distance."""
    data = _data(CAMERAS, coord=True, frames=2)
    for f in data:
        del f["meta"]["pre_fetched"]["camera"]
    ignored, _ = _run(fit_trainer, data)
    plain, _ = _run(fit_trainer, _data(None, coord=True, frames=2))
    t_i, t_p = ignored[0]["translation"][:, 0, :, 0], plain[0]["translation"][:, 0, :, 0]
    assert torch.equal(t_i[0], t_p[0]) and torch.equal(t_i[2], t_p[2])
    assert abs(float(t_i[1, 2] / t_p[1, 2]) - 2.0) < 0.05


def test_two_lanes_slice_the_cameras(device):
    """B = 32 as two lanes with the deferred check (16 copies of a millimetre trajectory, then 16 of a half-millimetre one: lane 1's
    cam_of is the second half) == the plain run's poses, and == the single batch."""
    from captra_amd.synthetic import cat_trajectories, make_otf_trajectory
    trainer = _trainer(device)

    def data(scaled):
        parts = [make_otf_trajectory(1, 3, seed=s, cameras=None if not scaled else [cam]) for s, cam in ((2, CAMERAS[0]), (3, CAMERAS[1]))]
        return cat_trajectories([p for p in parts for _ in range(16)])

    plain, _ = _run(trainer, data(False), hipgraph=True, lanes=True)
    mixed, _ = _run(trainer, data(True), hipgraph=True, lanes=True)
    assert trainer.model.camera[1].tolist() == [0] * 16 + [1] * 16
    _assert_same_poses(mixed, plain, "lanes")
    single, _ = _run(trainer, data(True), hipgraph=True, lanes=False)
    _assert_same_poses(single, mixed, "single batch")


def test_option_absent_and_the_pickle(det_trainer, tmp_path):
    """No camera anywhere: the model's camera is None, the plain entry points are called and the pickle has no `camera` entry; with the
    frames' cameras the *_cam entry points are called and the pickle carries each trajectory's K and depth unit, which eval lists."""
    import pickle
    from captra_amd import _lib, eval as ev
    model = det_trainer.model
    model.cfg["experiment_dir"] = str(tmp_path)
    calls, real = [], _lib.call
    _lib.call = lambda name, *args: (calls.append(name), real(name, *args))[1]
    try:
        _run(det_trainer, _data(None, det=True, frames=2), save=True)
        off = set(calls)
        assert model.camera is None and model.camera_cfg is None
        with open(tmp_path / "results" / "data" / f"inst{TRAJ_SEED}_track0.pkl", "rb") as f:
            assert "camera" not in pickle.load(f)
        del calls[:]
        _run(det_trainer, _data(CAMERAS, det=True, frames=2), save=True)
        on = set(calls)
    finally:
        _lib.call = real
    assert {"captra_crop_box_det", "captra_crop_ball_det"} <= off and not any(n.endswith("_cam") for n in off)
    assert {"captra_crop_box_det_cam", "captra_crop_ball_det_cam"} <= on and not {"captra_crop_box_det", "captra_crop_ball_det", "captra_crop_ball"} & on
    with open(tmp_path / "results" / "data" / f"inst{TRAJ_SEED + 1}_track0.pkl", "rb") as f:
        rec = pickle.load(f)
    assert np.asarray(rec["camera"]["K"]).reshape(3, 3).tobytes() == np.array([[591.0125, 0, 322.525], [0, 590.16775, 244.11084], [0, 0, 1]]).tobytes()
    assert float(rec["camera"]["depth_unit"]) == 0.0005
    assert ev.camera_table("t", rec) == ["t: fx 591.013; fy 590.168; cx 322.525; cy 244.111; depth unit 0.0005 m"]


def test_host_box_branch_and_rare_path_read_the_rows_camera(device):
    """full_data_batch_arrays with the pose on the HOST (each row's box projected with its own K) == the device-pose form, on three
    rows over three cameras (one skewed); and with trajectory 1's counts doubled under a halved unit, a ball of fewer than 10 members
    on it (the rare path: the torch restatement with the instance's K and unit) == the plain call's points, byte for byte."""
    from captra_amd import nocs_otf
    c = I.chain_inputs()
    dev = torch.device(device)
    gt = {"rotation": c["rot"], "translation": c["gt_trans"], "scale": c["gt_scale"]}
    scale = c["scale"].copy()
    depth = c["depth"].copy()
    depth[1] *= 2
    mask_d = torch.from_numpy(c["mask"]).to(dev)

    def both(K3, units, dimg, trans32, scale32):
        cams = nocs_otf.camera_table(np.stack(K3), units, dev)
        d = torch.from_numpy(dimg).to(dev)
        np.random.seed(0)
        on_dev = nocs_otf.full_data_batch_arrays(d, mask_d, None, None, gt, I.CHAIN_N, cameras=cams,
                                                 pose_dev=(torch.from_numpy(trans32).to(dev), torch.from_numpy(scale32).to(dev), I.CHAIN_FACTOR))
        np.random.seed(0)
        on_host = nocs_otf.full_data_batch_arrays(d, mask_d, trans32.astype(np.float64), np.float64(I.CHAIN_FACTOR) * scale32.astype(np.float64), gt,
                                                  I.CHAIN_N, cameras=cams)
        for k in ("points", "labels", "nocs"):
            assert torch.equal(on_dev[k], on_host[k]), k
        return on_dev

    # a skewed third camera: the rows' boxes differ by camera, and the two forms agree
    skew = both([I.K, I.K, C.SKEW_K], [0.001, 0.0005, 0.001], depth, c["trans"], scale)
    same_k = both([I.K, I.K, I.K], [0.001, 0.0005, 0.001], depth, c["trans"], scale)
    assert torch.equal(skew["points"][:2], same_k["points"][:2]) and not torch.equal(skew["points"][2], same_k["points"][2])
    def plain_call(trans32, scale32):
        np.random.seed(0)
        return nocs_otf.full_data_batch_arrays(torch.from_numpy(c["depth"]).to(dev), mask_d, None, None, gt, I.CHAIN_N, intrinsics=I.K,
                                               pose_dev=(torch.from_numpy(trans32).to(dev), torch.from_numpy(scale32).to(dev), I.CHAIN_FACTOR))

    plain = plain_call(c["trans"], scale)
    for k in ("points", "labels", "nocs"):
        assert torch.equal(same_k[k], plain[k]), k
    # trajectory 1 with a ball of fewer than 10 members -- the 0.05 m floor of the radius, the centre 45 mm behind the surface --: the
    # radius grows on the torch path, in the instance's own unit
    small, back = scale.copy(), c["trans"].copy()
    small[1] = np.float32(0.02)
    back[1, 2] += np.float32(0.045)
    ctr = back.astype(np.float64)[1]
    count = C.crop_ball(c["depth"][1], c["mask"][1], C.project(I.H, I.W, ctr[None], [0.012], I.K)[0], ctr, 0.05, np.linalg.inv(I.K).reshape(9), 0.001,
                        10 ** 6, I.H, I.W)[3]
    assert 0 < count < 10, count
    rare = both([I.K, I.K, I.K], [0.001, 0.0005, 0.001], depth, back, small)
    plain = plain_call(back, small)
    for k in ("points", "labels", "nocs"):
        assert torch.equal(rare[k], plain[k]), k


def test_shifted_principal_point(device):
    """One frame through full_data_batch_arrays: the images padded by q zero-depth columns on the left and p rows at the bottom under the
    camera with cx + q, cy + p (v = h - row: bottom padding shifts v) -- the same crop.  The sampled points agree to 1e-12 m: a handful
    of float64 roundings on values of about 1 m, derived from the arithmetic; no pixel of either image is within 1e-9 m of its sphere
    (tests/test_camera_judge_cpu.py), so none changes sides.  The kernels' member tables hold the same pixels in the same order."""
    from captra_amd import nocs_otf
    from tests.test_camera_gpu import _crop_ball, _crop_box
    s = C.shifted_inputs()
    dev = torch.device(device)
    gt = {"rotation": s["rot"], "translation": s["gt_trans"], "scale": s["gt_scale"]}
    pose = (torch.from_numpy(s["trans"]).to(dev), torch.from_numpy(s["scale"]).to(dev), I.CHAIN_FACTOR)
    out, tables = {}, {}
    for key in ("plain", "shifted"):
        depth, mask, K = s[key]
        cams = nocs_otf.camera_table(np.stack([K] * 3), [0.001] * 3, dev)
        assert tuple(cams[0].shape) == (1, 19)
        np.random.seed(0)
        out[key] = nocs_otf.full_data_batch_arrays(torch.from_numpy(depth).to(dev), torch.from_numpy(mask).to(dev), None, None, gt, I.CHAIN_N,
                                                   pose_dev=pose, cameras=cams)
        h, w = depth.shape[1:]
        tab = C.table([(K, 0.001)])
        _, box = _crop_box(device, h, w, s["trans"], s["scale"], I.CHAIN_FACTOR, tab=tab, cam_of=np.zeros(3, np.int32))
        case = I.ball_case(key, depth, mask, box["box"], box["center"], box["radius"], h * w, h, w, K)
        err, tables[key] = _crop_ball(device, case, tab, np.zeros(3, np.int32))
        assert err == 0
    a, b = out["plain"], out["shifted"]
    assert torch.equal(a["labels"], b["labels"]) and a["points"].dtype == torch.float64
    assert float((a["points"] - b["points"]).abs().max()) <= 1e-12
    assert float((a["nocs"] - b["nocs"]).abs().max()) <= 1e-11                              # (the points' difference divided by a scale >= 0.2)
    (pts1, obj1, pix1, cnt1), (pts2, obj2, pix2, cnt2) = tables["plain"], tables["shifted"]
    assert (cnt1[:, 0] == cnt2[:, 0]).all() and (cnt1[:, 0] >= 10).all()
    for i in range(3):
        k = int(cnt1[i, 0])
        np.testing.assert_array_equal((pix1[i, :k] // I.W) * (I.W + C.SHIFT_Q) + pix1[i, :k] % I.W + C.SHIFT_Q, pix2[i, :k])
        np.testing.assert_array_equal(obj1[i, :k], obj2[i, :k])
        assert np.abs(pts1[i, :k] - pts2[i, :k]).max() <= 1e-12
