"""The on-the-fly re-crop loop with flying depth pixels removed from every uploaded depth image (track_cfg/depth_filter, captra_amd/model.py;
include/captra_hip.h: captra_depth_support_filter) on the scene that has the defect, make_otf_trajectory(..., flying=0.5): the device
images and the recorded counts are the judge's (tests/depth_judge.py), the re-crop's candidate list loses every injected pixel, the
eager and the captured loop agree bit for bit, and without the option nothing changes."""
import pickle

import numpy as np
import pytest
import torch

from tests import depth_judge as J
from tests.weights import make_physical_state_dict

pytestmark = pytest.mark.gpu

FRAMES, BATCH, FLYING = 3, 2, 0.5
TRAJ_SEED, WEIGHT_SEED, RUN_SEED = 1, 31, 5001
OPTION = {"window": 3, "abs_mm": 10, "min_support": 12}
RULE = dict(window=3, abs_mm=10, rel_permille=0, min_support=12)
ABSENT, NULL = "absent", "null"


def _data():
    from captra_amd.synthetic import make_otf_trajectory
    return make_otf_trajectory(BATCH, FRAMES, seed=TRAJ_SEED, flying=FLYING)


def _trainer(device, option):
    """A track model with the seeded weights; option: the track_cfg/depth_filter section, NULL (the key set to None) or ABSENT (a
    configuration that never had the key)."""
    from captra_amd.configs import make_config
    from captra_amd.trainer import Trainer
    cfg = make_config("1", experiment_dir="/tmp/captra_depth_filter_test", nocs_otf=True)
    cfg["device"] = device
    cfg["init_frame"]["gt"] = True
    assert "depth_filter" not in cfg["track_cfg"]
    if option != ABSENT:
        cfg["track_cfg"]["depth_filter"] = None if option == NULL else dict(option)
    trainer = Trainer(cfg)
    model = trainer.model
    model.load_state_dict(make_physical_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, WEIGHT_SEED, 1, True, "nocs"))
    return trainer


@pytest.fixture(scope="module")
def trainers(device):
    return {"on": _trainer(device, OPTION), NULL: _trainer(device, NULL), ABSENT: _trainer(device, ABSENT)}


def _run(trainer, data, hipgraph, save=False):
    """One seeded loop -> (poses of frames 1.., pred_dict)."""
    model = trainer.model
    model.use_graph = hipgraph
    torch.manual_seed(RUN_SEED); np.random.seed(RUN_SEED)
    pred, _ = trainer.test(data, save=save, no_eval=True)
    poses = [{k: pred["poses"][i][k].clone() for k in ("rotation", "translation", "scale")} for i in range(1, len(data))]
    return poses, dict(model.pred_dict)


def _assert_same_poses(a, b):
    assert len(a) == len(b)
    for i, (pa, pb) in enumerate(zip(a, b)):
        for key in pa:
            assert torch.equal(pa[key], pb[key]), (key, i + 1)


@pytest.fixture(scope="module")
def judged():
    """The scene and, per frame, the judge's (image, counts) of its depth images: computed once, left unchanged."""
    data = _data()
    return data, [J.judge(f["meta"]["pre_fetched"]["depth"].numpy(), **RULE) for f in data]


@pytest.fixture(scope="module")
def eager_on(trainers, judged):
    return _run(trainers["on"], judged[0], hipgraph=False)


def test_device_depth_and_counts_are_the_judges(trainers, judged, eager_on):
    """(a) every frame's device image and pred_dict['depth_filter'] entry, frame 0 included."""
    data, want = judged
    model = trainers["on"].model
    record = eager_on[1]["depth_filter"]
    assert len(record) == FRAMES
    for i in range(FRAMES):
        dev = model.feed_dict[i]["pre_fetched"]["depth"]
        assert dev.dtype == torch.int32 and tuple(dev.shape) == (BATCH, 480, 640)
        assert np.array_equal(dev.cpu().numpy(), want[i][0]), i
        assert record[i].dtype == torch.int32 and record[i].is_cuda and tuple(record[i].shape) == (BATCH,)
        assert record[i].cpu().tolist() == want[i][1].tolist(), i
        injected = data[i]["meta"]["pre_fetched"]["flying"].numpy()
        assert want[i][1].tolist() == injected.sum(axis=(1, 2)).tolist()           # (the scene's condition: all of them, nothing else)


def test_counts_reach_the_pickle_and_the_eval_table(trainers, judged, tmp_path, capsys):
    """(a) --save: every trajectory's pickle carries its counts, and `python -m captra_amd.eval` lists them."""
    from captra_amd import eval as ev
    data, want = judged
    model = trainers["on"].model
    model.cfg["experiment_dir"] = str(tmp_path)
    _run(trainers["on"], data, hipgraph=False, save=True)
    names = sorted(p.name for p in (tmp_path / "results" / "data").iterdir())
    assert names == [f"inst{TRAJ_SEED + b}_track0.pkl" for b in range(BATCH)]
    lines = []
    for b, name in enumerate(names):
        with open(tmp_path / "results" / "data" / name, "rb") as f:
            rec = pickle.load(f)
        got = [int(np.asarray(r["removed"])) for r in rec["depth_filter"]]
        assert got == [int(want[i][1][b]) for i in range(FRAMES)]
        lines += ev.depth_filter_table(name.rsplit(".", 1)[0], rec)
        assert f"removed {sum(got)} pixels in {FRAMES} frames" in lines[-1]
    capsys.readouterr()
    ev.main(["--obj_category", "1", "--experiment_dir", str(tmp_path), "--eval_device"])
    printed = capsys.readouterr().out
    assert "track_cfg/depth_filter" in printed and all(line in printed for line in lines)


def _candidate_pixels(depth, mask, center, radius, num_points):
    """Row-major pixel numbers of the re-crop's candidate list of one image (nocs_otf.crop_candidates: the ball members among the
    box's depth-carrying pixels, in the order the list has them)."""
    from captra_amd.nocs_otf import crop_candidates, proj_corners
    H, W = depth.shape
    box = proj_corners(H, W, center, radius)
    r0, c0, r1, c1 = int(box[0, 0]), int(box[0, 1]), int(box[1, 0]), int(box[1, 1])
    rc = torch.nonzero(depth[r0:r1 + 1, c0:c1 + 1] > 0)
    pts, _, idx, perm = crop_candidates(depth, mask, center, radius, num_points)
    assert pts.shape[0] == rc.shape[0] and perm is None
    return ((rc[:, 0] + r0) * W + rc[:, 1] + c0)[idx].cpu().numpy()


def test_recrop_candidates_lose_the_flying_pixels(trainers, judged, eager_on):
    """(b) frame 1 re-cropped around the pose that entered it: the candidate list built from the model's own (filtered) device image
    holds none of the injected pixels, built from the uploaded image it holds some -- in every trajectory."""
    data, _ = judged
    model = trainers["on"].model
    pose0 = eager_on[1]["poses"][0]
    N = model.feed_dict[1]["points"].shape[2]
    pre = model.feed_dict[1]["pre_fetched"]
    raw = data[1]["meta"]["pre_fetched"]["depth"].to(pre["depth"].device).int()
    for b in range(BATCH):
        center = pose0["translation"][b, model.root].reshape(3).double().cpu().numpy()
        radius = float(model.radius) * float(pose0["scale"][b, model.root])
        injected = np.flatnonzero(data[1]["meta"]["pre_fetched"]["flying"][b].numpy().reshape(-1))
        filtered = _candidate_pixels(pre["depth"][b], pre["mask"][b], center, radius, N)
        unfiltered = _candidate_pixels(raw[b], pre["mask"][b], center, radius, N)
        hit = np.isin(unfiltered, injected).sum()
        print(f"trajectory {b}: {len(unfiltered)} candidates with {hit} injected pixels; filtered {len(filtered)}")
        assert len(filtered) >= 10 and not np.isin(filtered, injected).any()
        assert hit >= 1
        assert len(np.unique(filtered)) == len(np.unique(unfiltered)) - len(np.unique(unfiltered[np.isin(unfiltered, injected)]))


def test_eager_and_captured_loop_agree(trainers, judged, eager_on):
    """(c) hipgraph=True against the eager loop: poses bit-identical, the same record."""
    graph = _run(trainers["on"], judged[0], hipgraph=True)
    _assert_same_poses(eager_on[0], graph[0])
    for a, b in zip(eager_on[1]["depth_filter"], graph[1]["depth_filter"]):
        assert torch.equal(a, b)


def test_eager_and_captured_loop_agree_on_two_lanes(trainers):
    """(c) once at the smallest batch the re-crop's two lanes accept (32: 16 copies of two trajectories)."""
    from captra_amd.synthetic import cat_trajectories, make_otf_trajectory
    singles = [make_otf_trajectory(1, FRAMES, seed=s, flying=FLYING) for s in (TRAJ_SEED, TRAJ_SEED + 1)]
    data = lambda: cat_trajectories([singles[b % 2] for b in range(32)])
    model = trainers["on"].model
    assert model.otf_lanes and model._otf_lanes_usable({"points": torch.empty(32, 3, 8, device=model.device)})
    assert not model._otf_lanes_usable({"points": torch.empty(30, 3, 8, device=model.device)})
    eager = _run(trainers["on"], data(), hipgraph=False)
    graph = _run(trainers["on"], data(), hipgraph=True)
    _assert_same_poses(eager[0], graph[0])
    for a, b in zip(eager[1]["depth_filter"], graph[1]["depth_filter"]):
        assert torch.equal(a, b) and tuple(a.shape) == (32,) and torch.equal(a[:2], a[2:4]) and int(a.min()) > 0


def test_option_absent_changes_nothing(trainers, judged, eager_on, monkeypatch):
    """(d) the key set to None: no launch of the filter, no record, the device image is the upload, and the poses are those of a model
    whose configuration never had the key -- which are not the poses of the filtered run."""
    from captra_amd import _lib
    data, _ = judged
    calls, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *args: (calls.append(name), real(name, *args))[1])
    null = _run(trainers[NULL], data, hipgraph=False)
    monkeypatch.setattr(_lib, "call", real)
    assert calls and "captra_depth_support_filter" not in calls
    assert trainers[NULL].model.depth_filter is None and "depth_filter" not in null[1]
    for i in range(FRAMES):
        frame = trainers[NULL].model.feed_dict[i]
        assert "depth_filter_removed" not in frame
        assert torch.equal(frame["pre_fetched"]["depth"].cpu(), data[i]["meta"]["pre_fetched"]["depth"].int())
    absent = _run(trainers[ABSENT], data, hipgraph=False)
    assert "depth_filter" not in absent[1]
    _assert_same_poses(null[0], absent[0])
    assert any(not torch.equal(a[k], b[k]) for a, b in zip(eager_on[0], absent[0]) for k in a)
