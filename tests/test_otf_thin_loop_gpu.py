"""The on-the-fly re-crop loop with its over-long candidate lists thinned on the device (track_cfg/otf_thin, captra_amd/model.py,
nocs_otf.py; include/captra_hip.h: captra_otf_thin) at the timed configuration: num_points 4096, the close-up scene
make_otf_trajectory(..., blob_px=90) whose crops hold about 25 000 ball members -- more than the 5 x 4096 an unthinned list holds.
Without the option every frame of that scene is a rare-path frame (run twice); with it none is, and the sync-free stage, the
synchronous stage and the two lanes produce the same clouds and poses bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FRAMES, CLOSE_UP = 4, 90
TRAJ_SEEDS, WEIGHT_SEED, RUN_SEED = (1, 2), 31, 5001


def _data(blob_px, batch32=False):
    from captra_amd.synthetic import cat_trajectories, make_otf_trajectory
    if not batch32:
        return make_otf_trajectory(1, FRAMES, seed=TRAJ_SEEDS[0], blob_px=blob_px)
    return cat_trajectories([make_otf_trajectory(1, FRAMES, seed=s, blob_px=blob_px) for s in TRAJ_SEEDS for _ in range(16)])


@pytest.fixture(scope="module")
def trainers(device):
    """(option on, option off): two track models with the same seeded weights."""
    from captra_amd.configs import make_config
    from captra_amd.synthetic import make_physical_state_dict
    from captra_amd.trainer import Trainer
    out = []
    for on in (True, False):
        cfg = make_config("1", experiment_dir="/tmp/captra_otf_thin_test", nocs_otf=True, hipgraph=True)
        cfg["device"] = device
        cfg["init_frame"]["gt"] = True
        if on:
            cfg["track_cfg"]["otf_thin"] = {"device": True, "seed": 7}
        trainer = Trainer(cfg)
        model = trainer.model
        model.load_state_dict(make_physical_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, WEIGHT_SEED, 1, True, "nocs"))
        out.append(trainer)
    return out


def _run(trainer, data, lanes=False):
    """One seeded loop -> (clouds of frames 1.., poses of frames 1.., pred_dict, numpy's generator state, torch's CPU generator state)."""
    model = trainer.model
    model.otf_lanes = lanes
    torch.manual_seed(RUN_SEED); np.random.seed(RUN_SEED)
    pred, _ = trainer.test(data, save=False, no_eval=True)
    clouds = [model.feed_dict[i]["points"].clone() for i in range(1, FRAMES)]
    poses = [{k: pred["poses"][i][k].clone() for k in ("rotation", "translation", "scale")} for i in range(1, FRAMES)]
    return clouds, poses, dict(model.pred_dict), np.random.get_state(), torch.get_rng_state()


def _assert_same(a, b):
    for i, (ca, cb) in enumerate(zip(a[0], b[0])):
        assert torch.equal(ca, cb), f"cloud of frame {i + 1}"
    for i, (pa, pb) in enumerate(zip(a[1], b[1])):
        for key in pa:
            assert torch.equal(pa[key], pb[key]), (key, i + 1)


def _same_np_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.fixture(scope="module")
def close_up_on(trainers):
    """The option on, close-up scene, single batch, sync-free stage: the run the other forms are compared with -- and every verdict
    its deferred checks read."""
    import captra_amd.model as M
    reads = []
    orig = M._OtfCheck.read
    M._OtfCheck.read = lambda self: (reads.append(orig(self)), reads[-1])[1]
    try:
        run = _run(trainers[0], _data(CLOSE_UP))
    finally:
        M._OtfCheck.read = orig
    return run, reads


def test_close_up_has_no_rare_frame_with_the_option(close_up_on):
    """1. Every deferred verdict says 'not rare' (without the option every one of them says 'rare': the lists are longer than 5 N),
    and pred_dict['otf_thin'] counts every trajectory on every frame."""
    run, reads = close_up_on
    assert len(reads) >= FRAMES - 1
    assert not any(rare for rare, _ in reads), reads
    assert all(longest == 5 * 4096 for _, longest in reads), reads
    record = run[2]["otf_thin"]
    assert record[0] is None and len(record) == FRAMES
    assert [int(r.sum()) for r in record[1:]] == [1] * (FRAMES - 1) and all(tuple(r.shape) == (1,) for r in record[1:])


def test_close_up_deferred_equals_synchronous_stage(trainers, close_up_on, monkeypatch):
    """2. The sync-free stage against CAPTRA_OTF_DEFER off: clouds and poses bit-equal on every frame."""
    import captra_amd.model as M
    monkeypatch.setattr(M, "OTF_DEFER", False)
    sync = _run(trainers[0], _data(CLOSE_UP))
    _assert_same(close_up_on[0], sync)
    assert [int(r.sum()) for r in sync[2]["otf_thin"][1:]] == [1] * (FRAMES - 1)


def test_close_up_two_lanes_equal_the_single_batch(trainers):
    """3. B = 32 (16 copies of two trajectories) as two lanes against the single batch: bit-equal -- a lane draws what the whole batch
    draws.  Copies of a trajectory sit at different places of the batch, so they are thinned differently."""
    lanes = _run(trainers[0], _data(CLOSE_UP, True), lanes=True)
    single = _run(trainers[0], _data(CLOSE_UP, True), lanes=False)
    _assert_same(lanes, single)
    for a, b in zip(lanes[2]["otf_thin"][1:], single[2]["otf_thin"][1:]):
        assert torch.equal(a, b) and int(a.sum()) == 32
    assert not torch.equal(single[0][0][0], single[0][0][2])          # trajectories 0 and 2: the same scene, another subset


def test_nothing_thinned_equals_option_off(trainers):
    """4. blob_px = 70, where no list is over-long: clouds and poses bit-equal to the option off, numpy's generator state too, and no
    instance is recorded as thinned."""
    from captra_amd.synthetic import make_otf_trajectory
    data = lambda: make_otf_trajectory(1, FRAMES, seed=TRAJ_SEEDS[0])
    on, off = _run(trainers[0], data()), _run(trainers[1], data())
    _assert_same(on, off)
    assert _same_np_state(on[3], off[3]) and torch.equal(on[4], off[4])
    assert [int(r.sum()) for r in on[2]["otf_thin"][1:]] == [0] * (FRAMES - 1) and "otf_thin" not in off[2]


def test_close_up_draws_nothing_from_numpy(trainers, close_up_on):
    """5. The option on uses no numpy draw for thinning: after the close-up run numpy's generator stands where the seed put it, and
    torch's CPU generator where the frames' consume_noise_draws alone put it."""
    from captra_amd.pose_utils.part_dof_utils import consume_noise_draws
    model = trainers[0].model
    torch.manual_seed(RUN_SEED); np.random.seed(RUN_SEED)
    want_np = np.random.get_state()
    shape = {"scale": torch.empty(1, model.num_parts)}
    for _ in range(1, FRAMES):
        consume_noise_draws(shape, model.pose_perturb_cfg)
    assert _same_np_state(close_up_on[0][3], want_np)
    assert torch.equal(close_up_on[0][4], torch.get_rng_state())


def test_a_bound_outgrown_is_outgrown_once(trainers, close_up_on, monkeypatch):
    """A first stride bound of N (below T = 5 N): frame 1's thinned list outgrows it, the frame is flagged and run again -- and under the
    option the next frame's bound follows that verdict's longest list, so no later frame is flagged (left stale, every frame would
    be).  The replayed frame and the rest equal the run that never outgrew its bound."""
    import captra_amd.model as M
    monkeypatch.setattr(M, "OTF_FIRST_BOUND", 1)
    reads = []
    orig = M._OtfCheck.read
    monkeypatch.setattr(M._OtfCheck, "read", lambda self: (reads.append(orig(self)), reads[-1])[1])
    run = _run(trainers[0], _data(CLOSE_UP))
    assert [rare for rare, _ in reads] == [True] + [False] * (FRAMES - 2), reads
    _assert_same(run, close_up_on[0])


def test_thinned_frames_reach_the_pickle_and_the_eval_table(trainers):
    """--save: the per-trajectory record carries the frames' flags, and captra_amd.eval's table counts them."""
    from captra_amd.eval import otf_thin_table
    model = trainers[0].model
    sunk = []
    model.result_sink = sunk.extend
    try:
        model.otf_lanes = False
        torch.manual_seed(RUN_SEED); np.random.seed(RUN_SEED)
        trainers[0].test(_data(CLOSE_UP), save=True, no_eval=True)
    finally:
        model.result_sink = None
    (name, record), = sunk
    assert record["otf_thin"][0] is None and [int(r["thinned"]) for r in record["otf_thin"][1:]] == [1] * (FRAMES - 1)
    assert otf_thin_table(name.rsplit(".", 1)[0], record) == [f"{name.rsplit('.', 1)[0]}: thinned {FRAMES - 1} / {FRAMES - 1} frames"]


def test_option_needs_the_pose_on_the_device(trainers, monkeypatch):
    import captra_amd.model as M
    monkeypatch.setattr(M, "OTF_POSE_ON_DEVICE", False)
    with pytest.raises(ValueError, match="otf_thin"):
        _run(trainers[0], _data(CLOSE_UP))
