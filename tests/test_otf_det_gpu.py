"""The detector route of the on-the-fly re-crop (`--track_cfg/nocs2d_label True`) on the device: captra_crop_box_det against the
float64 judge (tests/det_judge.py, pinned to the reference by golden G16) bit for bit, captra_crop_ball_det against captra_crop_ball,
the route through nocs_otf.full_data_batch_arrays against G16's points / labels / NOCS, and the track loop in both forms of the stage."""
from pathlib import Path

import numpy as np
import pytest
import torch

from captra_amd import nocs_otf
from tests import det_judge
from tests.golden.make_golden_otf_det import CASES, CATEGORY, NUM_POINTS, RADIUS_FACTOR, make_case

pytestmark = pytest.mark.gpu
G16 = np.load(Path(__file__).resolve().parent / "golden" / "g16_otf_det.npz")
TAGS = [c[0] for c in CASES]


def _box_det(device, H, W, trans32, scale32, factor, boxes, cls, count, category, intrinsics=nocs_otf.NOCS_REAL_INTRINSICS):
    """captra_crop_box_det on host arrays -> dict of host arrays (the judge's keys)."""
    from captra_amd import _lib as L
    B, K = cls.shape
    dev = torch.device(device)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in (("trans", trans32.astype(np.float32)), ("scale", scale32.astype(np.float32)),
                                                                             ("boxes", boxes.astype(np.int32)), ("cls", cls.astype(np.int32)),
                                                                             ("count", count.astype(np.int32)))}
    kk = nocs_otf._intrinsics_on_device(intrinsics, dev)
    out = {"box": torch.empty(B, 4, dtype=torch.int32, device=dev), "center": torch.empty(B, 3, dtype=torch.float64, device=dev),
           "radius": torch.empty(B, dtype=torch.float64, device=dev), "radius_raw": torch.empty(B, dtype=torch.float64, device=dev),
           "sel": torch.full((B,), -7, dtype=torch.int32, device=dev)}
    with torch.cuda.device(dev):
        L.call("captra_crop_box_det", B, H, W, K, int(category), float(factor), L.ptr(t["trans"]), L.ptr(t["scale"]), kk.data_ptr(), L.ptr(t["boxes"]),
               L.ptr(t["cls"]), L.ptr(t["count"]), L.ptr(out["box"]), L.ptr(out["center"]), L.ptr(out["radius"]), L.ptr(out["radius_raw"]), L.ptr(out["sel"]))
    return {k: v.cpu().numpy() for k, v in out.items()}


def _equal_to_judge(got, want):
    for k in ("sel", "box"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    for k in ("radius", "radius_raw", "center"):
        assert got[k].tobytes() == want[k].astype(np.float64).tobytes(), (k, got[k], want[k])


def _golden_batch(K=4):
    """The five G16 cases as one batch, the detections padded to K slots with POISONED padding (the crop's own box, right class)."""
    cases = [make_case(t) for t in TAGS]
    B = len(cases)
    H, W = cases[0]["depth"].shape
    boxes = np.zeros((B, K, 4), np.int32)
    cls = np.full((B, K), CATEGORY, np.int32)
    masks = np.ones((B, K, H, W), np.uint8)
    count = np.zeros(B, np.int32)
    for b, c in enumerate(cases):
        n = len(c["det_class"])
        boxes[b] = nocs_otf.proj_corners(H, W, c["center"], c["radius"]).reshape(-1)
        boxes[b, :n], cls[b, :n], masks[b, :n], count[b] = c["det_boxes"], c["det_class"], c["det_masks"], n
    return cases, boxes, cls, masks, count


def test_selection_kernel_on_the_golden_cases(device):
    cases, boxes, cls, _, count = _golden_batch()
    H, W = cases[0]["depth"].shape
    trans, scale = np.stack([c["trans32"] for c in cases]), np.array([c["scale32"] for c in cases], np.float32)
    got = _box_det(device, H, W, trans, scale, RADIUS_FACTOR, boxes, cls, count, CATEGORY)
    _equal_to_judge(got, det_judge.select_batch(H, W, trans, scale, RADIUS_FACTOR, boxes, cls, count, CATEGORY))
    for b, tag in enumerate(TAGS):                     # and against the reference itself
        assert got["sel"][b] == int(G16[f"{tag}_sel"]) and got["radius_raw"][b].tobytes() == np.float64(G16[f"{tag}_radius"]).tobytes(), tag
        np.testing.assert_array_equal(got["box"][b].reshape(2, 2), G16[f"{tag}_corners"])


@pytest.mark.parametrize("B,K", [(1, 1), (5, 3), (5, 64), (1, 65), (5, 65)])
def test_selection_kernel_on_random_boxes(device, B, K):
    """Seeded random boxes on a 64 x 48 image with scaled intrinsics: hits, growth, give-ups, rows without the class, det_count below K
    with poisoned padding (a slot that would win), ties (duplicated boxes), K one past a wave."""
    H, W = 48, 64
    intr = nocs_otf.NOCS_REAL_INTRINSICS * np.array([[0.1], [0.1], [1.0]])
    for rep in range(4):
        rng = np.random.default_rng([B, K, rep])
        trans = np.stack([rng.uniform(-0.3, 0.3, B), rng.uniform(-0.25, 0.25, B), rng.uniform(-1.6, -0.9, B)], 1).astype(np.float32)
        scale = rng.choice([0.02, 0.1, 0.2, 0.5, 0.8], B).astype(np.float32)
        y1, x1 = rng.integers(-4, H, (B, K)), rng.integers(-4, W, (B, K))
        boxes = np.stack([y1, x1, y1 + rng.integers(0, 30, (B, K)), x1 + rng.integers(0, 30, (B, K))], -1).astype(np.int32)
        if K > 2:
            boxes[:, K // 2] = boxes[:, 0]                                     # ties
        cls = rng.integers(1, 4, (B, K)).astype(np.int32)
        cls[:, K // 2] = cls[:, 0]
        count = rng.integers(0, K + 1, B).astype(np.int32)
        count[0] = K if rep % 2 == 0 else count[0]
        if B > 1:
            cls[1] = 3                                                          # a row without the category
        for b in range(B):                                                      # poisoned padding: the whole image, right class
            boxes[b, count[b]:] = (0, 0, H - 1, W - 1)
            cls[b, count[b]:] = 1
        got = _box_det(device, H, W, trans, scale, 0.6, boxes, cls, count, 1, intr)
        want = det_judge.select_batch(H, W, trans, scale, 0.6, boxes, cls, count, 1, intr)
        _equal_to_judge(got, want)
        if B > 1:
            assert want["sel"][1] == -1


def test_rows_without_a_detection_equal_crop_box(device):
    from captra_amd import _lib as L
    rng = np.random.default_rng(9)
    B, K, H, W = 70, 3, 480, 640
    trans = np.stack([rng.uniform(-0.6, 0.6, B), rng.uniform(-0.5, 0.5, B), rng.uniform(-2.5, -0.4, B)], 1).astype(np.float32)
    scale = rng.uniform(0.01, 0.6, B).astype(np.float32)
    boxes = np.tile(np.array([0, 0, H - 1, W - 1], np.int32), (B, K, 1))
    cls = np.full((B, K), 2, np.int32)
    count = np.where(np.arange(B) % 2 == 0, 0, K).astype(np.int32)          # no detections at all / none of the category
    cls[np.arange(B) % 2 == 0] = 1                                          # (padding of the right class: takes no part)
    got = _box_det(device, H, W, trans, scale, 0.6, boxes, cls, count, 1)
    t_d, s_d = torch.from_numpy(trans).to(device), torch.from_numpy(scale).to(device)
    kk = nocs_otf._intrinsics_on_device(nocs_otf.NOCS_REAL_INTRINSICS, torch.device(device))
    box, ctr, rad = torch.empty(B, 4, dtype=torch.int32, device=device), torch.empty(B, 3, dtype=torch.float64, device=device), torch.empty(B, dtype=torch.float64, device=device)
    with torch.cuda.device(device):
        L.call("captra_crop_box", B, H, W, 0.6, L.ptr(t_d), L.ptr(s_d), kk.data_ptr(), L.ptr(box), L.ptr(ctr), L.ptr(rad))
    assert (got["sel"] == -1).all()
    np.testing.assert_array_equal(got["box"], box.cpu().numpy())
    assert got["center"].tobytes() == ctr.cpu().numpy().tobytes() and got["radius"].tobytes() == rad.cpu().numpy().tobytes()
    assert got["radius_raw"].tobytes() == (0.6 * scale.astype(np.float64)).tobytes()


def test_crop_ball_det_equals_crop_ball_with_the_selected_mask(device):
    from captra_amd import _lib as L
    cases, boxes, cls, masks, count = _golden_batch()
    B, K = cls.shape
    H, W = cases[0]["depth"].shape
    trans, scale = np.stack([c["trans32"] for c in cases]), np.array([c["scale32"] for c in cases], np.float32)
    j = det_judge.select_batch(H, W, trans, scale, RADIUS_FACTOR, boxes, cls, count, CATEGORY)
    assert (j["sel"] >= 0).any() and (j["sel"] < 0).any()
    dev = torch.device(device)
    depth = torch.from_numpy(np.stack([c["depth"].astype(np.int32) for c in cases])).to(dev)
    mask = torch.from_numpy(np.stack([c["mask"] for c in cases]).astype(np.uint8)).to(dev)
    picked = torch.from_numpy(np.stack([masks[b, j["sel"][b]] if j["sel"][b] >= 0 else cases[b]["mask"].astype(np.uint8) for b in range(B)])).to(dev)
    dm, sel = torch.from_numpy(masks).to(dev), torch.from_numpy(j["sel"]).to(dev)
    box, ctr, rad = (torch.from_numpy(np.ascontiguousarray(j[k])).to(dev) for k in ("box", "center", "radius"))
    kk = nocs_otf._intrinsics_on_device(nocs_otf.NOCS_REAL_INTRINSICS, dev)
    cap = nocs_otf.CROP_CAP

    def outs():
        return (torch.zeros(B, cap, 3, dtype=torch.float64, device=dev), torch.zeros(B, cap, dtype=torch.uint8, device=dev),
                torch.zeros(B, cap, dtype=torch.int32, device=dev), torch.zeros(B, 2, dtype=torch.int32, device=dev))
    a, b_ = outs(), outs()
    with torch.cuda.device(dev):
        L.call("captra_crop_ball", B, H, W, cap, L.ptr(depth), L.ptr(picked), L.ptr(box), L.ptr(ctr), L.ptr(rad), kk.data_ptr() + 72, *map(L.ptr, a))
        L.call("captra_crop_ball_det", B, H, W, cap, K, L.ptr(depth), L.ptr(mask), L.ptr(dm), L.ptr(sel), L.ptr(box), L.ptr(ctr), L.ptr(rad),
               kk.data_ptr() + 72, *map(L.ptr, b_))
    for x, y in zip(a, b_):
        assert torch.equal(x, y)
    assert int(a[3][:, 0].min()) > 0 and bool((a[1] != 0).any())


def _gt_of(cases):
    return {"rotation": np.stack([np.asarray(c["pose"]["rotation"], np.float64).reshape(3, 3) for c in cases]),
            "translation": np.stack([np.asarray(c["pose"]["translation"], np.float64).reshape(3) for c in cases]),
            "scale": np.array([float(np.asarray(c["pose"]["scale"]).reshape(-1)[0]) for c in cases])}


def test_detector_route_vs_reference_golden(device):
    """Golden G16 end to end (the reference's full_data_from_depth_image with mask_from_nocs2d): every case on its own, as the reference
    ran it (the thinning permutation of a case comes out of numpy's generator seeded for that case), incl. `grow`'s larger crop and
    `giveup`'s whole-image one; tolerances of test_crop_and_resample_vs_reference_gpu (golden G11)."""
    cases, boxes, cls, masks, count = _golden_batch()
    dev = torch.device(device)
    for b, (tag, seed, _) in enumerate(CASES):
        c = cases[b]
        det = {"det_boxes": torch.from_numpy(boxes[b:b + 1]).to(dev), "det_class": torch.from_numpy(cls[b:b + 1]).to(dev),
               "det_count": torch.from_numpy(count[b:b + 1]).to(dev), "det_masks": torch.from_numpy(masks[b:b + 1]).to(dev), "category": CATEGORY}
        np.random.seed(100 + seed)
        full = nocs_otf.full_data_batch_arrays(torch.from_numpy(c["depth"].astype(np.int32))[None].to(dev), torch.from_numpy(c["mask"])[None].to(dev), None, None,
                                               _gt_of([c]), NUM_POINTS, pose_dev=(torch.from_numpy(c["trans32"])[None].to(dev),
                                                                                  torch.tensor([c["scale32"]], device=dev), RADIUS_FACTOR), det=det)
        np.testing.assert_allclose(full["points"][0].cpu().numpy(), G16[f"{tag}_points"], atol=1e-15, rtol=0, err_msg=tag)
        np.testing.assert_array_equal(full["labels"][0].cpu().numpy(), G16[f"{tag}_labels"], err_msg=tag)
        np.testing.assert_allclose(full["nocs"][0].cpu().numpy(), G16[f"{tag}_nocs"], atol=1e-12, rtol=0, err_msg=tag)


def test_rare_path_frame_crops_with_the_selected_mask_and_grown_radius(device):
    """Synchronous stage, trajectories whose ball holds fewer than 10 depth pixels (the centre 6 cm further behind the surface): they take the
    torch path on the host, which must see the selected mask and the radius as the selection grew it -- row 1 selects at once, row 2
    after growth; row 0 is an ordinary crop.  == the same frames handed those masks and radii directly (pose through the host)."""
    from captra_amd.synthetic import make_frame
    depth, mask, center, pose = make_frame(3)
    H, W = depth.shape
    dev = torch.device(device)
    behind = np.asarray(center, np.float32) + np.array([0, 0, -0.06], np.float32)
    trans = np.stack([np.asarray(center, np.float32), behind, behind])
    scale = np.array([0.12 / 0.6, 0.004 / 0.6, 0.004 / 0.6], np.float32)
    shifted = np.zeros_like(mask)
    shifted[3:, 5:] = mask[:-3, :-5]
    box0 = [nocs_otf.proj_corners(H, W, trans[b].astype(np.float64), 0.6 * np.float64(scale[b])).reshape(-1) for b in range(3)]
    boxes = np.zeros((3, 2, 4), np.int32)
    boxes[:, 0] = (5, 5, 40, 40)                                               # wrong class
    boxes[0, 1], boxes[1, 1] = box0[0], box0[1]
    boxes[2, 1] = (box0[2][0], box0[2][3] + 3, box0[2][2], box0[2][3] + 60)    # beside the box: reached after growth
    cls = np.tile(np.array([2, CATEGORY], np.int32), (3, 1))
    count = np.full(3, 2, np.int32)
    masks = np.stack([np.stack([np.ones_like(mask), shifted])] * 3).astype(np.uint8)
    j = det_judge.select_batch(H, W, trans, scale, 0.6, boxes, cls, count, CATEGORY)
    assert j["sel"].tolist() == [1, 1, 1] and j["rounds"][0] == 0 and j["rounds"][1] == 0 and j["rounds"][2] > 0
    # rows 1 and 2 really are rare: fewer than 10 valid pixels within the (clamped) radius of the centre
    rr, cc = np.nonzero(depth > 0)
    ray = (np.linalg.inv(nocs_otf.NOCS_REAL_INTRINSICS) @ np.stack([cc, H - rr, np.ones_like(cc)]).astype(np.float64)).T
    p = ray * depth[rr, cc].astype(np.float64)[:, None] / ray[:, 2:3]
    p = np.stack([p[:, 0], p[:, 1], -p[:, 2]], 1) * 0.001
    for b in (1, 2):
        assert int((np.sqrt(((p - trans[b].astype(np.float64)) ** 2).sum(-1)) <= j["radius"][b] * (1 + 1e-9)).sum()) < 10
    d = torch.from_numpy(np.stack([depth.astype(np.int32)] * 3)).to(dev)
    gt = _gt_of([{"pose": pose}] * 3)
    det = {"det_boxes": torch.from_numpy(boxes).to(dev), "det_class": torch.from_numpy(cls).to(dev), "det_count": torch.from_numpy(count).to(dev),
           "det_masks": torch.from_numpy(masks).to(dev), "category": CATEGORY}
    np.random.seed(3)
    got = nocs_otf.full_data_batch_arrays(d, torch.from_numpy(np.stack([mask] * 3)).to(dev), None, None, gt, NUM_POINTS,
                                          pose_dev=(torch.from_numpy(trans).to(dev), torch.from_numpy(scale).to(dev), 0.6), det=det)
    np.random.seed(3)
    want = nocs_otf.full_data_batch_arrays(d, torch.from_numpy(np.stack([shifted] * 3)).to(dev), trans.astype(np.float64), j["radius_raw"], gt, NUM_POINTS)
    for k in ("points", "labels", "nocs"):
        assert torch.equal(got[k], want[k]), k
    assert int((got["labels"][1] == 0).sum()) > 0


# ---- the track loop ------------------------------------------------------------------------------------------------------------
def _loop_data(B, T, N, seed, detections):
    from captra_amd.synthetic import make_otf_detections, make_otf_trajectory
    data = make_otf_detections(B, T, seed=seed) if detections else make_otf_trajectory(B, T, seed=seed)
    for f in data:                                     # N points per cloud: the re-crop samples as many as the frame's cloud holds
        f["points"], f["labels"], f["nocs"] = f["points"][..., :N].contiguous(), f["labels"][..., :N].contiguous(), f["nocs"][..., :N].contiguous()
    return data


def _trainer(device, wseed):
    from captra_amd.configs import make_config
    from captra_amd.synthetic import make_physical_state_dict
    from captra_amd.trainer import Trainer
    cfg = make_config("1", experiment_dir="/tmp/captra_otf_det_test", nocs_otf=True, **{"init_frame/gt": True})
    cfg["device"] = device
    cfg["track_cfg"]["nocs2d_label"] = True
    trainer = Trainer(cfg)
    model = trainer.model
    model.load_state_dict(make_physical_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, wseed, 1, True, "nocs"))
    return trainer


def _run(trainer, data, tseed):
    torch.manual_seed(tseed)
    np.random.seed(tseed)
    pred, _ = trainer.test(data, save=False, no_eval=True)
    model = trainer.model
    T = len(data)
    return ([{k: v.clone() for k, v in p.items()} for p in pred["poses"]], [model.feed_dict[i]["points"].clone() for i in range(1, T)],
            [model.feed_dict[i]["labels"].clone() for i in range(1, T)])


@pytest.mark.parametrize("defer", [False, True])
def test_track_loop_crops_with_the_selected_detections(device, defer, monkeypatch):
    """B = 2, 4 frames, N = 512, nocs2d_label on.  Run A's frames carry detections; run B's carry none, and its pre-fetched mask is, per
    frame, the mask the judge selects under run A's own previous poses (no radius growth, asserted): poses, labels and clouds are equal
    bit for bit -- with the synchronous stage and with the sync-free one.  (Cropping with the ground-truth mask gives other labels.)"""
    import captra_amd.model as M
    from captra_amd.synthetic import OTF_LOOP_SETUPS
    monkeypatch.setattr(M, "OTF_DEFER", defer)
    B, T, N = 2, 4, 512
    _, dseed, wseed, tseed = OTF_LOOP_SETUPS["b"]
    trainer = _trainer(device, wseed)
    data_a = _loop_data(B, T, N, dseed, True)
    poses_a, clouds_a, labels_a = _run(trainer, data_a, tseed)
    assert trainer.model._otf_defer_usable(trainer.model.feed_dict[1]) == defer
    data_b = _loop_data(B, T, N, dseed, False)
    H, W = data_b[0]["meta"]["pre_fetched"]["mask"].shape[1:]
    gt_differs = False
    for i in range(1, T):
        pre = data_a[i]["meta"]["pre_fetched"]
        last = poses_a[i - 1]
        j = det_judge.select_batch(H, W, last["translation"][:, 0].reshape(B, 3).cpu().numpy(), last["scale"][:, 0].reshape(B).cpu().numpy(),
                                   trainer.model.radius, pre["det_boxes"].numpy(), pre["det_class"].numpy(), pre["det_count"].numpy(), 1)
        assert (j["rounds"] == 0).all() and (j["sel"] >= 0).all()
        chosen = torch.stack([pre["det_masks"][b, int(j["sel"][b])].bool() for b in range(B)])
        gt_differs |= not torch.equal(chosen, data_b[i]["meta"]["pre_fetched"]["mask"].bool())
        data_b[i]["meta"]["pre_fetched"]["mask"] = chosen
    assert gt_differs
    poses_b, clouds_b, labels_b = _run(trainer, data_b, tseed)
    for i in range(T):
        for k in poses_a[i]:
            assert torch.equal(poses_a[i][k], poses_b[i][k]), (k, i)
    for i in range(T - 1):
        assert torch.equal(clouds_a[i], clouds_b[i]) and torch.equal(labels_a[i], labels_b[i]), i
        assert 0 < int((labels_a[i] == 0).sum()) < labels_a[i].numel()


def test_flag_without_detections_keeps_the_pre_fetched_mask(device, caplog):
    """nocs2d_label on and no det_* keys in the frames: the bits of the pre-fetched-mask path (the same loop with the flag off feeds
    RotationNet other labels, so the comparand is the re-crop itself: the clouds and labels of frame 1, whose entering pose is the
    ground truth either way), and ONE warning per model object."""
    import logging
    from captra_amd.synthetic import OTF_LOOP_SETUPS
    B, T, N = 2, 3, 512
    _, dseed, wseed, tseed = OTF_LOOP_SETUPS["b"]
    trainer = _trainer(device, wseed)
    with caplog.at_level(logging.WARNING, logger="captra_amd.model"):
        poses, clouds, labels = _run(trainer, _loop_data(B, T, N, dseed, False), tseed)
        poses2, clouds2, labels2 = _run(trainer, _loop_data(B, T, N, dseed, False), tseed)
    assert sum("no detections" in r.getMessage() for r in caplog.records) == 1
    for a, b in zip(clouds + labels, clouds2 + labels2):
        assert torch.equal(a, b)
    trainer.model.track_cfg["nocs2d_label"] = False
    trainer.model.track_cfg["gt_label"] = True            # the same label routing, the flag off: the parent's pre-fetched-mask path
    poses3, clouds3, labels3 = _run(trainer, _loop_data(B, T, N, dseed, False), tseed)
    for i in range(T):
        for k in poses[i]:
            assert torch.equal(poses[i][k], poses3[i][k]), (k, i)
    for a, b in zip(clouds + labels, clouds3 + labels3):
        assert torch.equal(a, b)
