"""The detector route of the on-the-fly re-crop (`--track_cfg/nocs2d_label True`), CPU side: the float64 judge of the selection
(tests/det_judge.py) against golden G16 -- the reference's own full_data_from_depth_image(mask_from_nocs2d=True), see
tests/golden/make_golden_otf_det.py --, the ABI, and the data side (trajectory files, detector result pickles, synthetic detections)."""
import pickle
from pathlib import Path

import numpy as np
import pytest
import torch

from captra_amd import trajectory_io as tio
from tests import det_judge
from tests.golden.make_golden_otf_det import CASES, CATEGORY, make_case

G16 = np.load(Path(__file__).resolve().parent / "golden" / "g16_otf_det.npz")


@pytest.mark.parametrize("tag", [c[0] for c in CASES])
def test_judge_reproduces_the_reference_selection(tag):
    c = make_case(tag)
    H, W = c["depth"].shape
    sel, radius, corners, rounds = det_judge.select(H, W, c["center"], c["radius"], c["det_boxes"], c["det_class"], len(c["det_class"]), CATEGORY)
    assert sel == int(G16[f"{tag}_sel"])
    assert np.float64(radius).tobytes() == np.float64(G16[f"{tag}_radius"]).tobytes()
    np.testing.assert_array_equal(corners, G16[f"{tag}_corners"])
    assert rounds == int(G16[f"{tag}_rounds"])
    # each case takes the branch it is named for
    assert {"hit": sel == 1 and rounds == 0, "grow": sel == 1 and rounds >= 2 and radius <= 0.5, "giveup": sel == 0 and radius > 0.5,
            "noclass": sel == -1 and rounds == 0, "tie": sel == 1 and rounds == 0}[tag]


def test_judge_ignores_padding_and_ends_on_a_radius_that_cannot_grow():
    c = make_case("hit")
    H, W = c["depth"].shape
    boxes = np.concatenate([c["det_boxes"], c["det_boxes"][:1]])          # a padding slot that would win: the crop's own box, right class
    cls = np.concatenate([c["det_class"], [CATEGORY]]).astype(np.int32)
    assert det_judge.select(H, W, c["center"], c["radius"], boxes, cls, 3, CATEGORY)[0] == 1
    assert det_judge.select(H, W, c["center"], c["radius"], boxes, cls, 4, CATEGORY)[0] == 3
    g = make_case("giveup")
    for bad in (0.0, -1.0, 5e-324):
        sel, radius, _, rounds = det_judge.select(H, W, g["center"], bad, g["det_boxes"], g["det_class"], 2, CATEGORY)
        assert (sel, rounds) == (0, 0) and radius == bad


def test_new_entry_points_in_header_and_binding_table():
    import ctypes
    from captra_amd import _lib
    from tests.test_abi import declared_symbols
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in ("captra_crop_box_det", "captra_crop_ball_det"):
        assert name in declared_symbols() and name in _lib._SIGNATURES and hasattr(lib, name)
    assert len(_lib._SIGNATURES["captra_crop_box_det"]) == 18 and len(_lib._SIGNATURES["captra_crop_ball_det"]) == 18


def test_make_otf_detections_is_deterministic_in_its_seed():
    from captra_amd.synthetic import make_otf_detections
    a, b, c = (make_otf_detections(2, 2, seed=s, num_det=3) for s in (4, 4, 5))
    differs = False
    for fa, fb, fc in zip(a, b, c):
        pa, pb, pc = (f["meta"]["pre_fetched"] for f in (fa, fb, fc))
        for k in tio.DET_KEYS:
            assert torch.equal(pa[k], pb[k])
            differs |= not torch.equal(pa[k], pc[k])
        assert pa["det_boxes"].shape == (2, 3, 4) and pa["det_masks"].shape == (2, 3, 480, 640) and pa["det_masks"].dtype == torch.uint8
        for t in range(2):                            # one detection of the category: the ground-truth mask moved, so it differs from it
            k = int(torch.nonzero(pa["det_class"][t] == 1).reshape(-1)[0])
            assert int((pa["det_class"][t] == 1).sum()) == 1
            assert not torch.equal(pa["det_masks"][t, k].bool(), pa["mask"][t].bool())
            assert (pa["det_masks"][t, k].bool() & pa["mask"][t].bool()).sum() > 0.8 * pa["mask"][t].sum()
    assert differs


def test_trajectory_file_round_trip_of_detections(tmp_path):
    from captra_amd.synthetic import make_otf_detections
    frames = make_otf_detections(2, 2, seed=3, num_det=2)
    paths = []
    for b in range(2):
        paths.append(str(tmp_path / f"t{b}.npz"))
        tio.save_trajectory_npz(paths[-1], frames, b)
    back = tio.stack_trajectories([tio.load_trajectory_npz(p) for p in paths])
    both = tio.concat_frame_batches([tio.stack_trajectories([tio.load_trajectory_npz(p)]) for p in paths])
    for f, g, h in zip(frames, back, both):
        for k in tio.DET_KEYS + ("depth", "mask"):
            assert torch.equal(torch.as_tensor(f["meta"]["pre_fetched"][k]), g["meta"]["pre_fetched"][k].to(f["meta"]["pre_fetched"][k].dtype)), k
            assert torch.equal(g["meta"]["pre_fetched"][k], h["meta"]["pre_fetched"][k]), k
        assert g["meta"]["pre_fetched"]["det_boxes"].dtype == torch.int32 and g["meta"]["pre_fetched"]["det_masks"].dtype == torch.uint8
        assert g["meta"]["ori_path"] == f["meta"]["ori_path"] == h["meta"]["ori_path"]


def test_nocs2d_result_loader_pads_to_k(tmp_path):
    rng = np.random.default_rng(0)
    n, H, W = 3, 12, 16
    res = {"pred_class_ids": np.array([2, 1, 5]), "pred_bboxes": rng.integers(0, 12, (n, 4)), "pred_masks": rng.random((H, W, n)) < 0.5}
    with open(tmp_path / "results_test_scene_7_0003.pkl", "wb") as f:
        pickle.dump(res, f)
    det = tio.load_nocs2d_result(str(tmp_path), "scene_7", "0003", slots=5)
    assert det["det_boxes"].shape == (5, 4) and det["det_boxes"].dtype == np.int32 and int(det["det_count"]) == 3
    np.testing.assert_array_equal(det["det_boxes"][:3], res["pred_bboxes"])
    np.testing.assert_array_equal(det["det_class"], [2, 1, 5, -1, -1])
    np.testing.assert_array_equal(det["det_masks"][:3], np.moveaxis(res["pred_masks"], 2, 0).astype(np.uint8))
    assert not det["det_masks"][3:].any() and det["det_masks"].dtype == np.uint8
    assert tio.load_nocs2d_result(str(tmp_path), "scene_7", "0003")["det_boxes"].shape == (3, 4)
    # through the frames' depth paths, as the reference names the file (scene = the directory, frame = the first four characters)
    frames = [{"meta": {"ori_path": ["x/scene_7/0003_depth.png"] * 2, "pre_fetched": {"depth": torch.zeros(2, H, W), "mask": torch.zeros(2, H, W)}}}]
    pre = tio.attach_nocs2d_detections(frames, str(tmp_path), slots=4)[0]["meta"]["pre_fetched"]
    assert pre["det_masks"].shape == (2, 4, H, W) and pre["det_count"].tolist() == [3, 3] and pre["det_class"].dtype == torch.int32
