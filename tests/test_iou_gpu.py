"""GPU: box IoUs and predicted NOCS corners of the evaluation on the device (captra_amd/csrc/box_iou.hip: captra_box_iou,
captra_part_extent; pose_utils/bbox_utils.py device counterparts; cfg['eval_device']) against the host numpy protocol.

Occupancy counts on generic pairs are held to the float64 judge of tests/iou_judge.py (no tolerance: bounds from the points within
rounding of a face); axis-aligned pairs, where whole grid planes sit on faces, to the project's IoU tolerance 2e-3; the extent
form to 1e-6 (the G10 tolerance of tests/test_eval_cpu.py); the corners bit for bit."""
import pickle
from pathlib import Path

import numpy as np
import pytest
import torch

from captra_amd.pose_utils import bbox_utils as BU
from tests import clouds
from tests import iou_judge as J
from tests.golden.make_golden_eval import make_inputs
from tests.weights import make_state_dict

pytestmark = pytest.mark.gpu
G = Path(__file__).resolve().parent / "golden"
IOU_TOL, EXTENT_TOL = 2e-3, 1e-6


def _dev(a, device):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device)


def _run(gt, pred, device, nocs=False):
    """gt (J,C,8,3), pred (J,8,3) numpy -> (iou (J,) fp32, counts (J,C,2) or None) numpy."""
    iou, counts = BU.box_iou_device(_dev(gt, device), _dev(pred, device), nocs, return_counts=True)
    return iou.cpu().numpy(), None if counts is None else counts.cpu().numpy()


def _iou_of_counts(inter, union):
    return np.float32(1.0) if union == 0 else np.float32(inter) / np.float32(union)


def test_occupancy_counts_within_the_float64_judge(device):
    pairs = J.generic_pairs()
    iou, counts = _run(np.stack([p[1] for p in pairs])[:, None], np.stack([p[2] for p in pairs]), device)
    assert iou.dtype == np.float32 and counts.dtype == np.int32
    for k, (name, b1, b2) in enumerate(pairs):
        r = J.bounds(b1, b2)
        inter, union = int(counts[k, 0, 0]), int(counts[k, 0, 1])
        print(name, "kernel", inter, union, "decided", r["inter"], r["union"], "A", r["A"], "iou", iou[k], "host", BU.iou_3d(b1, b2))
        assert r["A"] <= J.CAP * r["union64"], (name, r["A"], r["union64"])        # a pair above the cap is a wrong test input
        assert r["inter"] <= inter <= r["inter"] + r["A"], (name, inter, r["inter"], r["A"])
        assert r["union"] <= union <= r["union"] + r["A"], (name, union, r["union"], r["A"])
        assert iou[k] == _iou_of_counts(inter, union), name


def test_axis_aligned_pairs_vs_host(device):
    pairs = J.axis_aligned_pairs()
    iou, _ = _run(np.stack([p[1] for p in pairs])[:, None], np.stack([p[2] for p in pairs]), device)
    for k, (name, b1, b2) in enumerate(pairs):
        host = BU.iou_3d(b1, b2)
        print(name, iou[k], host)
        assert abs(float(iou[k]) - host) <= IOU_TOL, (name, iou[k], host)


def test_extent_form_vs_host_with_symmetric_candidates(device):
    gts, preds = [], []
    for seed in (12, 13, 21, 22):
        gc, pc, gt, pred = make_inputs(seed, 1)
        gb, pb = BU.bbox_from_corners(gc), BU.bbox_from_corners(pc)
        cands = [BU.pose_box({"rotation": np.matmul(gt["rotation"], BU._y_rotation(2 * np.pi * i / 20)), "translation": gt["translation"],
                              "scale": gt["scale"]}, gb)[0] for i in range(20)]
        for box in (BU.pose_box(pred, pb)[0], BU.pose_box(pred, gb)[0]):
            gts.append(np.stack(cands))
            preds.append(box)
    iou, counts = _run(np.stack(gts), np.stack(preds), device, nocs=True)
    assert counts is None
    for k in range(len(preds)):
        host = max(BU.nocs_iou_3d(g, preds[k]) for g in gts[k])
        print(k, iou[k], host)
        assert abs(float(iou[k]) - host) <= EXTENT_TOL, (k, iou[k], host)
    one, _ = _run(np.stack(gts)[:, :1], np.stack(preds), device, nocs=True)
    for k in range(len(preds)):
        assert abs(float(one[k]) - BU.nocs_iou_3d(gts[k][0], preds[k])) <= EXTENT_TOL


def test_iou_properties_through_the_kernel(device):
    """tests/test_eval_cpu.py::test_iou_properties on the device."""
    box = BU.bbox_from_corners(np.array([[-0.2, -0.1, -0.3], [0.2, 0.1, 0.3]], np.float32))
    others = [box, box + np.float32(0.7), box + np.float32(100.0), box + np.array([0.2, 0.0, 0.0], np.float32)]
    iou, counts = _run(np.stack([box] * 4)[:, None], np.stack(others), device)
    assert iou[0] == 1.0 and counts[0, 0, 0] == counts[0, 0, 1] > 0
    assert iou[1] == 0.0 and counts[1, 0, 0] == 0 and counts[1, 0, 1] > 0      # disjoint, still resolved by the 50^3 grid
    assert iou[2] == 1.0 and counts[2, 0, 1] == 0                               # the reference's "both empty" artefact
    assert 0.0 < iou[3] < 1.0
    ext, _ = _run(np.stack([box] * 2)[:, None], np.stack([box, box + np.float32(10.0)]), device, nocs=True)
    assert abs(float(ext[0]) - 1.0) < 1e-6 and ext[1] == 0.0


def test_best_of_candidates_is_pythons_max(device):
    pairs = J.generic_pairs()
    C = 5
    jobs = [(pairs[j][2], [pairs[(j + 7 * c) % len(pairs)][1] for c in range(C)]) for j in range(0, 12)]
    jobs.append((pairs[0][2], [pairs[3][1], pairs[0][1], pairs[0][1], pairs[3][1], pairs[0][1]]))      # a tie: the first one wins
    iou, counts = _run(np.stack([np.stack(c) for _, c in jobs]), np.stack([p for p, _ in jobs]), device)
    single, single_counts = _run(np.stack([np.stack(c) for _, c in jobs]).reshape(-1, 1, 8, 3),
                                 np.repeat(np.stack([p for p, _ in jobs]), C, axis=0), device)
    np.testing.assert_array_equal(counts.reshape(-1, 1, 2), single_counts)         # a pair's counts do not depend on its neighbours
    for j in range(len(jobs)):
        values = [_iou_of_counts(int(a), int(b)) for a, b in counts[j]]
        assert iou[j] == max(values), j
        assert values.index(max(values)) == int(np.argmax(single[j * C:(j + 1) * C])), j
    assert iou[-1] == single[(len(jobs) - 1) * C + 1]


def test_part_extent_bit_exact(device):
    g = torch.Generator().manual_seed(9)
    B, P, N = 5, 4, 4096
    labels = torch.randint(0, P + 1, (B, N), generator=g)                           # label P = background: ignored
    labels[1][labels[1] == 2] = 0                                                   # cloud 1: part 2 is empty
    labels[3][:] = P                                                                # cloud 3: nothing but background
    nocs = (torch.rand(B, N, 3, generator=g) - 0.5)
    nocs[2, 100:200] = nocs[2, :100]                                                # duplicated points
    nocs[0, 7] = torch.tensor([-0.75, 0.0, 0.6])
    labels[0, 7] = 1
    labels[2, :200] = 3
    ref = BU.get_pred_nocs_corners(labels, nocs, P)
    got = BU.pred_nocs_corners_device(labels.to(device), nocs.to(device), P)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, P, 2, 3)
    np.testing.assert_array_equal(got.double().cpu().numpy(), ref)
    assert not ref[1, 2].any() and not ref[3].any() and ref[0, 1, 0, 0] == -0.75
    # a leading frame axis: one launch for a trajectory, and int32 labels as the step's read-out produces them
    both = BU.pred_nocs_corners_device(torch.stack([labels, labels.flip(0)]).int().to(device), torch.stack([nocs, nocs.flip(0)]).to(device), P)
    np.testing.assert_array_equal(both.double().cpu().numpy(), np.stack([ref, ref[::-1]]))


@pytest.mark.parametrize("tag,P,sym,nocs", [("rigid_sym", 1, True, True), ("rigid", 1, False, True), ("arti", 4, False, False)])
def test_g10_through_the_device_path(device, tag, P, sym, nocs):
    """Golden G10 (the reference's own numbers, tests/test_eval_cpu.py::test_part_iou_vs_reference) through
    eval_single_part_iou_device, without and with a leading frame axis."""
    g10 = np.load(G / "g10_eval.npz")
    gc, pc, gt, pred = make_inputs(11 + P + int(sym), P)
    t = lambda d: {k: _dev(v, device).unsqueeze(0) for k, v in d.items()}
    got = BU.eval_single_part_iou_device(_dev(gc, device).unsqueeze(0), _dev(pc, device).unsqueeze(0), t(gt), t(pred), nocs=nocs, sym=sym)
    tol = EXTENT_TOL if nocs else IOU_TOL
    for name in ("npcs_iou", "iou", "gt_bbox_iou"):
        assert tuple(got[name].shape) == (1, P) and got[name].is_cuda
        print(tag, name, got[name].cpu().numpy()[0], g10[f"{tag}_{name}"])
        np.testing.assert_allclose(got[name].cpu().numpy()[0], g10[f"{tag}_{name}"], atol=tol, rtol=0, err_msg=name)
    rep = lambda d: {k: v.unsqueeze(0).repeat((3,) + (1,) * v.dim()) for k, v in d.items()}
    frames = BU.eval_single_part_iou_device(_dev(gc, device).unsqueeze(0), _dev(pc, device)[None, None].repeat(3, 1, 1, 1, 1), rep(t(gt)),
                                            rep(t(pred)), nocs=nocs, sym=sym)
    for name in ("npcs_iou", "iou", "gt_bbox_iou"):
        assert tuple(frames[name].shape) == (3, 1, P)
        np.testing.assert_array_equal(frames[name].cpu().numpy(), np.broadcast_to(got[name].cpu().numpy(), (3, 1, P)))


def _flatten(d, prefix=""):
    out = {}
    for k, v in d.items():
        if isinstance(v, dict):
            out.update(_flatten(v, f"{prefix}{k}/"))
        else:
            out[f"{prefix}{k}"] = v
    return out


def _track(device, cat, objcfg, kind, tag, exp_dir, eval_device):
    from captra_amd.configs import make_config
    from captra_amd.trainer import Trainer
    cfg = make_config(cat, objcfg, experiment_dir=str(exp_dir))
    cfg["device"] = device
    cfg["track_cfg"]["gt_label"] = (tag == "drawers")
    if eval_device is not None:
        cfg["eval_device"] = eval_device
    trainer = Trainer(cfg)
    trainer.model.load_state_dict(make_state_dict({k: tuple(v.shape) for k, v in trainer.model.state_dict().items()}, seed=7))
    data = clouds.make_trajectory(kind, 2, 3, seed=0)
    torch.manual_seed(1234)
    np.random.seed(1234)
    _, loss = trainer.test(data, save=True)
    return trainer, loss


def _same_but_iou(off, on, what):
    """Identical key sets and Python types; IoU entries within 2e-3, every other entry equal."""
    assert list(off) == list(on), what
    for k in off:
        a, b = off[k], on[k]
        assert type(a) is type(b), (what, k, type(a), type(b))
        if torch.is_tensor(a):
            a, b = a.detach().cpu().numpy(), b.detach().cpu().numpy()
        if isinstance(a, np.ndarray):
            assert a.dtype == b.dtype and a.shape == b.shape, (what, k)
        if "iou" in k:
            np.testing.assert_allclose(b, a, atol=IOU_TOL, rtol=0, err_msg=f"{what} {k}")
        else:
            np.testing.assert_array_equal(b, a, err_msg=f"{what} {k}")


@pytest.mark.parametrize("tag,cat,objcfg,kind", [("bottle", "1", "obj_info_nocs.yml", "nocs"), ("drawers", "drawers", "obj_info_sapien.yml", "arti")])
def test_track_and_eval_cli_with_the_key_on_and_off(device, tmp_path, tag, cat, objcfg, kind):
    """`Trainer.test(data, save=True)` on the G13 set-up (tests/test_model_gpu.py::test_track_loss_dict_vs_reference) with
    cfg['eval_device'] off and on: the loss dict and the per-instance records differ in nothing but the IoU values (<= 2e-3), the
    result pickles' pred.corners are the same bits; `captra_amd.eval --eval_device` over those pickles gives the same table."""
    from captra_amd import eval as ev
    t_off, loss_off = _track(device, cat, objcfg, kind, tag, tmp_path / "off", False)
    t_on, loss_on = _track(device, cat, objcfg, kind, tag, tmp_path / "on", True)
    assert not t_off.model.eval_device and t_on.model.eval_device
    flat_off, flat_on = _flatten(loss_off), _flatten(loss_on)
    assert any(k.startswith("avg_iou/") for k in flat_off) and any(k.startswith("frame_iou/") for k in flat_off)
    for k, v in flat_on.items():
        if "iou" in k:
            assert type(v) is float, (k, type(v))
            print(tag, k, flat_off[k], v)
    _same_but_iou(flat_off, flat_on, "loss_dict")
    _same_but_iou(_flatten(t_off.model.per_diff_dict), _flatten(t_on.model.per_diff_dict), "per_diff_dict")
    names = sorted(p.name for p in (tmp_path / "off" / "results" / "data").iterdir())
    assert names and names == sorted(p.name for p in (tmp_path / "on" / "results" / "data").iterdir())
    for name in names:
        recs = []
        for which in ("off", "on"):
            with open(tmp_path / which / "results" / "data" / name, "rb") as f:
                recs.append(pickle.load(f))
        a, b = recs[0]["pred"]["corners"], recs[1]["pred"]["corners"]
        assert a[0] is None and b[0] is None and len(a) == len(b) == 3
        for x, y in zip(a[1:], b[1:]):
            assert type(x) is type(y) and x.dtype == y.dtype == np.float64 and x.shape == y.shape
            np.testing.assert_array_equal(x, y)
    args = ["--obj_category", cat, "--obj_config", objcfg, "--experiment_dir", str(tmp_path / "off")]
    ev.main(args)
    with open(tmp_path / "off" / "results" / "err.pkl", "rb") as f:
        host = pickle.load(f)
    header = (tmp_path / "off" / "results" / "err.csv").read_text().splitlines()[0]
    ev.main(args + ["--eval_device"])
    with open(tmp_path / "off" / "results" / "err.pkl", "rb") as f:
        dev = pickle.load(f)
    assert (tmp_path / "off" / "results" / "err.csv").read_text().splitlines()[0] == header
    assert any(k.startswith("iou_") for k in next(iter(host.values())))
    _same_but_iou(_flatten(host), _flatten(dev), "err.pkl")


def test_default_off_makes_no_call_into_the_new_symbols(device, tmp_path, monkeypatch):
    from captra_amd import _lib
    t_absent, _ = _track(device, "1", "obj_info_nocs.yml", "nocs", "bottle", tmp_path / "absent", None)
    assert "eval_device" not in t_absent.model.cfg
    calls, real = [], _lib.call

    def counting(name, *args):
        calls.append(name)
        return real(name, *args)

    monkeypatch.setattr(_lib, "call", counting)
    new = {"captra_box_iou", "captra_part_extent"}
    t_absent.model.compute_loss(test=True, per_instance=True, eval_iou=True, test_prefix="test")
    t_absent.model._save([["0", "0"]] * 3)
    assert "avg_iou" in t_absent.model.loss_dict and not new & set(calls), calls
    t_absent.model.eval_device = True                                                # the positive control: the same model, key on
    t_absent.model.compute_loss(test=True, per_instance=True, eval_iou=True, test_prefix="test")
    assert calls.count("captra_box_iou") == 1 and calls.count("captra_part_extent") == 1, calls
