"""The judge of captra_image_members (tests/image_fit_judge.py) proven on the CPU: it reproduces the reference's erosion and
back-projection on fixture G17 (tests/golden/g17_image_members.npz: pixels and order identical, points equal as float64 or off by at
most one unit in the last place of the double -- the allowance DESIGN.md section 7 states for the crop), the checks tell every one of
its deliberate mutations apart, the coordinate decode is held on all 256 byte values, and the chain judge -> RANSAC judge recovers the
ground-truth pose of three synthetic scenes."""
from pathlib import Path

import numpy as np
import pytest

from tests import image_fit_judge as IJ

GOLDEN = Path(__file__).resolve().parent / "golden" / "g17_image_members.npz"
_G = {}


def _golden():
    if not _G:
        with np.load(GOLDEN) as z:
            _G.update({k: z[k] for k in z.files})
    return _G


def _within_one_ulp(a, b) -> bool:
    return bool((np.abs(a - b) <= np.spacing(np.abs(b))).all())


def failures(variant=None):
    """Every check of this file that holds the judge to G17 and to the rule, run on the judge with `variant` -> the names of those
    that fail."""
    z = _golden()
    bad = []
    for k in range(int(z["num_cases"])):
        depth, mask, inst, ks = z[f"depth{k}"], z[f"mask{k}"], int(z[f"inst{k}"]), int(z[f"ks{k}"])
        h, w = depth.shape
        own = (mask == inst).astype(np.uint8) * 200
        ref_pix = z[f"rows{k}"] * w + z[f"cols{k}"]
        kinv = IJ.kinv_of(z[f"intrinsics{k}"])
        coord = np.zeros((1, h, w, 3), np.uint8)
        if not np.array_equal(IJ.eroded(own, ks, variant), z[f"eroded{k}"] == inst):
            bad.append(f"erosion {k}")
        got = IJ.members(depth[None], own[None], coord, kinv, 16384, ks, variant=variant)
        n = int(got["counts"][0, 0])
        if n != len(ref_pix) or got["counts"][0, 1] != n or not np.array_equal(got["pix"][0, :n], ref_pix):
            bad.append(f"pixels and order {k}")
        elif not _within_one_ulp(got["tgt64"][0][:, :n].T, z[f"pts{k}"]):
            bad.append(f"points {k}")
        if (got["labels"][0, :n] != 0).any() or (got["labels"][0, n:] != -1).any() or (got["pix"][0, n:] != -1).any() or got["tgt64"][0][:, n:].any():
            bad.append(f"padding {k}")
        holes = int(((z[f"eroded{k}"] == inst) & (depth <= 0)).sum())
        if got["counts"][0, 2] != holes:
            bad.append(f"holes {k}")
        # subsampling, from the rule: the stride is the smallest whose members fit the cap, and the members kept are every stride-th
        for cap in (len(ref_pix) - 1, len(ref_pix) // 3, 5):
            step = -(-len(ref_pix) // cap)
            sub = IJ.members(depth[None], own[None], coord, kinv, cap, ks, variant=variant)
            want = ref_pix[::step]
            if tuple(sub["counts"][0, :2]) != (len(ref_pix), len(want)) or not np.array_equal(sub["pix"][0, :len(want)], want) or (sub["pix"][0, len(want):] != -1).any():
                bad.append(f"subsampling {k} cap {cap}")
    # a batch: every image's result is what the image gives alone (image 0's last rows are the instance over image 1's background rows,
    # and the other way round)
    rng = np.random.default_rng(7)
    depth = rng.integers(500, 900, (3, 12, 16)).astype(np.int32)
    mask = np.zeros((3, 12, 16), np.uint8)
    mask[0, 6:, 2:14], mask[1, 5:, 1:15], mask[2, :7, :] = 1, 1, 1
    mask[1, :3, :] = 0
    coord = rng.integers(0, 256, (3, 12, 16, 3)).astype(np.uint8)
    kinv = IJ.kinv_of(IJ.NOCS_INTRINSICS["real"])
    for border in (1, 2, 3):
        batch = IJ.members(depth, mask, coord, kinv, 64, border, variant=variant)
        for i in range(3):
            alone = IJ.members(depth[i:i + 1], mask[i:i + 1], coord[i:i + 1], kinv, 64, border)
            if not all(np.array_equal(batch[key][i], alone[key][0]) for key in ("pix", "counts", "src", "tgt64", "labels")):
                bad.append(f"image {i} of a batch, border {border}")
    # the decode, through the members' src
    for name in ("image", "table"):
        rgb = np.ascontiguousarray(z[f"coord_bgr_{name}"][:, :, ::-1])              # the loader's reorder: channel k = NOCS axis k
        hh, ww = rgb.shape[:2]
        for negate, key in ((False, f"nocs_{name}"), (True, f"nocs_negz_{name}")):
            got = IJ.members(np.ones((1, hh, ww), np.int32), np.ones((1, hh, ww), np.uint8), rgb[None], kinv, hh * ww, 0, negate, variant=variant)
            if not np.array_equal(got["src"][0, 0].T.reshape(hh, ww, 3), z[key].astype(np.float32)):
                bad.append(f"decode {name} negate_z={negate}")
    return bad


def test_judge_reproduces_g17():
    assert failures() == []


@pytest.mark.parametrize("variant", IJ.MUTATIONS)
def test_checks_catch_the_mutation(variant):
    bad = failures(variant)
    print(variant, "->", bad)
    assert bad, f"the judge with '{variant}' passes every check: the checks cannot tell it from the rule"


def test_decode_all_256_values():
    z = _golden()
    table = z["coord_bgr_table"]
    assert table.shape == (256, 1, 3) and (table[:, 0, 0] == np.arange(256)).all()
    d = IJ.decode(table[:, 0, ::-1])
    np.testing.assert_array_equal(d, z["nocs_table"][:, 0])
    np.testing.assert_array_equal(IJ.decode(table[:, 0, ::-1], True), z["nocs_negz_table"][:, 0])
    v = np.arange(256) / 255.0 - 0.5
    np.testing.assert_array_equal(d[:, 0], v)
    assert d.min() == -0.5 and d.max() == 0.5 and not (d == 0).any()                  # no byte encodes the centre: -0.0 cannot arise
    assert (np.diff(d[:, 0].astype(np.float32)) > 0).all()


def test_tgt_agrees_allows_the_neighbouring_float32_only():
    x = np.array([0.1, -2.5, 1e-3])
    f = x.astype(np.float32)
    assert IJ.tgt_agrees(f, x) and IJ.tgt_agrees(np.nextafter(f, np.float32(9)), x) and IJ.tgt_agrees(np.nextafter(f, np.float32(-9)), x)
    assert not IJ.tgt_agrees(np.nextafter(np.nextafter(f, np.float32(9)), np.float32(9)), x)


# seeds 1, 2, 3 of make_otf_trajectory(1, 1, coord=True), judge chain at the shipped init_frame settings (inlier_th 0.005 x
# data_radius, 64 hypotheses, seed 0), measured on the CPU: rotation / translation / relative scale error against the scene's pose
MEASURED = {1: (0.016743, 0.008498, 3.353e-05), 2: (0.011410, 0.008000, 7.725e-05), 3: (0.011043, 0.010017, 6.114e-05)}
BOUNDS = tuple(2.0 * max(v[k] for v in MEASURED.values()) for k in range(3))            # 0.0335 degrees, 0.0200 mm, 1.545e-4


def test_judge_chain_recovers_the_synthetic_pose():
    """The accuracy anchor.  The errors come from the 8-bit coordinate image (half a step is 0.6 mm at scale 0.31) and millimetre
    depth, averaged over about 14 600 members, every one an inlier.  Measured per seed (rotation degrees, translation mm, relative
    scale): seed 1: 0.016743, 0.008498, 3.353e-05; seed 2: 0.011410, 0.008000, 7.725e-05; seed 3: 0.011043, 0.010017, 6.114e-05.
    Asserted: at most twice the largest measured value of each -- 0.0335 degrees, 0.0200 mm, 1.545e-4; the seeds are fixed, the
    factor covers a later change of num_hyps."""
    from captra_amd import synthetic as S
    from captra_amd.configs import make_config
    from captra_amd.track_options import INIT_FIT_INLIER_TH
    th = INIT_FIT_INLIER_TH * float(make_config("1")["data_radius"])
    kinv = IJ.kinv_of(IJ.NOCS_INTRINSICS["real"])
    for seed in MEASURED:
        frame = S.make_otf_trajectory(1, 1, seed=seed, coord=True)[0]
        pre = frame["meta"]["pre_fetched"]
        mem = IJ.members(pre["depth"].numpy(), pre["mask"].numpy(), pre["coord"].numpy(), kinv, 16384)
        ref, _ = IJ.fit_chain(mem, th)
        assert ref["valid"][0, 0] and ref["num_inliers"][0, 0] == mem["counts"][0, 1] == mem["counts"][0, 0]
        gt = frame["meta"]["nocs2camera"][0]
        err = IJ.pose_errors(ref["rot"][0, 0], ref["scale"][0, 0], ref["trans"][0, 0], gt["rotation"][0].numpy(), gt["scale"][0].numpy(),
                             gt["translation"][0].numpy())
        print(f"seed {seed}: rotation {err[0]:.6f} deg, translation {err[1]:.6f} mm, scale {err[2]:.3e}")
        assert all(e <= b for e, b in zip(err, BOUNDS)), (seed, err, BOUNDS)
