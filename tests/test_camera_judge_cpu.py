"""tests/camera_judge.py pinned on the CPU: with ONE camera and unit 0.001 it reproduces, byte for byte, what the existing judges give on
their own cases (otf_inputs.judge_ball, the box cases, det_judge, image_fit_judge); each of its mutations is caught by at least one
check of the device test's table (camera_judge.checks(), which tests/test_camera_gpu.py compares with the kernels bit for bit); the
host helper nocs_otf.camera_rows builds the judge's table; the doubled-count / halved-unit identity is exact; and the shifted
principal point's inputs keep every pixel away from its sphere."""
import numpy as np
import pytest

from captra_amd import nocs_otf
from tests import camera_judge as C, det_judge, image_fit_judge as IJ, otf_inputs as I


def _one(K, n):
    return C.table([(K, 0.001)]), np.zeros(n, np.int32)


def test_one_camera_reproduces_judge_ball():
    for case in I.ball_cases():
        got = C.ball_batch(case, *_one(case["intrinsics"], len(case["depth"])))
        for b, (g, w) in enumerate(zip(got, I.judge_ball(case))):
            assert g[3:] == w[3:], (case["name"], b)
            for x, y in zip(g[:3], w[:3]):
                assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), (case["name"], b)


@pytest.mark.parametrize("h,w,K", [(I.H, I.W, I.K), (480, 640, nocs_otf.NOCS_REAL_INTRINSICS)], ids=["48x64", "480x640"])
def test_one_camera_reproduces_the_box_cases(h, w, K):
    for trans, scale, factor in I.box_poses(h, w):
        got = C.crop_box(h, w, trans, scale, factor, *_one(K, len(scale)))
        c64, r_in = trans.astype(np.float64), np.float64(factor) * scale.astype(np.float64)
        want = nocs_otf.proj_corners_batch(h, w, c64, r_in, K).reshape(-1, 4)
        np.testing.assert_array_equal(got["box"], want)
        assert got["center"].tobytes() == c64.tobytes() and got["radius"].tobytes() == np.maximum(r_in, 0.05).tobytes()


def test_one_camera_reproduces_det_judge():
    boxes, cls, count, category = C.mixed_detections()
    trans, scale, factor = C.mixed_box_poses()
    for K in (I.K, C.SKEW_K):
        got = C.crop_box_det(I.H, I.W, trans, scale, factor, boxes, cls, count, category, *_one(K, 4))
        want = det_judge.select_batch(I.H, I.W, trans, scale, factor, boxes, cls, count, category, K)
        for k in got:
            assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), k


@pytest.mark.parametrize("border,cap", [(0, 7), (1, 16), (3, 64)])
def test_one_camera_reproduces_image_fit_judge(border, cap):
    for n, K in enumerate((IJ.NOCS_INTRINSICS["real"], IJ.NOCS_INTRINSICS["camera"], C.SKEW_K)):
        depth, mask, coord = IJ.blob_case(100 * border + cap + n, members_wanted=cap + n, border=border)
        got = C.members(depth, mask, coord, *_one(K, len(depth)), cap, border, bool(n & 1))
        want = IJ.members(depth, mask, coord, IJ.kinv_of(K), cap, border, bool(n & 1))
        assert IJ.same(got, want) and got["tgt"].tobytes() == want["tgt"].tobytes()


def test_every_mutation_is_caught_by_the_device_tests_table():
    base = C.checks()
    assert all(C.same_check(base[k], v) for k, v in C.checks().items())           # the table is a pure function
    for m in C.MUTATIONS:
        mutant = C.checks(m)
        caught = [k for k in base if not C.same_check(base[k], mutant[k])]
        assert caught, m
    kt, ks = C.knife_edge_poses()
    assert len(ks) > 0 and (I.plane_gap(kt, ks, 1.0) >= 1e-3).all() and I.projected_extent(kt, ks, 1.0, C.KNIFE_K) < 2.0 ** 30


def test_mixed_batch_has_no_pixel_on_its_sphere():
    """The bit-for-bit membership comparison needs no pixel within rounding of its sphere (otf_judge.boundary_pixels' 4 ulp)."""
    from tests import otf_judge as J
    for tab in (C.table(C.MIXED_CAMS), C.scaled_kinv_table()):
        case = C.mixed_ball_case()
        for b in range(4):
            _, kinv, unit = C.row_of(tab, C.MIXED_CAM_OF, b)
            rows, cols = np.nonzero(case["depth"][b] > 0)
            pts = C.backproject_pixels(rows, cols, case["depth"][b][rows, cols], I.H, kinv, unit)
            rad = case["radius"][b]
            assert (np.abs(J.distances(pts, case["center"][b]) - rad) > 4 * np.spacing(rad)).all(), b


def test_camera_rows_builds_the_judges_table():
    K = np.stack([C.MIXED_CAMS[c][0] for c in C.MIXED_CAM_OF])
    unit = np.array([C.MIXED_CAMS[c][1] for c in C.MIXED_CAM_OF])
    tab, cam_of = nocs_otf.camera_rows(K, unit)
    assert tab.shape == (3, nocs_otf.CAM_ROW) and cam_of.dtype == np.int32 and cam_of.tolist() == [0, 1, 2, 1]        # first appearance
    want = C.table(C.MIXED_CAMS)
    for b in range(4):
        assert tab[cam_of[b]].tobytes() == want[C.MIXED_CAM_OF[b]].tobytes(), b


def test_doubled_counts_under_a_halved_unit_are_exact():
    """p = (ray z / ray_z) unit with z doubled and unit halved: two power-of-two scalings, so the float64 result keeps its bytes -- over
    100 000 random pixels of the NOCS REAL camera, and with a ray_z that is not 1."""
    rng = np.random.default_rng(0)
    rows, cols = rng.integers(0, 480, 100000), rng.integers(0, 640, 100000)
    d = rng.integers(1, 30000, 100000)
    for kinv in (IJ.kinv_of(nocs_otf.NOCS_REAL_INTRINSICS), 1.7 * IJ.kinv_of(nocs_otf.NOCS_REAL_INTRINSICS)):
        a = C.backproject_pixels(rows, cols, d, 480, kinv, 0.001)
        b = C.backproject_pixels(rows, cols, 2 * d, 480, kinv, 0.0005)
        assert a.tobytes() == b.tobytes()
    assert np.float64(0.0005) * 2 == np.float64(0.001)


def test_shifted_principal_point_inputs_stay_off_their_spheres():
    """The condition of the shifted-principal-point comparison (tests/test_camera_loop_gpu.py): no pixel of either image within 1e-9 m of
    its sphere, so that a float64 rounding cannot move a pixel across it; and the judge itself agrees to 1e-12 m on the two images."""
    s = C.shifted_inputs()
    for key in ("plain", "shifted"):
        depth, _, K = s[key]
        assert C.sphere_gap(depth, s["centers"], s["radii"], K, 0.001) > 1e-9, key
    (d1, m1, K1), (d2, m2, K2) = s["plain"], s["shifted"]
    for b in range(3):
        box1 = C.project(I.H, I.W, s["centers"][b:b + 1], s["radii"][b:b + 1], K1)[0]
        box2 = C.project(I.H + C.SHIFT_P, I.W + C.SHIFT_Q, s["centers"][b:b + 1], s["radii"][b:b + 1], K2)[0]
        a = C.crop_ball(d1[b], m1[b], box1, s["centers"][b], s["radii"][b], np.linalg.inv(K1).reshape(9), 0.001, 10 ** 6, I.H, I.W)
        c = C.crop_ball(d2[b], m2[b], box2, s["centers"][b], s["radii"][b], np.linalg.inv(K2).reshape(9), 0.001, 10 ** 6, I.H + C.SHIFT_P, I.W + C.SHIFT_Q)
        assert a[3] == c[3] >= 10
        np.testing.assert_array_equal((a[2] // I.W) * (I.W + C.SHIFT_Q) + a[2] % I.W + C.SHIFT_Q, c[2])
        np.testing.assert_array_equal(a[1], c[1])
        assert np.abs(a[0] - c[0]).max() <= 1e-12
