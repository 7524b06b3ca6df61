"""The camera model's entry points (captra_crop_ball_cam, captra_crop_ball_det_cam, captra_crop_box_cam, captra_crop_box_det_cam,
captra_image_members_cam; include/captra_hip.h, "The CAMERA MODEL") through the C ABI:

  * identity: every existing ball, box, detector-box and image-member case through the _cam entry point with the table [case K, 0.001]
    gives the plain entry point's bytes, sentinel rows beyond the counts included;
  * the mixed batch (tests/camera_judge.py: checks()): four rows over three cameras, cam_of = [2, 0, 1, 0], against the float64 judge
    BIT FOR BIT -- the table whose checks catch each of the judge's mutations (tests/test_camera_judge_cpu.py);
  * row independence, table order, the exactness of a doubled count under a halved unit, and the refusals.

No tolerance anywhere: the kernels are written operation by operation under -ffp-contract=off."""
import numpy as np
import pytest
import torch

from captra_amd import nocs_otf
from tests import camera_judge as C, image_fit_judge as IJ, otf_inputs as I

pytestmark = pytest.mark.gpu

PTS_SENTINEL, OBJ_SENTINEL, PIX_SENTINEL, CNT_SENTINEL = -7.25e77, 0xEE, -9, -77
BALL_CASES = I.ball_cases()


@pytest.fixture(scope="module", autouse=True)
def _leave_the_allocator_as_found():
    """Set up first, so torn down last: when this module's tensors and models are gone its cached blocks go back to the driver.  Tests
    that run later in the same process (fused.pointwise_mlp2 wants its two sources within 1 GiB of each other) find the caching
    allocator as a run without this module leaves it."""
    yield
    import gc
    gc.collect()
    torch.cuda.empty_cache()


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _cams(device, tab, cam_of):
    return _dev(np.asarray(tab, np.float64).reshape(-1, C.CAM_ROW), device), _dev(np.asarray(cam_of, np.int32), device)


def _crop_ball(device, case, tab=None, cam_of=None, ncam=None, null=()):
    """captra_crop_ball / _det (tab None) or captra_crop_ball_cam / _det_cam on a case -> (err, (pts, obj, pix, counts)) over sentinels."""
    from captra_amd import _lib as L
    B, h, w, cap = len(case["depth"]), case["h"], case["w"], case["cap"]
    depth, mask, box = _dev(case["depth"], device), _dev(case["mask"], device), _dev(case["box"], device)
    ctr, rad, kinv = _dev(case["center"], device), _dev(case["radius"], device), _dev(case["kinv"], device)
    pts = torch.full((B, cap, 3), PTS_SENTINEL, dtype=torch.float64, device=device)
    obj = torch.full((B, cap), OBJ_SENTINEL, dtype=torch.uint8, device=device)
    pix = torch.full((B, cap), PIX_SENTINEL, dtype=torch.int32, device=device)
    counts = torch.full((B, 2), CNT_SENTINEL, dtype=torch.int32, device=device)
    outs = (L.ptr(pts), L.ptr(obj), L.ptr(pix), L.ptr(counts))
    lib = L.lib()
    with torch.cuda.device(device):
        if tab is None:
            cam = (L.ptr(kinv),)
            name = "captra_crop_ball"
        else:
            t_d, c_d = _cams(device, tab, cam_of)
            cam = (len(t_d) if ncam is None else ncam, None if "cams" in null else L.ptr(t_d), None if "cam_of" in null else L.ptr(c_d))
            name = "captra_crop_ball_cam"
        if case["det"] is None:
            err = getattr(lib, name)(B, h, w, cap, L.ptr(depth), L.ptr(mask), L.ptr(box), L.ptr(ctr), L.ptr(rad), *cam, *outs, L.stream_ptr())
        else:
            dm, sel = _dev(case["det"]["masks"], device), _dev(case["det"]["sel"], device)
            name = name.replace("crop_ball", "crop_ball_det")
            err = getattr(lib, name)(B, h, w, cap, case["det"]["ndet"], L.ptr(depth), L.ptr(mask), L.ptr(dm), L.ptr(sel), L.ptr(box), L.ptr(ctr),
                                     L.ptr(rad), *cam, *outs, L.stream_ptr())
    torch.cuda.synchronize(device)
    return err, (pts.cpu().numpy(), obj.cpu().numpy(), pix.cpu().numpy(), counts.cpu().numpy())


def _same_bytes(a, b, tag):
    for x, y, what in zip(a, b, ("pts", "obj", "pix", "counts")):
        assert x.tobytes() == y.tobytes(), (tag, what)


def _assert_ball_equals(got, want, cap, tag):
    """got: the kernel's four arrays; want: the judge's list per instance; rows at and beyond min(count, cap) untouched."""
    pts, obj, pix, counts = got
    for b, (j_pts, j_obj, j_pix, count, valid) in enumerate(want):
        assert (int(counts[b, 0]), int(counts[b, 1])) == (count, valid), (tag, b)
        k = min(count, cap)
        assert len(j_pts) == k
        np.testing.assert_array_equal(pix[b, :k], j_pix, err_msg=str((tag, b)))
        np.testing.assert_array_equal(obj[b, :k], j_obj, err_msg=str((tag, b)))
        assert pts[b, :k].tobytes() == j_pts.tobytes(), (tag, b)
        assert (pts[b, k:] == PTS_SENTINEL).all() and (obj[b, k:] == OBJ_SENTINEL).all() and (pix[b, k:] == PIX_SENTINEL).all(), (tag, b)


def _one_camera(case):
    return C.table([(case["intrinsics"], 0.001)]), np.zeros(len(case["depth"]), np.int32)


# ---- identity -----------------------------------------------------------------------------------------------------------------
def test_identity_ball_and_detector_ball(device):
    """Every case of otf_inputs.ball_cases(), the detector variant included: the _cam call with [case K, 0.001] == the plain call."""
    totals = set()
    for case in BALL_CASES:
        err_p, plain = _crop_ball(device, case)
        err_c, cam = _crop_ball(device, case, *_one_camera(case))
        assert err_p == 0 and err_c == 0, case["name"]
        _same_bytes(cam, plain, case["name"])
        totals |= {int((b[2] - b[0] + 1) * (b[3] - b[1] + 1)) for b in case["box"] if b[2] >= b[0] and b[3] >= b[1]}
    assert totals >= {63, 64, 65, 1023, 1024, 1025, 2049} and any(c["det"] is not None for c in BALL_CASES)


def _crop_box(device, h, w, trans, scale, factor, intrinsics=None, tab=None, cam_of=None, det=None, ncam=None, null=()):
    """captra_crop_box(_det)(_cam) -> (err, dict of host arrays over sentinels); det = (boxes (B,K,4), cls (B,K), count (B,), category)."""
    from captra_amd import _lib as L
    B = len(scale)
    t_d, s_d = _dev(np.asarray(trans, np.float32).reshape(B, 3), device), _dev(np.asarray(scale, np.float32), device)
    out = {"box": torch.full((B, 4), CNT_SENTINEL, dtype=torch.int32, device=device),
           "center": torch.full((B, 3), PTS_SENTINEL, dtype=torch.float64, device=device),
           "radius": torch.full((B,), PTS_SENTINEL, dtype=torch.float64, device=device)}
    lib = L.lib()
    if tab is None:
        kk = nocs_otf._intrinsics_on_device(intrinsics, torch.device(device))
        cam, suffix = (kk.data_ptr(),), ""
    else:
        tab_d, cof_d = _cams(device, tab, cam_of)
        cam = (len(tab_d) if ncam is None else ncam, None if "cams" in null else L.ptr(tab_d), None if "cam_of" in null else L.ptr(cof_d))
        suffix = "_cam"
    with torch.cuda.device(device):
        if det is None:
            err = getattr(lib, "captra_crop_box" + suffix)(B, h, w, float(factor), L.ptr(t_d), L.ptr(s_d), *cam, L.ptr(out["box"]), L.ptr(out["center"]),
                                                           L.ptr(out["radius"]), L.stream_ptr())
        else:
            boxes, cls, count, category = det
            out["radius_raw"] = torch.full((B,), PTS_SENTINEL, dtype=torch.float64, device=device)
            out["sel"] = torch.full((B,), CNT_SENTINEL, dtype=torch.int32, device=device)
            d = [_dev(np.asarray(x, np.int32), device) for x in (boxes, cls, count)]
            err = getattr(lib, "captra_crop_box_det" + suffix)(B, h, w, cls.shape[1], int(category), float(factor), L.ptr(t_d), L.ptr(s_d), *cam,
                                                               *map(L.ptr, d), L.ptr(out["box"]), L.ptr(out["center"]), L.ptr(out["radius"]),
                                                               L.ptr(out["radius_raw"]), L.ptr(out["sel"]), L.stream_ptr())
    torch.cuda.synchronize(device)
    return err, {k: v.cpu().numpy() for k, v in out.items()}


def _same_dict(a, b, tag):
    assert a.keys() == b.keys()
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (tag, k)


def test_identity_box(device):
    """otf_inputs.box_poses on both image sizes and the poses of a lost track: captra_crop_box_cam with [K, 0.001] == captra_crop_box."""
    for h, w, K in ((I.H, I.W, I.K), (480, 640, nocs_otf.NOCS_REAL_INTRINSICS)):
        for n, (trans, scale, factor) in enumerate(I.box_poses(h, w) + [I.lost_poses()]):
            err_p, plain = _crop_box(device, h, w, trans, scale, factor, K)
            err_c, cam = _crop_box(device, h, w, trans, scale, factor, tab=C.table([(K, 0.001)]), cam_of=np.zeros(len(scale), np.int32))
            assert err_p == 0 and err_c == 0
            _same_dict(cam, plain, (h, w, n))


def _random_detections(B, K, rep, H=48, W=64):
    """The seeded boxes of tests/test_otf_det_gpu.py's random case."""
    rng = np.random.default_rng([B, K, rep])
    trans = np.stack([rng.uniform(-0.3, 0.3, B), rng.uniform(-0.25, 0.25, B), rng.uniform(-1.6, -0.9, B)], 1).astype(np.float32)
    scale = rng.choice([0.02, 0.1, 0.2, 0.5, 0.8], B).astype(np.float32)
    y1, x1 = rng.integers(-4, H, (B, K)), rng.integers(-4, W, (B, K))
    boxes = np.stack([y1, x1, y1 + rng.integers(0, 30, (B, K)), x1 + rng.integers(0, 30, (B, K))], -1).astype(np.int32)
    if K > 2:
        boxes[:, K // 2] = boxes[:, 0]
    cls = rng.integers(1, 4, (B, K)).astype(np.int32)
    cls[:, K // 2] = cls[:, 0]
    count = rng.integers(0, K + 1, B).astype(np.int32)
    count[0] = K if rep % 2 == 0 else count[0]
    if B > 1:
        cls[1] = 3
    for b in range(B):
        boxes[b, count[b]:] = (0, 0, H - 1, W - 1)
        cls[b, count[b]:] = 1
    return trans, scale, boxes, cls, count


def test_identity_detector_box(device):
    """The detector route's existing cases -- the golden batch (G16's five) and the seeded random boxes at every (B, K) of
    tests/test_otf_det_gpu.py -- through captra_crop_box_det_cam with [K, 0.001] == captra_crop_box_det."""
    from tests.golden.make_golden_otf_det import CASES, CATEGORY, RADIUS_FACTOR, make_case
    cases = [make_case(c[0]) for c in CASES]
    B, K = len(cases), 4
    H, W = cases[0]["depth"].shape
    boxes, cls, count = np.zeros((B, K, 4), np.int32), np.full((B, K), CATEGORY, np.int32), np.zeros(B, np.int32)
    for b, c in enumerate(cases):
        n = len(c["det_class"])
        boxes[b] = nocs_otf.proj_corners(H, W, c["center"], c["radius"]).reshape(-1)
        boxes[b, :n], cls[b, :n], count[b] = c["det_boxes"], c["det_class"], n
    trans, scale = np.stack([c["trans32"] for c in cases]), np.array([c["scale32"] for c in cases], np.float32)
    runs = [(H, W, nocs_otf.NOCS_REAL_INTRINSICS, trans, scale, RADIUS_FACTOR, (boxes, cls, count, CATEGORY))]
    intr = nocs_otf.NOCS_REAL_INTRINSICS * np.array([[0.1], [0.1], [1.0]])
    for B, K in ((1, 1), (5, 3), (5, 64), (1, 65), (5, 65)):
        for rep in range(4):
            t, s, bx, cl, cn = _random_detections(B, K, rep)
            runs.append((48, 64, intr, t, s, 0.6, (bx, cl, cn, 1)))
    grew = False
    for n, (h, w, Km, t, s, factor, det) in enumerate(runs):
        err_p, plain = _crop_box(device, h, w, t, s, factor, Km, det=det)
        err_c, cam = _crop_box(device, h, w, t, s, factor, tab=C.table([(Km, 0.001)]), cam_of=np.zeros(len(s), np.int32), det=det)
        assert err_p == 0 and err_c == 0
        _same_dict(cam, plain, n)
        grew |= bool((plain["radius_raw"] > np.float64(factor) * s.astype(np.float64)).any())
    assert grew


def _members(device, depth, mask, coord, cap, border, negate_z, kinv=None, tab=None, cam_of=None, ncam=None, null=(), split=0):
    """captra_image_members (kinv) or captra_image_members_cam (tab, cam_of) on poisoned outputs -> (err, dict)."""
    import ctypes
    from captra_amd import _lib as L
    b, h, w = depth.shape
    t = {"depth": _dev(np.asarray(depth, np.int32), device), "mask": _dev(np.asarray(mask, np.uint8), device), "coord": _dev(np.asarray(coord, np.uint8), device),
         "src": torch.full((b, 1, 3, cap), 123.5, dtype=torch.float32, device=device), "tgt": torch.full((b, 3, cap), 123.5, dtype=torch.float32, device=device),
         "labels": torch.full((b, cap), -77, dtype=torch.int32, device=device), "pix": torch.full((b, cap), -77, dtype=torch.int32, device=device),
         "counts": torch.full((b, 3), -77, dtype=torch.int32, device=device)}
    outs = [L.ptr(t[k]) for k in ("src", "tgt", "labels", "pix", "counts")]
    lib = L.lib()
    lib.captra_image_members_set_split(ctypes.c_int(split))
    try:
        with torch.cuda.device(device):
            if tab is None:
                k_d = _dev(np.asarray(kinv, np.float64).reshape(9), device)
                err = lib.captra_image_members(b, h, w, cap, border, int(negate_z), L.ptr(t["depth"]), L.ptr(t["mask"]), L.ptr(t["coord"]), L.ptr(k_d),
                                               *outs, L.stream_ptr())
            else:
                tab_d, cof_d = _cams(device, tab, cam_of)
                err = lib.captra_image_members_cam(b, h, w, cap, border, int(negate_z), L.ptr(t["depth"]), L.ptr(t["mask"]), L.ptr(t["coord"]),
                                                   len(tab_d) if ncam is None else ncam, None if "cams" in null else L.ptr(tab_d),
                                                   None if "cam_of" in null else L.ptr(cof_d), *outs, L.stream_ptr())
        torch.cuda.synchronize(device)
    finally:
        lib.captra_image_members_set_split(ctypes.c_int(0))
    return err, {k: t[k].cpu().numpy() for k in ("src", "tgt", "labels", "pix", "counts")}


NONSQUARE = np.array([[31.0, 0.7, 15.25], [0.0, 23.5, 12.75], [0.0, 0.0, 1.0]])


def _member_cases():
    """The inputs of tests/test_image_fit_gpu.py: the border x cap grid of blob cases, the edge images, the thin images, the full frame."""
    out = []
    for border in (0, 1, 2, 3):
        for cap in (1, 7, 64):
            for n, want in enumerate((cap, cap + 1, 2 * cap + 1)):
                K = (IJ.NOCS_INTRINSICS["real"], IJ.NOCS_INTRINSICS["camera"], NONSQUARE)[n]
                out.append((f"blob b{border} c{cap} m{want}", *IJ.blob_case(100 * border + cap + n, members_wanted=want, border=border), K, cap, border, n & 1))
        h, w = 24, 32
        rng = np.random.default_rng(border)
        depth = rng.integers(400, 3000, (6, h, w)).astype(np.int32)
        coord = rng.integers(0, 256, (6, h, w, 3)).astype(np.uint8)
        mask = np.zeros((6, h, w), np.uint8)
        mask[1, 4:20, 5:25] = 255
        depth[1] = 0
        mask[2] = 1
        mask[3, h - 6:, :] = 9
        mask[4, 6:, 3:w - 3] = 200
        mask[5, :6, :] = 7
        mask[5, :6, w - 1] = 0
        out.append((f"edges b{border}", depth, mask, coord, NONSQUARE, 64, border, 1))
    for h, w in ((1, 37), (29, 1), (1, 1), (5, 3)):
        for border in (0, 1, 3):
            rng = np.random.default_rng(h * 100 + w + border)
            depth = rng.integers(-1, 2000, (3, h, w)).astype(np.int32)
            mask = (rng.random((3, h, w)) < 0.8).astype(np.uint8) * 3
            out.append((f"thin {h}x{w} b{border}", depth, mask, rng.integers(0, 256, (3, h, w, 3)).astype(np.uint8), IJ.NOCS_INTRINSICS["real"], 7, border, 0))
    rng = np.random.default_rng(5)
    h, w = 480, 640
    r, c = np.mgrid[0:h, 0:w]
    depth = (900 + 0.3 * r + 0.2 * c + rng.integers(0, 5, (2, h, w))).astype(np.int32)
    depth[rng.random((2, h, w)) < 0.02] = 0
    mask = np.stack([(r - 230) ** 2 + (c - 330) ** 2 < 90 ** 2, (abs(r - 200) < 110) & (abs(c - 300) < 100)]).astype(np.uint8)
    mask[rng.random((2, h, w)) < 0.01] = 0
    out.append(("480x640", depth, mask, rng.integers(0, 256, (2, h, w, 3)).astype(np.uint8), IJ.NOCS_INTRINSICS["real"], 16384, 1, 0))
    return out


def test_identity_image_members(device):
    """Every input of tests/test_image_fit_gpu.py: captra_image_members_cam with [K, 0.001] == captra_image_members, padding slots included,
    with the launcher's geometry and with five workgroups per image."""
    for name, depth, mask, coord, K, cap, border, negate_z in _member_cases():
        kinv = IJ.kinv_of(K)
        tab = C.table([(K, 0.001)])
        assert tab[0, 9:18].tobytes() == kinv.tobytes()
        for split in (0, 5):
            err_p, plain = _members(device, depth, mask, coord, cap, border, negate_z, kinv=kinv, split=split)
            err_c, cam = _members(device, depth, mask, coord, cap, border, negate_z, tab=tab, cam_of=np.zeros(len(depth), np.int32), split=split)
            assert err_p == 0 and err_c == 0, name
            _same_dict(cam, plain, (name, split))


# ---- the mixed batch: the table of checks -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def want():
    return C.checks()


def test_mixed_ball_equals_judge(device, want):
    """Four rows over three cameras (otf_inputs.K, WIDE_K, a skewed one counting half millimetres), cam_of = [2, 0, 1, 0], boxes of 64,
    1023, 1025 and 3072 pixels: pix, obj, counts and the float64 pts bytes == the judge, with a table that holds every member and with
    cap = 100 below the member count of rows; and with every K^-1 of the table scaled (ray_z != 1: the division rounds)."""
    tab = C.table(C.MIXED_CAMS)
    for cap in (I.H * I.W, 100):
        case = C.mixed_ball_case(cap)
        err, got = _crop_ball(device, case, tab, C.MIXED_CAM_OF)
        assert err == 0
        w = want[f"ball_cap{cap}"]
        _assert_ball_equals(got, list(zip(w["pts"], w["obj"], w["pix"], w["counts"][:, 0].tolist(), w["counts"][:, 1].tolist())), cap, cap)
    assert (want["ball_cap100"]["counts"][:, 0] > 100).any() and (want["ball_cap100"]["counts"][:, 0] < 100).any()
    case = C.mixed_ball_case()
    err, got = _crop_ball(device, case, C.scaled_kinv_table(), C.MIXED_CAM_OF)
    assert err == 0
    w = want["ball_scaled_kinv"]
    _assert_ball_equals(got, list(zip(w["pts"], w["obj"], w["pix"], w["counts"][:, 0].tolist(), w["counts"][:, 1].tolist())), case["cap"], "scaled")


def test_mixed_box_and_detector_box_equal_judge(device, want):
    """captra_crop_box_cam and captra_crop_box_det_cam on the mixed batch's poses; and the knife-edge poses whose corner projects to a
    column boundary exactly under the constant 1000.0 (and one column lower under 1 / depth_unit)."""
    tab = C.table(C.MIXED_CAMS)
    trans, scale, factor = C.mixed_box_poses()
    err, got = _crop_box(device, I.H, I.W, trans, scale, factor, tab=tab, cam_of=C.MIXED_CAM_OF)
    assert err == 0
    _same_dict(got, want["box"], "box")
    kt, ks = C.knife_edge_poses()
    err, got = _crop_box(device, I.H, I.W, kt, ks, 1.0, tab=C.table([(C.KNIFE_K, C.THIRD_UNIT)]), cam_of=np.zeros(len(ks), np.int32))
    assert err == 0 and len(ks) > 0
    _same_dict(got, want["box_knife_edge"], "knife edge")
    boxes, cls, count, category = C.mixed_detections()
    err, got = _crop_box(device, I.H, I.W, trans, scale, factor, tab=tab, cam_of=C.MIXED_CAM_OF, det=(boxes, cls, count, category))
    assert err == 0
    _same_dict(got, {k: np.asarray(v, got[k].dtype) for k, v in want["box_det"].items()}, "box_det")
    assert (want["box_det"]["sel"] >= 0).any() and (want["box_det"]["sel"] < 0).any()


def test_mixed_image_members_equal_judge(device, want):
    """captra_image_members_cam on four images under the mixed cameras: pix, labels, counts and src bit for bit, tgt as the plain kernel is
    held to its judge (tests/image_fit_judge.py: tgt_agrees)."""
    depth, mask, coord = C.mixed_members_case()
    err, got = _members(device, depth, mask, coord, 16, 1, True, tab=C.table(C.MIXED_CAMS), cam_of=C.MIXED_CAM_OF)
    assert err == 0
    w = want["members"]
    for k in ("counts", "pix", "labels", "src"):
        np.testing.assert_array_equal(got[k], w[k], err_msg=k)
    assert IJ.tgt_agrees(got["tgt"], w["tgt64"])
    assert (w["counts"][:, 0] > 16).any()


# ---- row independence, table order, the depth unit ------------------------------------------------------------------------------
def _row(case, b):
    return {**case, "depth": case["depth"][b:b + 1], "mask": case["mask"][b:b + 1], "box": case["box"][b:b + 1], "center": case["center"][b:b + 1],
            "radius": case["radius"][b:b + 1]}


def test_row_independence_and_table_order(device):
    """Each row of the mixed batch == a B = 1, ncam = 1 launch of that row; permuting the table's rows and remapping cam_of changes no byte."""
    tab = C.table(C.MIXED_CAMS)
    case = C.mixed_ball_case(100)
    _, whole = _crop_ball(device, case, tab, C.MIXED_CAM_OF)
    trans, scale, factor = C.mixed_box_poses()
    _, whole_box = _crop_box(device, I.H, I.W, trans, scale, factor, tab=tab, cam_of=C.MIXED_CAM_OF)
    depth, mask, coord = C.mixed_members_case()
    _, whole_mem = _members(device, depth, mask, coord, 16, 1, True, tab=tab, cam_of=C.MIXED_CAM_OF)
    for b in range(4):
        one = tab[C.MIXED_CAM_OF[b]][None]
        err, alone = _crop_ball(device, _row(case, b), one, [0])
        assert err == 0
        _same_bytes(alone, tuple(x[b:b + 1] for x in whole), ("ball", b))
        err, alone = _crop_box(device, I.H, I.W, trans[b:b + 1], scale[b:b + 1], factor, tab=one, cam_of=[0])
        _same_dict(alone, {k: v[b:b + 1] for k, v in whole_box.items()}, ("box", b))
        err, alone = _members(device, depth[b:b + 1], mask[b:b + 1], coord[b:b + 1], 16, 1, True, tab=one, cam_of=[0])
        _same_dict(alone, {k: v[b:b + 1] for k, v in whole_mem.items()}, ("members", b))
    perm = np.array([1, 2, 0])                                  # new row j holds old row perm[j]
    remap = np.argsort(perm).astype(np.int32)[C.MIXED_CAM_OF]
    _, moved = _crop_ball(device, case, tab[perm], remap)
    _same_bytes(moved, whole, "table order: ball")
    _, moved = _crop_box(device, I.H, I.W, trans, scale, factor, tab=tab[perm], cam_of=remap)
    _same_dict(moved, whole_box, "table order: box")
    _, moved = _members(device, depth, mask, coord, 16, 1, True, tab=tab[perm], cam_of=remap)
    _same_dict(moved, whole_mem, "table order: members")


def test_out_of_range_camera_index_is_clamped(device):
    """cam_of outside [0, ncam): the nearest row of the table (memory safety; the host wrapper never builds one)."""
    tab = C.table(C.MIXED_CAMS)
    case = C.mixed_ball_case(100)
    _, want_ = _crop_ball(device, case, tab, [0, 2, 2, 0])
    err, got = _crop_ball(device, case, tab, [-5, 3, 2 ** 31 - 1, -2 ** 31])
    assert err == 0
    _same_bytes(got, want_, "clamped")


def test_depth_unit_exactness(device):
    """Depth counts doubled with the unit halved: pts, tgt and every other output byte-equal to the plain case (both scalings are by a
    power of two, exact in float64)."""
    half = lambda K: C.table([(K, 0.0005)])
    for case in [c for c in BALL_CASES if c["name"] in ("cut_33x31", "cut_3x683", "neg_48x64", "three_cap100", "det")]:
        _, plain = _crop_ball(device, case)
        err, cam = _crop_ball(device, {**case, "depth": case["depth"] * 2}, half(case["intrinsics"]), np.zeros(len(case["depth"]), np.int32))
        assert err == 0
        _same_bytes(cam, plain, case["name"])
    for name, depth, mask, coord, K, cap, border, negate_z in _member_cases()[:9]:
        _, plain = _members(device, depth, mask, coord, cap, border, negate_z, kinv=IJ.kinv_of(K))
        err, cam = _members(device, depth * 2, mask, coord, cap, border, negate_z, tab=half(K), cam_of=np.zeros(len(depth), np.int32))
        assert err == 0
        _same_dict(cam, plain, name)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(device):
    """ncam = 0 and a NULL table or index: -1, no launch, not a byte written -- in all five entry points."""
    tab = C.table(C.MIXED_CAMS)
    trans, scale, factor = C.mixed_box_poses()
    det = C.mixed_detections()
    depth, mask, coord = C.mixed_members_case()
    det_case = next(c for c in BALL_CASES if c["det"] is not None)
    for kw in (dict(ncam=0), dict(ncam=-1), dict(null=("cams",)), dict(null=("cam_of",))):
        for case, cam_of in ((C.mixed_ball_case(100), C.MIXED_CAM_OF), (det_case, np.zeros(len(det_case["depth"]), np.int32))):
            err, (pts, obj, pix, counts) = _crop_ball(device, case, tab, cam_of, **kw)
            assert err == -1, kw
            assert (pts == PTS_SENTINEL).all() and (obj == OBJ_SENTINEL).all() and (pix == PIX_SENTINEL).all() and (counts == CNT_SENTINEL).all(), kw
        for d in (None, det):
            err, out = _crop_box(device, I.H, I.W, trans, scale, factor, tab=tab, cam_of=C.MIXED_CAM_OF, det=d, **kw)
            assert err == -1, kw
            assert (out["box"] == CNT_SENTINEL).all() and (out["center"] == PTS_SENTINEL).all() and (out["radius"] == PTS_SENTINEL).all(), kw
            if d is not None:
                assert (out["radius_raw"] == PTS_SENTINEL).all() and (out["sel"] == CNT_SENTINEL).all(), kw
        err, out = _members(device, depth, mask, coord, 16, 1, True, tab=tab, cam_of=C.MIXED_CAM_OF, **kw)
        assert err == -1, kw
        assert (out["src"] == 123.5).all() and (out["tgt"] == 123.5).all() and (out["labels"] == -77).all() and (out["pix"] == -77).all(), kw
        assert (out["counts"] == -77).all(), kw
