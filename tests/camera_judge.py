"""Float64 numpy restatement of the camera model's four rules (include/captra_hip.h, "The CAMERA MODEL": captra_crop_ball_cam,
captra_crop_ball_det_cam, captra_crop_box_cam, captra_crop_box_det_cam, captra_image_members_cam) with a camera PER ROW:

  * a camera table is (C,19) float64 -- K row-major, K^-1 row-major, depth_unit -- and cam_of (B,) names a row per trajectory;
  * back-projection of trajectory i: ray = Kinv_i (col, h - row, 1); z = float64(float32(d)); p = (ray z / ray_z) unit_i, p_z negated;
  * box projection: nocs_otf.proj_corners_batch's operations with K_i; its 1000.0 is a constant, not a depth unit;
  * the detector route: tests/det_judge.py's selection with K_i; the image members: tests/image_fit_judge.py's rule with Kinv_i, unit_i.

With one camera and unit 0.001 every function here gives, byte for byte, what the existing judges give (tests/test_camera_judge_cpu.py).
`variant` is the same judge with ONE deliberate mistake (MUTATIONS): what the device test's table of checks must be able to tell apart.
`checks()` is that table: the inputs tests/test_camera_gpu.py runs through the *_cam entry points and compares with this judge bit for bit."""
from __future__ import annotations

import numpy as np

from tests import det_judge, image_fit_judge as IJ, otf_inputs as I, otf_judge as J

CAM_ROW = 19
MUTATIONS = ("cam_of_ignored", "unit_before_division", "unit_in_projection", "last_kinv_for_all")
SKEW_K = np.array([[57.0, 0.9, 30.5], [0.0, 63.0, 25.25], [0.0, 0.0, 1.0]])          # fx != fy, a skew term
HALF_UNIT = 0.0005
UNITS_PER_MM = 0.001


def table(cams) -> np.ndarray:
    """[(K (3,3), depth_unit), ...] -> (C,19) float64: K, numpy.linalg.inv(K), unit per row (what nocs_otf.camera_rows builds)."""
    return np.stack([np.concatenate([np.asarray(K, np.float64).reshape(9), np.linalg.inv(np.asarray(K, np.float64)).reshape(9), [np.float64(u)]])
                     for K, u in cams])


def row_of(tab, cam_of, i, variant=None):
    """(K 9, Kinv 9, unit) trajectory i reads under `variant`."""
    tab = np.asarray(tab, np.float64).reshape(-1, CAM_ROW)
    c = 0 if variant == "cam_of_ignored" else int(np.clip(int(cam_of[i]), 0, len(tab) - 1))
    kinv = tab[-1, 9:18] if variant == "last_kinv_for_all" else tab[c, 9:18]
    return tab[c, :9], kinv, np.float64(tab[c, 18])


def backproject_pixels(rows, cols, d, h, kinv, unit, variant=None) -> np.ndarray:
    """Pixels (rows, cols) with depth counts d of an image of height h -> (n,3) float64 metres: ray = (k0 u + k1 v) + k2, .. with u = col,
    v = h - row; z = float64(float32(d)); p = (ray z / ray_z) unit, p_z negated."""
    k = np.asarray(kinv, np.float64).reshape(9)
    u, v = np.asarray(cols).astype(np.float64), (h - np.asarray(rows)).astype(np.float64)
    rx = (k[0] * u + k[1] * v) + k[2]
    ry = (k[3] * u + k[4] * v) + k[5]
    rz = (k[6] * u + k[7] * v) + k[8]
    z = np.asarray(d).astype(np.float32).astype(np.float64)
    unit = np.float64(unit)
    if variant == "unit_before_division":
        return np.stack([rx * z * unit / rz, ry * z * unit / rz, -(rz * z * unit / rz)], 1).reshape(-1, 3)
    return np.stack([(rx * z / rz) * unit, (ry * z / rz) * unit, (-(rz * z / rz)) * unit], 1).reshape(-1, 3)


def crop_ball(depth, mask, box, center, radius, kinv, unit, cap, h, w, variant=None):
    """One instance of captra_crop_ball_cam, otf_judge.crop_ball's outputs: (pts, obj, pix, count, valid)."""
    depth = np.asarray(depth).reshape(h, w)
    r0, c0, r1, c1 = (int(x) for x in np.asarray(box).reshape(4))
    if r1 < r0 or c1 < c0:
        rows = cols = np.zeros(0, np.int64)
    else:
        rr, cc = np.nonzero(depth[r0:r1 + 1, c0:c1 + 1] > 0)                      # row-major
        rows, cols = rr.astype(np.int64) + r0, cc.astype(np.int64) + c0
    pts = backproject_pixels(rows, cols, depth[rows, cols], h, kinv, unit, variant)
    with np.errstate(invalid="ignore"):
        member = J.distances(pts, center) <= np.float64(radius)
    count, valid = int(member.sum()), len(rows)
    keep = np.nonzero(member)[0][:min(count, int(cap))]
    obj = np.asarray(mask).reshape(h, w)[rows[keep], cols[keep]].astype(np.uint8)
    return pts[keep], obj, (rows[keep] * w + cols[keep]).astype(np.int32), count, valid


def ball_batch(case, tab, cam_of, variant=None) -> list:
    """Every instance of a ball case (tests/otf_inputs.py: ball_case) under the cameras: otf_inputs.judge_ball's list."""
    masks = I.masks_of(case)
    out = []
    for b in range(len(case["depth"])):
        _, kinv, unit = row_of(tab, cam_of, b, variant)
        out.append(crop_ball(case["depth"][b], masks[b], case["box"][b], case["center"][b], case["radius"][b], kinv, unit, case["cap"],
                             case["h"], case["w"], variant))
    return out


def project(h, w, centers, radii_in, K, mm=1000.0) -> np.ndarray:
    """nocs_otf.proj_corners_batch, operation by operation, for instances of ONE camera -> (B,4) int32 {row_min, col_min, row_max, col_max};
    mm: the constant the corners are multiplied by (1000.0: part of the reference's arithmetic)."""
    c = np.asarray(centers, np.float64).reshape(-1, 3)
    r = np.maximum(np.asarray(radii_in, np.float64).reshape(-1, 1), 0.05)
    lo, hi = c - r, c + r
    sel = np.array([[x, y, z] for y in (0, 1) for x in (0, 1) for z in (0, 1)])
    box = np.where(sel[None] == 0, lo[:, None, :], hi[:, None, :]) * np.float64(mm)
    homog = -box / box[:, :, 2:3]
    homog[:, :, 2] = -homog[:, :, 2]
    K = np.asarray(K, np.float64).reshape(3, 3)
    u = (K[0, 0] * homog[:, :, 0] + K[0, 1] * homog[:, :, 1]) + K[0, 2] * homog[:, :, 2]
    v = (K[1, 0] * homog[:, :, 0] + K[1, 1] * homog[:, :, 1]) + K[1, 2] * homog[:, :, 2]
    rows, cols = h - v.astype(np.int32), u.astype(np.int32)
    out = np.stack([rows.min(1), cols.min(1), rows.max(1), cols.max(1)], 1).astype(np.int64)
    out[:, :2] = np.maximum(out[:, :2], 0)
    out[:, 2:] = np.minimum(out[:, 2:], np.array([h - 1, w - 1]))
    return out.astype(np.int32)


def crop_box(h, w, trans32, scale32, factor, tab, cam_of, variant=None) -> dict:
    """captra_crop_box_cam from the fp32 pose as the kernel reads it -> box (B,4) int32, center (B,3), radius (B,) float64."""
    c = np.asarray(trans32, np.float32).reshape(-1, 3).astype(np.float64)
    r_in = np.float64(factor) * np.asarray(scale32, np.float32).reshape(-1).astype(np.float64)
    box = np.zeros((len(c), 4), np.int32)
    for i in range(len(c)):
        K, _, unit = row_of(tab, cam_of, i, variant)
        mm = np.float64(1.0) / unit if variant == "unit_in_projection" else 1000.0
        box[i] = project(h, w, c[i:i + 1], r_in[i:i + 1], K, mm)[0]
    with np.errstate(invalid="ignore"):
        return {"box": box, "center": c, "radius": np.where(r_in > 0.05, r_in, 0.05)}


def crop_box_det(h, w, trans32, scale32, factor, det_boxes, det_class, det_count, category, tab, cam_of, variant=None) -> dict:
    """captra_crop_box_det_cam: det_judge.select_batch's outputs with every row's own K."""
    keys = ("box", "center", "radius", "radius_raw", "sel")
    rows = []
    for i in range(len(det_count)):
        K, _, _ = row_of(tab, cam_of, i, variant)
        rows.append(det_judge.select_batch(h, w, np.asarray(trans32)[i:i + 1], np.asarray(scale32)[i:i + 1], factor, det_boxes[i:i + 1],
                                           det_class[i:i + 1], det_count[i:i + 1], category, K.reshape(3, 3)))
    return {k: np.concatenate([r[k] for r in rows]) for k in keys}


def members(depth, mask, coord, tab, cam_of, cap, border=0, negate_z=False, variant=None) -> dict:
    """captra_image_members_cam: image_fit_judge.members' dict with image i back-projected by its own camera."""
    depth = np.asarray(depth)
    b, h, w = depth.shape
    out = IJ.members(depth, mask, coord, np.asarray(tab, np.float64).reshape(-1, CAM_ROW)[0, 9:18], cap, border, negate_z)
    for i in range(b):
        used = int(out["counts"][i, 1])
        rows, cols = out["pix"][i, :used] // w, out["pix"][i, :used] % w
        _, kinv, unit = row_of(tab, cam_of, i, variant)
        out["tgt64"][i] = 0.0
        out["tgt64"][i, :, :used] = backproject_pixels(rows, cols, depth[i][rows, cols], h, kinv, unit, variant).T
    out["tgt"] = out["tgt64"].astype(np.float32)
    return out


# ---- the device test's table of checks ------------------------------------------------------------------------------------------
MIXED_CAMS = [(I.K, UNITS_PER_MM), (I.WIDE_K, UNITS_PER_MM), (SKEW_K, HALF_UNIT)]
MIXED_CAM_OF = np.array([2, 0, 1, 0], np.int32)
MIXED_SEED = 3
THIRD_UNIT = 0.0007              # the unit of knife_edge_poses' camera: 1 / unit is no power-of-two multiple of 1000


def mixed_frames(seed=MIXED_SEED):
    """Four 48 x 64 frames, one per row of the mixed batch: depth (4,H,W) int32 in the COUNTS of the row's camera (row 0's camera counts
    half millimetres: its image holds twice the numbers), mask (4,H,W) uint8."""
    kinds = ("dense", "half", "neg", "dense")
    frames = [I.frame(200 + 10 * seed + b, kinds[b]) for b in range(4)]
    depth = np.stack([f[0] for f in frames]).astype(np.int32)
    depth[0] *= 2
    return depth, np.stack([f[1] for f in frames])


def mixed_ball_case(cap=I.H * I.W, seed=MIXED_SEED):
    """The mixed batch as a ball case: boxes of 64, 1023, 1025 and 3072 pixels, each ball centred on its own camera's back-projection of
    a pixel in the box's middle, radii that cut the boxes (row 3: every pixel)."""
    depth, mask = mixed_frames(seed)
    tab = table(MIXED_CAMS)
    boxes = np.array([(20, 30, 27, 37), (7, 16, 39, 46), (11, 9, 35, 49), (0, 0, I.H - 1, I.W - 1)], np.int32)
    centers, radii = [], [0.05, 0.16, 0.2, I.ALL]
    for b in range(4):
        r, c = (boxes[b, 0] + boxes[b, 2]) // 2, (boxes[b, 1] + boxes[b, 3]) // 2
        _, kinv, unit = row_of(tab, MIXED_CAM_OF, b)
        d = np.abs(depth[b, r, c]) if depth[b, r, c] != 0 else (2000 if b == 0 else 1000)
        centers.append(backproject_pixels([r], [c], [d], I.H, kinv, unit)[0] + np.array([0.003, -0.002, 0.004]))
    return I.ball_case(f"mixed_cap{cap}", depth, mask, boxes, np.stack(centers), radii, cap)


def mixed_box_poses():
    """(trans (4,3) fp32, scale (4,) fp32, factor) on the surfaces the mixed cameras see."""
    case = mixed_ball_case()
    return case["center"].astype(np.float32), np.array([0.17, 0.2, 0.3, 0.12], np.float32), 0.6


KNIFE_K = np.array([[64.0, 0.0, 0.0], [0.0, 64.0, 0.0], [0.0, 0.0, 1.0]])        # a power-of-two focal length, the principal point at 0


def knife_edge_poses(K=KNIFE_K, unit=THIRD_UNIT):
    """fp32 poses (trans (n,3), scale (n,)) at factor 1.0 on the 48 x 64 image whose box differs between the constant 1000.0 and 1 / unit.
    The cube's corners are binary fractions: x - r = j / 64 and z - r = -1, so under 1000.0 every product and quotient is exact and the
    corner projects to column j exactly; under 1 / unit = 1428.57.. the product rounds, and where the quotient comes back one ulp
    below j / 64 the truncation gives column j - 1.  Enumerated, not drawn."""
    out_t, out_s = [], []
    for j in range(1, 64):
        for r in (0.25, 0.125, 0.0625):
            t = np.array([j / 64 + r, 0.1 + r, -1.0 + r], np.float32)
            assert t.astype(np.float64).tolist() == [j / 64 + r, np.float64(np.float32(0.1 + r)), -1.0 + r]
            a = project(I.H, I.W, t.astype(np.float64)[None], [np.float64(r)], K, 1000.0)
            b = project(I.H, I.W, t.astype(np.float64)[None], [np.float64(r)], K, np.float64(1.0) / np.float64(unit))
            if not np.array_equal(a, b):
                out_t.append(t)
                out_s.append(r)
    return np.array(out_t, np.float32).reshape(-1, 3), np.array(out_s, np.float32)


def scaled_kinv_table(factors=(3.0, 1.7, 0.3)):
    """The mixed cameras' table with every K^-1 block multiplied by a factor: projectively the same inverse (p = ray z / ray_z does not
    change), but ray_z is no longer 1, so the division rounds and its place in the operation order shows."""
    tab = table(MIXED_CAMS)
    for c, f in enumerate(factors):
        tab[c, 9:18] *= f
    return tab


def mixed_detections(seed=MIXED_SEED, K=5):
    """Detections of the mixed batch's four rows: boxes around each row's own crop box (hits, growth), a row without the category."""
    rng = np.random.default_rng([seed, 77])
    trans, scale, factor = mixed_box_poses()
    tab = table(MIXED_CAMS)
    own = crop_box(I.H, I.W, trans, scale, factor, tab, MIXED_CAM_OF)["box"]
    y1, x1 = rng.integers(-4, I.H, (4, K)), rng.integers(-4, I.W, (4, K))
    boxes = np.stack([y1, x1, y1 + rng.integers(0, 30, (4, K)), x1 + rng.integers(0, 30, (4, K))], -1).astype(np.int32)
    boxes[:, 1] = own + np.array([1, -2, 3, 2], np.int32)
    boxes[3, 1] = (0, 0, 2, 2)                        # row 3: its category far from the crop: the radius grows
    cls = rng.integers(1, 4, (4, K)).astype(np.int32)
    cls[:, 1] = 1
    cls[2] = 3                                        # a row without the category
    return boxes, cls, np.array([K, K - 1, K, 3], np.int32), 1


def mixed_members_case(seed=MIXED_SEED):
    """Four 24 x 32 images for captra_image_members_cam under the mixed cameras (row 0's depth in half millimetres)."""
    depth, mask, coord = IJ.blob_case(40 + seed, b=4, members_wanted=20)
    depth = depth.copy()
    depth[0] *= 2
    return depth, mask, coord


def checks(variant=None) -> dict:
    """The table: name -> what the judge (under `variant`) says the *_cam entry points produce on the mixed batch.  A mutation is caught
    when at least one entry differs from checks(None)."""
    tab = table(MIXED_CAMS)
    out = {}
    for cap in (I.H * I.W, 100):
        case = mixed_ball_case(cap)
        res = ball_batch(case, tab, MIXED_CAM_OF, variant)
        out[f"ball_cap{cap}"] = {"pts": [r[0] for r in res], "obj": [r[1] for r in res], "pix": [r[2] for r in res],
                                 "counts": np.array([(r[3], r[4]) for r in res], np.int32)}
    trans, scale, factor = mixed_box_poses()
    out["box"] = crop_box(I.H, I.W, trans, scale, factor, tab, MIXED_CAM_OF, variant)
    case = mixed_ball_case()
    res = ball_batch(case, scaled_kinv_table(), MIXED_CAM_OF, variant)
    out["ball_scaled_kinv"] = {"pts": [r[0] for r in res], "obj": [r[1] for r in res], "pix": [r[2] for r in res],
                               "counts": np.array([(r[3], r[4]) for r in res], np.int32)}
    kt, ks = knife_edge_poses()
    out["box_knife_edge"] = crop_box(I.H, I.W, kt, ks, 1.0, table([(KNIFE_K, THIRD_UNIT)]), np.zeros(len(ks), np.int32), variant)
    boxes, cls, count, category = mixed_detections()
    out["box_det"] = crop_box_det(I.H, I.W, trans, scale, factor, boxes, cls, count, category, tab, MIXED_CAM_OF, variant)
    depth, mask, coord = mixed_members_case()
    out["members"] = members(depth, mask, coord, tab, MIXED_CAM_OF, 16, 1, True, variant)
    return out


def same_check(a, b) -> bool:
    """Two entries of checks() agree in every byte."""
    for k in a:
        xs, ys = (a[k], b[k]) if isinstance(a[k], list) else ([a[k]], [b[k]])
        if len(xs) != len(ys) or any(np.asarray(x).shape != np.asarray(y).shape or np.asarray(x).tobytes() != np.asarray(y).tobytes()
                                     for x, y in zip(xs, ys)):
            return False
    return True


# ---- the shifted principal point --------------------------------------------------------------------------------------------------
def padded(depth, mask, q, p):
    """Images (B,h,w) with q zero-depth columns on the left and p rows at the bottom -> (B,h+p,w+q): pixel (r,c) moves to (r,c+q), and
    v = (h + p) - r moves by p."""
    B, h, w = depth.shape
    d2 = np.zeros((B, h + p, w + q), depth.dtype)
    m2 = np.zeros((B, h + p, w + q), mask.dtype)
    d2[:, :h, q:] = depth
    m2[:, :h, q:] = mask
    return d2, m2


def shifted_K(K, q, p):
    K2 = np.array(K, np.float64)
    K2[0, 2] += q
    K2[1, 2] += p
    return K2


def sphere_gap(depth, centers, radii, K, unit) -> float:
    """The smallest | |p - c| - r | over every depth pixel of every image (B,h,w) under one camera."""
    B, h, w = depth.shape
    kinv = np.linalg.inv(np.asarray(K, np.float64)).reshape(9)
    gap = np.inf
    for b in range(B):
        rows, cols = np.nonzero(depth[b] > 0)
        pts = backproject_pixels(rows, cols, depth[b][rows, cols], h, kinv, unit)
        gap = min(gap, float(np.abs(J.distances(pts, centers[b]) - np.float64(radii[b])).min()))
    return gap


SHIFT_Q, SHIFT_P = 5, 3


def shifted_inputs():
    """The shifted-principal-point comparison's inputs: otf_inputs.chain_inputs() (three trajectories on 48 x 64 whose balls hold between
    10 and CHAIN_STRIDE members), the same images padded by SHIFT_Q zero-depth columns on the left and SHIFT_P rows at the bottom, and the
    camera with cx + q, cy + p.  -> dict: plain / shifted = (depth, mask, K), centers (3,3), radii (3,) as captra_crop_box derives them."""
    c = I.chain_inputs()
    d2, m2 = padded(c["depth"], c["mask"], SHIFT_Q, SHIFT_P)
    return {**c, "plain": (c["depth"], c["mask"], I.K), "shifted": (d2, m2, shifted_K(I.K, SHIFT_Q, SHIFT_P)),
            "centers": c["trans"].astype(np.float64), "radii": np.maximum(np.float64(I.CHAIN_FACTOR) * c["scale"].astype(np.float64), 0.05)}
