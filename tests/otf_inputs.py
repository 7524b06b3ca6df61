"""Seeded inputs of the re-crop kernels' direct tests: shared by tests/test_otf_kernels_gpu.py (kernel == judge, bit for bit) and
tests/test_otf_judge_cpu.py (no generated input has a pixel within 4 ulp of its sphere; the judge == nocs_otf on the same frames).

A small image, 48 x 64 with fx = fy = 60 and the principal point at the centre: the kernels take h, w and the intrinsics as
arguments.  Depths are about a metre, so a pixel is about 1/60 m wide and the whole image about 1.07 m x 0.8 m.  One case runs on
a 5 x 700 image: a box of 2049 = 3 x 683 pixels does not exist inside 48 x 64."""
from __future__ import annotations

import numpy as np

from captra_amd import nocs_otf
from tests import otf_judge as J

H, W = 48, 64
K = np.array([[60.0, 0.0, 32.0], [0.0, 60.0, 24.0], [0.0, 0.0, 1.0]])
WIDE_H, WIDE_W = 5, 700
WIDE_K = np.array([[60.0, 0.0, 350.0], [0.0, 60.0, 2.5], [0.0, 0.0, 1.0]])
ALL = 100.0                                      # a radius that takes every pixel with a depth


def kinv(intrinsics=K) -> np.ndarray:
    return np.linalg.inv(np.asarray(intrinsics, np.float64)).reshape(9)


def frame(seed, kind="dense", h=H, w=W):
    """-> depth (h,w) int32 millimetres, mask (h,w) uint8 (0, 1 and a few other non-zero bytes: the kernel copies the byte).
    kind: dense (every pixel > 0), half (about half of them 0), neg (a third negative, a third 0), zero."""
    rng = np.random.default_rng([seed, h, w])
    r, c = np.mgrid[0:h, 0:w]
    depth = (1000.0 + 90.0 * np.sin(r / 7.0 + seed) + 70.0 * np.cos(c / 9.0) + rng.uniform(-15, 15, (h, w))).astype(np.int32)
    u = rng.random((h, w))
    if kind == "half":
        depth[u < 0.5] = 0
    elif kind == "neg":
        depth[u < 0.33] = 0
        depth[u > 0.67] = -depth[u > 0.67]
    elif kind == "zero":
        depth[:] = 0
    else:
        assert kind == "dense", kind
    mask = rng.choice(np.array([0, 1, 1, 1, 200], np.uint8), (h, w))
    return depth, mask


def ball_case(name, depth, mask, box, center, radius, cap, h=H, w=W, intrinsics=K, det=None, named=()):
    depth, mask = np.asarray(depth, np.int32).reshape(-1, h, w), np.asarray(mask, np.uint8).reshape(-1, h, w)
    B = len(depth)
    return {"name": name, "h": h, "w": w, "kinv": kinv(intrinsics), "intrinsics": np.asarray(intrinsics, np.float64), "depth": depth, "mask": mask,
            "box": np.asarray(box, np.int32).reshape(B, 4), "center": np.asarray(center, np.float64).reshape(B, 3),
            "radius": np.asarray(radius, np.float64).reshape(B), "cap": int(cap), "det": det, "named": tuple(named)}


def _centre(rng):
    return np.array([rng.uniform(-0.2, 0.2), rng.uniform(-0.15, 0.15), -rng.uniform(0.95, 1.05)])


# box shapes (rows, cols) by pixel total: a wave is 64 pixels, a pass of the workgroup 1024
BOX_SHAPES = [(1, 1), (3, 21), (8, 8), (1, 64), (5, 13), (48, 1), (33, 31), (16, 64), (32, 32), (25, 41), (32, 64), (48, 64)]
TOTALS = sorted({bh * bw for bh, bw in BOX_SHAPES} | {2049})
assert set(TOTALS) >= {1, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 3072}


def ball_cases() -> list:
    """Every input of the captra_crop_ball / captra_crop_ball_det comparisons."""
    out = []
    for i, (bh, bw) in enumerate(BOX_SHAPES):
        rng = np.random.default_rng([11, bh, bw])
        r0, c0 = int(rng.integers(0, H - bh + 1)), int(rng.integers(0, W - bw + 1))
        box = (r0, c0, r0 + bh - 1, c0 + bw - 1)
        # every pixel a member: all waves of a pass full, counts = the box's total
        out.append(ball_case(f"all_{bh}x{bw}", *frame(i), box, _centre(rng), ALL, H * W))
        # about half the pixels without depth, a ball that cuts the box: centred near the surface at the box's middle, its radius
        # 0.55 .. 0.65 of the box's half diagonal (a pixel is 1/60 m wide at a metre)
        d, m = frame(100 + i, "half")
        z = 0.001 * float(np.abs(frame(100 + i)[0][r0 + bh // 2, c0 + bw // 2]))
        mid = np.array([((c0 + bw / 2) - 32) / 60 * z, ((H - (r0 + bh / 2)) - 24) / 60 * z, -z]) + rng.uniform(-0.004, 0.004, 3)
        out.append(ball_case(f"cut_{bh}x{bw}", d, m, box, mid, rng.uniform(0.55, 0.65) * np.hypot(bh, bw) / 120 + 0.02, H * W))
    # 2049 = 3 x 683 pixels: the wide image
    rng = np.random.default_rng(12)
    d, m = frame(7, "dense", WIDE_H, WIDE_W)
    out.append(ball_case("all_3x683", d, m, (1, 9, 3, 691), (0.3, 0.0, -1.0), ALL, WIDE_H * WIDE_W, WIDE_H, WIDE_W, WIDE_K))
    d, m = frame(8, "half", WIDE_H, WIDE_W)
    out.append(ball_case("cut_3x683", d, m, (1, 9, 3, 691), (0.31, 0.01, -0.99), 3.1234567, WIDE_H * WIDE_W, WIDE_H, WIDE_W, WIDE_K))
    # depth with negative values / nothing but zeros, one pass and three
    for kind in ("neg", "zero"):
        for bh, bw in ((16, 64), (48, 64)):
            d, m = frame(20, kind)
            out.append(ball_case(f"{kind}_{bh}x{bw}", d, m, (0, 0, bh - 1, bw - 1), _centre(rng), ALL if bh == 16 else 0.33, H * W))
    # empty boxes
    d, m = frame(21)
    out.append(ball_case("empty_rows", d, m, (30, 5, 29, 40), _centre(rng), ALL, H * W))
    out.append(ball_case("empty_cols", d, m, (5, 30, 40, 29), _centre(rng), ALL, H * W))
    out.append(ball_case("empty_both", d, m, (40, 50, 3, 2), _centre(rng), ALL, H * W))
    # more members than the table holds: instance 0 overflows, instance 1 (whose rows follow) does not; cap == count exactly
    d0, m0 = frame(30)
    d1, m1 = frame(31, "half")
    for cap, box0 in ((100, (0, 0, 47, 63)), (1000, (0, 0, 47, 63)), (1000, (16, 0, 31, 63)), (100, (3, 3, 12, 12)), (1024, (16, 0, 31, 63)),
                      (1023, (16, 0, 31, 63)), (1, (0, 0, 47, 63))):
        out.append(ball_case(f"cap{cap}_{(box0[2] - box0[0] + 1) * (box0[3] - box0[1] + 1)}", [d0, d1], [m0, m1], [box0, (18, 20, 29, 45)],
                         [_centre(rng), (0.0, 0.0, -1.0)], [ALL, 0.09], cap))
    # three instances of one launch: different frames, centres, radii; boxes = the projection of their balls (clamped at the border)
    rng = np.random.default_rng(13)
    frames = [frame(40, "dense"), frame(41, "half"), frame(42, "neg")]
    centers = np.array([[-0.45, 0.3, -1.0], [0.05, -0.02, -1.02], [0.4, -0.33, -0.97]]) + rng.uniform(-0.01, 0.01, (3, 3))
    radii = np.array([0.21, 0.0877, 0.3])
    boxes = nocs_otf.proj_corners_batch(H, W, centers, radii, K).reshape(3, 4)
    out.append(ball_case("three", [f[0] for f in frames], [f[1] for f in frames], boxes, centers, radii, H * W))
    out.append(ball_case("three_cap100", [f[0] for f in frames], [f[1] for f in frames], boxes, centers, radii, 100))
    # the detector variant: sel = -1, 0, ndet - 1, and indices outside the stack (the pre-fetched mask)
    ndet = 3
    rng = np.random.default_rng(14)
    B = 5
    frames = [frame(50 + b, "half" if b % 2 else "dense") for b in range(B)]
    det_masks = rng.choice(np.array([0, 1, 7], np.uint8), (B, ndet, H, W))
    centers = np.stack([_centre(rng) for _ in range(B)])
    radii = rng.uniform(0.15, 0.3, B)
    boxes = nocs_otf.proj_corners_batch(H, W, centers, radii, K).reshape(B, 4)
    out.append(ball_case("det", [f[0] for f in frames], [f[1] for f in frames], boxes, centers, radii, H * W,
                     det={"masks": det_masks, "sel": np.array([-1, 0, ndet - 1, ndet, ndet + 5], np.int32), "ndet": ndet}))
    # exact boundaries, from the judge's own float64 values of one pixel (which the boundary count leaves out by name)
    d, m = frame(60)
    box = (4, 6, 40, 57)
    rows, cols, pts = J.backproject(d, box, kinv(), H, W)
    i = int(np.nonzero((rows == 21) & (cols == 30))[0][0])
    pix = int(rows[i] * W + cols[i])
    out.append(ball_case("radius0_one_member", d, m, box, pts[i], 0.0, H * W, named=[pix]))
    centre = np.array([0.013, -0.021, -1.003])
    dist = J.distances(pts, centre)[i]
    assert 0.05 < dist < 0.3
    out.append(ball_case("radius_is_the_distance", d, m, box, centre, dist, H * W, named=[pix]))
    out.append(ball_case("radius_one_below_the_distance", d, m, box, centre, np.nextafter(dist, 0.0), H * W, named=[pix]))
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names), names
    return out


def masks_of(case) -> np.ndarray:
    """(B,h,w): the mask each instance of a case crops with (the detector variant's selection applied)."""
    if case["det"] is None:
        return case["mask"]
    det = case["det"]
    return np.stack([det["masks"][b, s] if 0 <= s < det["ndet"] else case["mask"][b] for b, s in enumerate(det["sel"])])


def judge_ball(case) -> list:
    """otf_judge.crop_ball of every instance of a case."""
    masks = masks_of(case)
    return [J.crop_ball(case["depth"][b], masks[b], case["box"][b], case["center"][b], case["radius"][b], case["kinv"], case["cap"], case["h"], case["w"])
            for b in range(len(case["depth"]))]


def boundary_count(case) -> int:
    return sum(len(J.boundary_pixels(case["depth"][b], case["box"][b], case["center"][b], case["radius"][b], case["kinv"], case["h"], case["w"],
                                     named=case["named"])) for b in range(len(case["depth"])))


# ---- captra_crop_box ----------------------------------------------------------------------------------------------------------
def f32_below(x):
    return np.nextafter(np.float32(x), np.float32(-np.inf))


def f32_above(x):
    return np.nextafter(np.float32(x), np.float32(np.inf))


def box_poses(h, w):
    """In-contract poses of captra_crop_box as launches (trans (B,3) fp32, scale (B,) fp32, radius_factor): around the frustum, the
    radius on / just above / just below the 0.05 floor and a scale of -0.0, balls close to the camera plane on either side of it
    and across it with |z +- r| >= 1e-3 (every projected value far inside int32: asserted by projected_extent)."""
    rng = np.random.default_rng([15, h, w])
    B = 70
    trans = np.stack([rng.uniform(-0.6, 0.6, B), rng.uniform(-0.5, 0.5, B), rng.uniform(-2.5, -0.4, B)], 1).astype(np.float32)
    scale = rng.uniform(0.01, 0.6, B).astype(np.float32)
    scale[:3] = (np.float32(-0.0), np.float32(0.0), np.float32(1e-30))
    launches = [(trans, scale, 0.6)]
    # factor 0.05 x scale 1.0 = the double 0.05 exactly
    fl_scale = np.array([1.0, f32_above(1.0), f32_below(1.0), 1.0, f32_above(1.0), f32_below(1.0)], np.float32)
    fl_trans = np.array([[0.1, -0.05, -0.9]] * 3 + [[-0.52, 0.4, -1.0]] * 3, np.float32)
    launches.append((fl_trans, fl_scale, 0.05))
    # the camera plane: r = 1.0 x scale; z + r or z - r a millimetre (and 1e-7, which covers the fp32 rounding of z and r) from 0, on
    # either side; balls behind the camera, across its plane, in front of it
    near = []
    mm = 1.0001e-3
    for r in (0.05, 0.25, 0.5):
        for z in (-r - mm, -r + mm, -r + 0.013, -0.5 * r, 0.0, 0.5 * r, r - mm, r + mm, r + 0.4):
            for xy in ((0.0, 0.0), (0.07, -0.04), (-0.3, 0.22)):
                near.append((xy[0], xy[1], z, r))
    near = np.array(near)
    launches.append((near[:, :3].astype(np.float32), near[:, 3].astype(np.float32), 1.0))
    return launches


def plane_gap(trans32, scale32, factor) -> np.ndarray:
    """min(|z + r|, |z - r|) per pose, from the values the kernel reads."""
    z = np.asarray(trans32, np.float32)[:, 2].astype(np.float64)
    r = np.maximum(np.float64(factor) * np.asarray(scale32, np.float32).astype(np.float64), 0.05)
    return np.minimum(np.abs(z + r), np.abs(z - r))


def projected_extent(trans32, scale32, factor, intrinsics) -> float:
    """Largest |u|, |v| over the eight corners of every pose, as proj_corners_batch evaluates them in float64 (must be finite and far
    below 2^31 for the int32 truncation to be defined)."""
    c = np.asarray(trans32, np.float32).astype(np.float64).reshape(-1, 3)
    r = np.maximum(np.float64(factor) * np.asarray(scale32, np.float32).astype(np.float64).reshape(-1, 1), 0.05)
    lo, hi = c - r, c + r
    sel = np.array([[x, y, z] for y in (0, 1) for x in (0, 1) for z in (0, 1)])
    box = np.where(sel[None] == 0, lo[:, None, :], hi[:, None, :]) * 1000.0
    homog = -box / box[:, :, 2:3]
    homog[:, :, 2] = -homog[:, :, 2]
    Km = np.asarray(intrinsics, np.float64)
    u = (Km[0, 0] * homog[:, :, 0] + Km[0, 1] * homog[:, :, 1]) + Km[0, 2] * homog[:, :, 2]
    v = (Km[1, 0] * homog[:, :, 0] + Km[1, 1] * homog[:, :, 1]) + Km[1, 2] * homog[:, :, 2]
    return float(max(np.abs(u).max(), np.abs(v).max()))


def lost_poses():
    """Poses a lost track produces, outside captra_crop_box's contract: (trans (B,3) fp32, scale (B,) fp32, radius_factor 0.5)."""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    rows = [((nan, 0.0, -1.0), 0.4), ((0.0, nan, -1.0), 0.4), ((0.0, 0.0, nan), 0.4), ((nan, nan, nan), 0.4),
            ((inf, 0.0, -1.0), 0.4), ((0.0, -inf, -1.0), 0.4), ((0.0, 0.0, -inf), 0.4), ((0.0, 0.0, inf), 0.4), ((-inf, inf, -inf), 0.4),
            ((0.0, 0.0, -1.0), nan), ((0.0, 0.0, -1.0), inf), ((0.0, 0.0, -1.0), -inf), ((nan, 0.0, -1.0), nan), ((inf, 0.0, 0.0), inf),
            ((0.0, 0.0, 0.0), 0.4), ((0.1, -0.1, 0.0), 0.02), ((0.0, 0.0, 1.0), 0.4), ((0.2, 0.1, 0.3), 0.4), ((0.0, 0.0, 3e38), 0.4),
            ((0.0, 0.0, -0.25), 0.5), ((0.1, 0.05, 0.25), 0.5), ((0.0, 0.0, -0.05), 0.0), ((0.0, 0.0, 0.05), 0.01),       # a corner at bz == 0
            ((0.0, 0.0, -1.0), 1e30), ((0.3, -0.2, -1.0), -1e30), ((0.0, 0.0, 0.0), 1e30), ((1e30, -1e30, -1.0), 0.4), ((1e-30, 0.0, -1e-30), 0.4),
            ((0.0, 0.0, -1e-4), 0.4), ((0.0, 0.0, -0.2 - 1e-7), 0.4)]
    trans = np.array([r[0] for r in rows], np.float32)
    scale = np.array([r[1] for r in rows], np.float32)
    return trans, scale, 0.5


# ---- captra_otf_candidates / captra_otf_finish ---------------------------------------------------------------------------------
def member_tables(B, cap, seed):
    """(B,cap,3) float64 member tables with every row defined (coordinates of the crop's kind, full double mantissas: the cast to
    fp32 rounds) and (B,cap) object bytes."""
    rng = np.random.default_rng([16, B, cap, seed])
    pts = rng.uniform(-0.5, 0.5, (B, cap, 3)) + np.array([0.0, 0.0, -1.0])
    obj = rng.choice(np.array([0, 1, 1, 200], np.uint8), (B, cap))
    return pts, obj


# (name, cap, stride, num_points, member counts, a rare row expected)
CANDIDATE_LAUNCHES = [
    ("s40_rare", 128, 40, 16, [0, 1, 9, 10, 11, 15, 16, 17, 21, 40, 41, 129], True),
    ("s40_plain", 128, 40, 16, [10, 11, 15, 16, 17, 21, 39, 40], False),
    ("s20_doubled_past_the_stride", 128, 20, 16, [11, 10, 20], True),                       # 11 -> 22 > 20
    ("s1100_cap_below_stride_rare", 128, 1100, 16, [0, 1, 9, 10, 11, 15, 16, 17, 21, 127, 128, 129, 1100, 1101, 129], True),
    ("s1100_cap_below_stride_one_over", 128, 1100, 16, [100, 129, 50], True),              # rare through `count > cap` alone
    ("s1100_cap_below_stride_plain", 128, 1100, 16, [10, 16, 21, 100, 128], False),
    ("s1100_plain", 2048, 1100, 16, [1100, 600, 10, 17, 1024, 1099], False),
    ("s1100_rare", 2048, 1100, 16, [1100, 1101, 2048, 2049, 9], True),
]


def random_rotations(B, seed):
    rng = np.random.default_rng([17, B, seed])
    out = []
    for _ in range(B):
        q, r = np.linalg.qr(rng.standard_normal((3, 3)))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        out.append(q)
    return np.stack(out)


# (name, cap, stride, member counts of the three instances)
FINISH_TABLES = [("s40", 128, 40, [17, 129, 5]), ("s40_b", 128, 40, [40, 0, 41]), ("s1100_cap_below_stride", 128, 1100, [129, 1101, 100]),
                 ("s1100", 2048, 1100, [1100, 333, 2049])]
FINISH_N = [1, 255, 256, 257]


def finish_inputs(cap, stride, n, seed, edge_rows):
    """B = 3: picks (3,n) int32 random in [0, stride) -- with edge_rows, row 1 all 0 and row 2 all stride - 1 --, mean (3,3) fp32,
    rot (3,3,3), trans (3,3), scale (3,) float64."""
    rng = np.random.default_rng([18, cap, stride, n, seed])
    picks = rng.integers(0, stride, (3, n)).astype(np.int32)
    if edge_rows:
        picks[1], picks[2] = 0, stride - 1
    mean = rng.uniform(-0.3, 0.3, (3, 3)).astype(np.float32) + np.array([0, 0, -1], np.float32)
    return picks, mean, random_rotations(3, seed), rng.uniform(-0.3, 0.3, (3, 3)) + np.array([0.0, 0.0, -1.0]), rng.uniform(0.2, 0.5, 3)


# ---- the chain ----------------------------------------------------------------------------------------------------------------
CHAIN_N, CHAIN_STRIDE, CHAIN_FACTOR = 64, 320, 0.6


def chain_inputs():
    """Three trajectories on the small image whose balls hold between 10 and CHAIN_STRIDE members (no rare row): depth, mask (3,H,W),
    trans (3,3) fp32, scale (3,) fp32 (radius = 0.6 scale, about 0.1 m = six pixels), and the ground-truth pose."""
    frames = [frame(70, "dense"), frame(71, "half"), frame(72, "neg")]
    trans = []
    for seed, (row, col) in zip((70, 71, 72), ((20, 26), (30, 44), (8, 60))):         # on the surface at that pixel (the last: at the border)
        z = 0.001 * float(frame(seed)[0][row, col])
        trans.append(((col - 32) / 60 * z, ((H - row) - 24) / 60 * z, -z))
    trans = np.array(trans, np.float32)
    scale = np.array([0.17, 0.2, 0.25], np.float32)
    picks, mean, rot, gt_trans, gt_scale = finish_inputs(H * W, CHAIN_STRIDE, CHAIN_N, 99, False)
    return {"depth": np.stack([f[0] for f in frames]), "mask": np.stack([f[1] for f in frames]), "trans": trans, "scale": scale, "mean": mean,
            "rot": rot, "gt_trans": trans.astype(np.float64) + 0.004, "gt_scale": gt_scale}


def chain_case():
    """The chain's crop as a ball case (box, centre, radius as captra_crop_box derives them: nocs_otf.proj_corners_batch of the fp32 pose)."""
    c = chain_inputs()
    centers = c["trans"].astype(np.float64)
    radii = np.maximum(np.float64(CHAIN_FACTOR) * c["scale"].astype(np.float64), 0.05)
    boxes = nocs_otf.proj_corners_batch(H, W, centers, radii, K).reshape(3, 4)
    return ball_case("chain", c["depth"], c["mask"], boxes, centers, radii, H * W)
