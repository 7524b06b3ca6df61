"""A numpy / float64 judge for captra_image_members (tests/test_image_fit_gpu.py, tests/test_image_fit_judge_cpu.py,
tests/test_image_fit_loop_gpu.py), written from the rule in include/captra_hip.h and not from the kernel:

  * eroded mask: pixel (r,c) is inside when mask != 0 at every (r',c') with r' in [r - border + 1, r + border] and [0,h), c' in
    [c - border + 1, c + border] and [0,w); border = 0: the pixel's own byte.  One image at a time, nothing wraps at a row end;
  * members: the inside pixels with depth > 0 in row-major order, c of them; c <= cap: all are used, else step = ceil(c / cap) and the
    members j with j % step == 0; used = ceil(c / step); holes = the inside pixels with depth <= 0;
  * slot s < used: pix = r w + c, labels = 0, tgt = (p_x, p_y, -p_z) * 0.001 of p = ray * z / ray_z, ray = kinv (c, h - r, 1) in
    float64 (z = the depth as float32), src_k = coord_k / 255.0 - 0.5 (src_2 negated with negate_z); the other slots -1 / -1 / 0.

`members(..., variant=...)` is the same judge with ONE deliberate mistake (MUTATIONS): what the tests must be able to tell apart.
`fit_chain` runs the members through the float64 RANSAC judge of tests/ransac_judge.py, as the model's first-pose fit does.
"""
import numpy as np

from tests import ransac_judge as RJ

NOCS_INTRINSICS = {"real": np.array([[591.0125, 0, 322.525], [0, 590.16775, 244.11084], [0, 0, 1]]),
                   "camera": np.array([[577.5, 0, 319.5], [0., 577.5, 239.5], [0., 0., 1.]])}
MUTATIONS = ("symmetric_window", "step_off_by_one", "h_minus_r_minus_1", "column_major", "neighbouring_image", "no_negate_z")


def eroded(mask, border, variant=None, nxt=None):
    """mask (h,w) any dtype -> (h,w) bool: the pixels inside the eroded mask.  (nxt: the next image of the batch, read only by the
    'neighbouring_image' mutation, which lets a window run past the last row as a flat buffer would.)"""
    h, w = mask.shape
    on = np.asarray(mask) != 0
    if border == 0:
        return on.copy()
    lo = border if variant == "symmetric_window" else border - 1
    out = np.zeros((h, w), bool)
    for r in range(h):
        for c in range(w):
            r0, r1 = max(r - lo, 0), r + border
            c0, c1 = max(c - lo, 0), min(c + border, w - 1)
            if variant == "neighbouring_image" and nxt is not None:
                rows = [on[rr] if rr < h else (np.asarray(nxt) != 0)[rr - h] for rr in range(r0, min(r1, 2 * h - 1) + 1)]
                out[r, c] = all(row[c0:c1 + 1].all() for row in rows)
            else:
                out[r, c] = on[r0:min(r1, h - 1) + 1, c0:c1 + 1].all()
    return out


def decode(coord, negate_z=False):
    """coord (...,3) uint8 -> float64 NOCS: coord / 255.0 - 0.5, the third axis negated with negate_z."""
    out = np.asarray(coord).astype(np.float64) / 255.0 - 0.5
    if negate_z:
        out[..., 2] = -out[..., 2]
    return out


def backproject(rows, cols, z, h, kinv, variant=None):
    """Pixels (rows, cols) with depths z (int) of an image of height h -> (n,3) float64 camera points in metres."""
    v = (h - rows - 1) if variant == "h_minus_r_minus_1" else (h - rows)
    k = np.asarray(kinv, np.float64).reshape(3, 3)
    u, v = cols.astype(np.float64), v.astype(np.float64)
    ray = np.stack([(k[i, 0] * u + k[i, 1] * v) + k[i, 2] for i in range(3)], -1)
    zz = z.astype(np.float32).astype(np.float64)
    p = ray * zz[:, None] / ray[:, 2:3]
    p[:, 2] = -p[:, 2]
    return p * 0.001


def members(depth, mask, coord, kinv, cap, border=0, negate_z=False, variant=None):
    """depth (b,h,w) int, mask (b,h,w), coord (b,h,w,3) uint8, kinv 9 or (3,3) float64 -> dict: src (b,1,3,cap) float32, tgt64 (b,3,cap)
    float64 (tgt: its float32 rounding), labels, pix (b,cap) int32, counts (b,3) int32."""
    depth, mask, coord = np.asarray(depth), np.asarray(mask), np.asarray(coord)
    b, h, w = depth.shape
    src = np.zeros((b, 1, 3, cap), np.float32)
    tgt64 = np.zeros((b, 3, cap), np.float64)
    labels = np.full((b, cap), -1, np.int32)
    pix = np.full((b, cap), -1, np.int32)
    counts = np.zeros((b, 3), np.int32)
    for i in range(b):
        inside = eroded(mask[i], border, variant, nxt=mask[i + 1] if i + 1 < b else None)
        member = inside & (depth[i] > 0)
        if variant == "column_major":
            cols, rows = np.nonzero(member.T)
        else:
            rows, cols = np.nonzero(member)
        c = len(rows)
        step = 1 if c <= cap else -(-c // cap)
        if variant == "step_off_by_one" and c > cap:
            step += 1
        rows, cols = rows[::step], cols[::step]
        used = len(rows)
        assert used == -(-c // step) and used <= cap
        counts[i] = (c, used, int((inside & (depth[i] <= 0)).sum()))
        if used == 0:
            continue
        pix[i, :used] = rows * w + cols
        labels[i, :used] = 0
        tgt64[i, :, :used] = backproject(rows, cols, depth[i][rows, cols], h, kinv, variant).T
        src[i, 0, :, :used] = decode(coord[i][rows, cols], negate_z and variant != "no_negate_z").T.astype(np.float32)
    return dict(src=src, tgt64=tgt64, tgt=tgt64.astype(np.float32), labels=labels, pix=pix, counts=counts)


def same(a, b) -> bool:
    """Two results of `members` agree in everything the kernel writes."""
    return all(np.array_equal(a[k], b[k]) for k in ("src", "tgt64", "labels", "pix", "counts"))


def tgt_agrees(got, tgt64) -> bool:
    """got float32 equals float32(judge) or the float32 next to it: the kernel's float64 result may differ from numpy's in the last
    bit of the double, which moves the float32 rounding only at a tie."""
    ref = np.asarray(tgt64).astype(np.float32)
    got = np.asarray(got, np.float32)
    return bool(((got == ref) | (got == np.nextafter(ref, np.float32(np.inf))) | (got == np.nextafter(ref, np.float32(-np.inf)))).all())


def kinv_of(intrinsics):
    return np.linalg.inv(np.asarray(intrinsics, np.float64)).reshape(9)


def fit_chain(mem, th, num_hyps=64, seed=0, dt=np.float64):
    """The members (a result of `members`, or the kernel's outputs as numpy arrays under the same keys with 'tgt' float32) through
    the RANSAC judge with the kernel's own draws: judge_batch's result for (b, 1)."""
    labels = np.asarray(mem["labels"])
    b, cap = labels.shape
    ranks = np.zeros((b, 1, num_hyps, 3), np.int64)
    for i in range(b):
        count = int((labels[i] == 0).sum())
        if count >= 3:
            ranks[i, 0] = RJ.draw_ranks(seed, i, 0, num_hyps, count)
    return RJ.judge_batch(labels, np.asarray(mem["src"], np.float32), np.asarray(mem["tgt"], np.float32), th, ranks, None, dt), ranks


def pose_errors(rot, scale, trans, gt_rot, gt_scale, gt_trans):
    """Rotation (degrees), translation (mm) and relative scale error of one pose against the ground truth."""
    cos = (np.trace(np.asarray(rot, np.float64).T @ np.asarray(gt_rot, np.float64)) - 1.0) / 2.0
    return (float(np.degrees(np.arccos(np.clip(cos, -1.0, 1.0)))),
            float(1000.0 * np.linalg.norm(np.asarray(trans, np.float64).reshape(3) - np.asarray(gt_trans, np.float64).reshape(3))),
            float(abs(float(scale) - float(gt_scale)) / float(gt_scale)))


# ---- small cases shared by the CPU and GPU tests ------------------------------------------------------------------------
def blob_case(seed, b=3, h=24, w=32, members_wanted=None, border=0):
    """b images of h x w with a rectangular instance each (somewhere inside, holes in the mask and in the depth), random coordinate
    images.  members_wanted: image 0 gets exactly that many members at `border` (depth holes are adjusted), for the step cases."""
    rng = np.random.default_rng(seed)
    depth = rng.integers(400, 3000, (b, h, w)).astype(np.int32)
    depth[rng.random((b, h, w)) < 0.1] = 0
    depth[rng.random((b, h, w)) < 0.02] = -5
    mask = np.zeros((b, h, w), np.uint8)
    for i in range(b):
        r0, c0 = (rng.integers(0, max(h // 3, 1)), rng.integers(0, max(w // 3, 1)))
        mask[i, r0:r0 + max(2 * h // 3, 1), c0:c0 + max(2 * w // 3, 1)] = rng.integers(1, 256)
    holes = rng.random((b, h, w)) < 0.01
    if members_wanted is not None:
        holes[0] = False                     # (a hole of the mask costs a whole window: image 0 keeps the pixels its count needs)
    mask[holes] = 0
    coord = rng.integers(0, 256, (b, h, w, 3)).astype(np.uint8)
    if members_wanted is not None:
        inside = eroded(mask[0], border)
        rows, cols = np.nonzero(inside)
        assert len(rows) >= members_wanted, (len(rows), members_wanted)
        depth[0][inside] = 0
        keep = np.sort(rng.choice(len(rows), members_wanted, replace=False))
        depth[0][rows[keep], cols[keep]] = rng.integers(400, 3000, members_wanted)
    return depth, mask, coord
