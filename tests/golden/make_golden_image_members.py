"""Golden fixture G17 (image members): the reference's mask erosion and back-projection (datasets/nocs_data/nocs_utils.py
`remove_border`, `backproject`) on tiny single-instance images, and the coordinate decode of its pose preprocessing on random bytes.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_image_members.py [--ref /root/reference]

Nothing of the reference is copied: nocs_utils is imported read-only from --ref (it needs numpy and torch only) and run on seeded
images.  Written per case: the inputs (depth (h,w) int32, mask (h,w) uint8 with the instance's id on its pixels and 255 = background,
the id, the kernel size, the intrinsics) and the reference's outputs (the eroded mask, the points (n,3) float64 and the pixel rows /
columns of backproject on the eroded instance).  The decode has no function of its own in the reference (it is three lines inside a
loop that reads files, get_gt_poses.py:73-76), so it is computed here with numpy from its definition -- channels reversed, / 255 - 0.5,
the third axis negated for the splits whose images are not mirrored -- on a random (6,8,3) image and on all 256 byte values.  Data only, ~30 KB.
"""
import argparse
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
INTRINSICS = (np.array([[591.0125, 0, 322.525], [0, 590.16775, 244.11084], [0, 0, 1]]),
              np.array([[577.5, 0, 319.5], [0., 577.5, 239.5], [0., 0., 1.]]))
CASES = ((12, 16, 1, 0), (12, 16, 2, 1), (16, 20, 1, 1), (16, 20, 2, 0), (24, 32, 1, 0), (24, 32, 2, 1))    # (h, w, kernel size, intrinsics)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=str(HERE / "g17_image_members.npz"))
    args = ap.parse_args()
    sys.path.insert(0, str(Path(args.ref) / "datasets" / "nocs_data"))
    import nocs_utils as NU

    blob = {"num_cases": np.int64(len(CASES))}
    for k, (h, w, ks, which) in enumerate(CASES):
        rng = np.random.default_rng(1800 + k)
        inst = int(rng.integers(1, 7))
        mask = np.full((h, w), 255, np.uint8)
        r0, c0 = int(rng.integers(0, 3)), int(rng.integers(0, 3))                 # k even: the instance touches the image's corner
        if k % 2 == 0:
            r0 = c0 = 0
        mask[r0:r0 + 2 * h // 3, c0:c0 + 3 * w // 4] = inst
        mask[rng.random((h, w)) < 0.01] = 255                                     # background specks inside the instance
        depth = rng.integers(300, 4000, (h, w)).astype(np.int32)
        depth[rng.random((h, w)) < 0.1] = 0
        out = NU.remove_border(mask, kernel_size=ks)
        pts, idxs = NU.backproject(depth, INTRINSICS[which], out == inst)
        assert len(pts) >= 3, (k, len(pts))
        blob[f"depth{k}"], blob[f"mask{k}"], blob[f"inst{k}"], blob[f"ks{k}"] = depth, mask, np.int64(inst), np.int64(ks)
        blob[f"intrinsics{k}"] = INTRINSICS[which]
        blob[f"eroded{k}"], blob[f"pts{k}"] = out, np.asarray(pts, np.float64)
        blob[f"rows{k}"], blob[f"cols{k}"] = np.asarray(idxs[0], np.int64), np.asarray(idxs[1], np.int64)
    rng = np.random.default_rng(1899)
    for name, bgr in (("image", rng.integers(0, 256, (6, 8, 3)).astype(np.uint8)),
                      ("table", np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, axis=2))):
        rgb = bgr[:, :, ::-1]
        nocs = rgb / 255. - 0.5
        flipped = nocs.copy()
        flipped[..., 2] = -flipped[..., 2]
        blob[f"coord_bgr_{name}"], blob[f"nocs_{name}"], blob[f"nocs_negz_{name}"] = bgr, nocs, flipped
    np.savez_compressed(args.out, **blob)
    print("wrote", args.out, Path(args.out).stat().st_size, "bytes")


if __name__ == "__main__":
    main()
