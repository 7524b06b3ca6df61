"""captra_image_members (csrc/image_fit.hip) through the C ABI against the numpy / float64 judge of tests/image_fit_judge.py.

pix, labels, counts and src are bit-equal to the judge's; tgt equals float32(judge) or the float32 next to it (the kernel's float64
back-projection may differ from numpy's in the last bit of the double, which moves the float32 rounding only at a tie).  Every case
runs with one workgroup per image, with the launcher's own choice and with several workgroups per image
(captra_image_members_set_split): the result does not depend on the launch geometry."""
import ctypes

import numpy as np
import pytest

from tests import image_fit_judge as IJ

SPLITS = (0, 1, 5)              # the launcher's choice, one workgroup per image, five (shares of 154 pixels on 24 x 32)
NONSQUARE = np.array([[31.0, 0.7, 15.25], [0.0, 23.5, 12.75], [0.0, 0.0, 1.0]])     # fx != fy, a skew term
POISON_F, POISON_I = 123.5, -77


def _abi(device, depth, mask, coord, kinv, cap, border, negate_z, split=0, shape=None, null=()):
    """The C ABI on poisoned outputs -> (err, dict of numpy outputs).  shape = (b, h, w) overrides what the arrays say; null: names
    of pointers handed over as NULL."""
    import torch
    from captra_amd import _lib as L
    b, h, w = depth.shape
    t = {"depth": torch.from_numpy(np.ascontiguousarray(depth, np.int32)).to(device), "mask": torch.from_numpy(np.ascontiguousarray(mask, np.uint8)).to(device),
         "coord": torch.from_numpy(np.ascontiguousarray(coord, np.uint8)).to(device), "kinv": torch.from_numpy(np.asarray(kinv, np.float64).reshape(9)).to(device),
         "src": torch.full((b, 1, 3, cap), POISON_F, dtype=torch.float32, device=device), "tgt": torch.full((b, 3, cap), POISON_F, dtype=torch.float32, device=device),
         "labels": torch.full((b, cap), POISON_I, dtype=torch.int32, device=device), "pix": torch.full((b, cap), POISON_I, dtype=torch.int32, device=device),
         "counts": torch.full((b, 3), POISON_I, dtype=torch.int32, device=device)}
    p = {k: (None if k in null or v.numel() == 0 else L.ptr(v)) for k, v in t.items()}
    b_, h_, w_ = shape if shape is not None else (b, h, w)
    lib = L.lib()
    lib.captra_image_members_set_split(ctypes.c_int(split))
    try:
        with torch.cuda.device(device):
            err = lib.captra_image_members(b_, h_, w_, cap, border, negate_z, p["depth"], p["mask"], p["coord"], p["kinv"], p["src"], p["tgt"],
                                           p["labels"], p["pix"], p["counts"], L.stream_ptr())
        torch.cuda.synchronize(device)
    finally:
        lib.captra_image_members_set_split(ctypes.c_int(0))
    return err, {k: t[k].cpu().numpy() for k in ("src", "tgt", "labels", "pix", "counts")}


def _check(got, ref, name):
    for k in ("counts", "pix", "labels", "src"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=f"{name}: {k}")
    assert IJ.tgt_agrees(got["tgt"], ref["tgt64"]), name
    for i, (c, used, _) in enumerate(ref["counts"]):                 # the padding slots, spelled out
        assert (got["labels"][i, used:] == -1).all() and (got["pix"][i, used:] == -1).all(), name
        assert (got["src"][i, :, :, used:] == 0).all() and (got["tgt"][i, :, used:] == 0).all(), name
    assert np.isfinite(got["src"]).all() and np.isfinite(got["tgt"]).all(), name


def _run(device, depth, mask, coord, K, cap, border, negate_z, name, splits=SPLITS):
    kinv = IJ.kinv_of(K)
    ref = IJ.members(depth, mask, coord, kinv, cap, border, bool(negate_z))
    first = None
    for split in splits:
        err, got = _abi(device, depth, mask, coord, kinv, cap, border, negate_z, split)
        assert err == 0, (name, split)
        _check(got, ref, f"{name} split={split}")
        if first is None:
            first = got
        for k in got:
            assert got[k].tobytes() == first[k].tobytes(), (name, split, k)
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [1, 7, 64])
@pytest.mark.parametrize("border", [0, 1, 2, 3])
def test_members_vs_judge(device, border, cap):
    """B = 3 images of 24 x 32: image 0 with exactly cap, cap + 1 and 2 cap + 1 members (steps 1, 2 and 3), images 1 and 2 random
    instances with holes in mask and depth; both NOCS intrinsics and a non-square matrix, negate_z on and off."""
    for n, (want, step) in enumerate(((cap, 1), (cap + 1, 2), (2 * cap + 1, 3))):
        depth, mask, coord = IJ.blob_case(100 * border + cap + n, members_wanted=want, border=border)
        K = (IJ.NOCS_INTRINSICS["real"], IJ.NOCS_INTRINSICS["camera"], NONSQUARE)[n]
        ref = _run(device, depth, mask, coord, K, cap, border, n & 1, f"border={border} cap={cap} members={want}")
        c, used, _ = ref["counts"][0]
        assert c == want and -(-c // max(-(-c // cap), 1)) == used and (1 if c <= cap else -(-c // cap)) == step


@pytest.mark.gpu
@pytest.mark.parametrize("border", [0, 1, 2, 3])
def test_edges_and_neighbouring_images(device, border):
    """An empty mask; a mask whose depth is all zero; an instance touching all four image edges (members at pixel (0,0) and at
    (h-1,w-1)); an instance in the first rows of image i + 1 under an image i whose last rows are background, and the other way round:
    the window must not cross images, nor wrap at a row end."""
    h, w, cap = 24, 32, 64
    rng = np.random.default_rng(border)
    depth = rng.integers(400, 3000, (6, h, w)).astype(np.int32)
    coord = rng.integers(0, 256, (6, h, w, 3)).astype(np.uint8)
    mask = np.zeros((6, h, w), np.uint8)
    mask[1, 4:20, 5:25] = 255                                         # image 0: empty mask; image 1: no depth under the mask
    depth[1] = 0
    mask[2] = 1                                                       # image 2: touches all four edges
    mask[3, h - 6:, :] = 9                                            # image 3: last rows set, image 4: first rows background
    mask[4, 6:, 3:w - 3] = 200
    mask[5, :6, :] = 7                                                # image 4: last rows set over image 5's first rows set ...
    mask[5, :6, w - 1] = 0                                            # ... whose row ends are background (a wrap would erode column 0)
    ref = _run(device, depth, mask, coord, NONSQUARE, cap, border, 1, f"edges border={border}")
    assert tuple(ref["counts"][0]) == (0, 0, 0)
    assert ref["counts"][1][0] == 0 and ref["counts"][1][2] > 0
    assert ref["counts"][2][0] == h * w and ref["pix"][2][0] == 0                      # every pixel of a full mask survives any border
    full = IJ.members(depth[2:3], mask[2:3], coord[2:3], IJ.kinv_of(NONSQUARE), 16384, border, True)
    assert full["pix"][0][h * w - 1] == h * w - 1                                      # ... the last one too
    err, got = _abi(device, depth[2:3], mask[2:3], coord[2:3], IJ.kinv_of(NONSQUARE), 16384, border, 1, split=3)
    assert err == 0
    _check(got, full, "full mask, cap 16384")
    alone = [IJ.members(depth[i:i + 1], mask[i:i + 1], coord[i:i + 1], IJ.kinv_of(NONSQUARE), cap, border, True) for i in range(6)]
    for i in range(6):                                                                 # an image's result does not depend on its neighbours
        for k in ("pix", "counts"):
            np.testing.assert_array_equal(ref[k][i], alone[i][k][0])


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", [(1, 37), (29, 1), (1, 1), (5, 3)])
def test_thin_images(device, h, w):
    for border in (0, 1, 3):
        rng = np.random.default_rng(h * 100 + w + border)
        depth = rng.integers(-1, 2000, (3, h, w)).astype(np.int32)
        mask = (rng.random((3, h, w)) < 0.8).astype(np.uint8) * 3
        coord = rng.integers(0, 256, (3, h, w, 3)).astype(np.uint8)
        _run(device, depth, mask, coord, IJ.NOCS_INTRINSICS["real"], 7, border, 0, f"h={h} w={w} border={border}", splits=(0, 1, 2))


@pytest.mark.gpu
def test_full_frame_more_members_than_cap(device):
    """480 x 640, B = 2, instances of more than 16384 members at cap 16384 (steps 2 and 3), with the launcher's own geometry, one
    workgroup per image and 75."""
    rng = np.random.default_rng(5)
    h, w = 480, 640
    r, c = np.mgrid[0:h, 0:w]
    depth = (900 + 0.3 * r + 0.2 * c + rng.integers(0, 5, (2, h, w))).astype(np.int32)
    depth[rng.random((2, h, w)) < 0.02] = 0
    mask = np.stack([(r - 230) ** 2 + (c - 330) ** 2 < 90 ** 2, (abs(r - 200) < 110) & (abs(c - 300) < 100)]).astype(np.uint8)
    mask[rng.random((2, h, w)) < 0.01] = 0
    coord = rng.integers(0, 256, (2, h, w, 3)).astype(np.uint8)
    ref = _run(device, depth, mask, coord, IJ.NOCS_INTRINSICS["real"], 16384, 1, 0, "480x640", splits=(0, 1, 75))
    assert ref["counts"][0][0] > 16384 and ref["counts"][1][0] > 2 * 16384
    assert -(-ref["counts"][0][0] // 16384) == 2 and -(-ref["counts"][1][0] // 16384) == 3


@pytest.mark.gpu
def test_refused_arguments_leave_the_outputs_untouched(device):
    depth, mask, coord = IJ.blob_case(3)
    kinv = IJ.kinv_of(IJ.NOCS_INTRINSICS["real"])
    b, h, w = depth.shape
    refused = [dict(shape=(-1, h, w)), dict(shape=(b, -1, w)), dict(shape=(b, h, -1)), dict(border=-1), dict(border=4),
               dict(shape=(1, 65536, 32768)), dict(shape=(1, 2 ** 31 - 1, 2))]
    refused += [dict(null=(k,)) for k in ("depth", "mask", "coord", "kinv", "src", "tgt", "labels", "pix", "counts")]
    for kw in refused:
        args = dict(cap=7, border=1)
        args.update({k: v for k, v in kw.items() if k in ("cap", "border")})
        err, got = _abi(device, depth, mask, coord, kinv, args["cap"], args["border"], 0, shape=kw.get("shape"), null=kw.get("null", ()))
        assert err == -1, kw
        assert (got["src"] == POISON_F).all() and (got["tgt"] == POISON_F).all(), kw
        assert (got["labels"] == POISON_I).all() and (got["pix"] == POISON_I).all() and (got["counts"] == POISON_I).all(), kw
    import torch
    from captra_amd import _lib as L
    with torch.cuda.device(device):                                   # cap < 1: no output array to hand over at all
        for cap in (0, -3):
            assert L.lib().captra_image_members(b, h, w, cap, 0, 0, None, None, None, None, None, None, None, None, None, L.stream_ptr()) == -1
    for shape in ((0, h, w), (b, 0, w), (b, h, 0)):                   # nothing to do: 0, and nothing written
        err, got = _abi(device, depth, mask, coord, kinv, 7, 1, 0, shape=shape, null=("depth", "src"))
        assert err == 0 and (got["counts"] == POISON_I).all() and (got["labels"] == POISON_I).all(), shape


@pytest.mark.gpu
def test_wrapper_and_fit(device):
    """nocs_otf.image_members: the kernel's outputs in the layouts part_fit_ransac_cn reads, the validation of its neighbours."""
    import torch
    from captra_amd.nocs_otf import image_members
    from captra_amd.pose_utils.pose_fit import part_fit_ransac_cn
    depth, mask, coord = IJ.blob_case(11)
    K = IJ.NOCS_INTRINSICS["camera"]
    d, m, c = (torch.from_numpy(a).to(device) for a in (depth, mask, coord))
    out = image_members(d, m.bool(), c, K, cap=64, border=1, negate_z=True)
    ref = IJ.members(depth, mask, coord, IJ.kinv_of(K), 64, 1, True)
    _check({k: v.cpu().numpy() for k, v in out.items()}, ref, "wrapper")
    one = image_members(d[1], m[1], c[1], K, cap=64, border=1, negate_z=True)
    for k in out:
        assert torch.equal(one[k], out[k][1]), k
    rot, scale, trans, valid, info = part_fit_ransac_cn(out["labels"], out["src"], out["tgt"], num_hyps=8, inlier_th=0.01)
    assert rot.shape == (3, 1, 3, 3) and torch.isfinite(rot).all() and torch.isfinite(scale).all() and torch.isfinite(trans).all()
    with pytest.raises(RuntimeError):
        image_members(d.cpu(), m, c, K)
    for bad in (dict(cap=2), dict(cap=16385), dict(border=4), dict(border=-1)):
        with pytest.raises(ValueError):
            image_members(d, m, c, K, **bad)
    with pytest.raises(ValueError):
        image_members(d.long(), m, c, K)
    with pytest.raises(ValueError):
        image_members(d, m, c[..., :2].contiguous(), K)
