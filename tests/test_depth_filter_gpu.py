"""captra_depth_support_filter (csrc/depth_filter.hip, captra_amd.nocs_otf.depth_support_filter) held bit for bit -- images and removed
counts -- to the numpy judge (tests/depth_judge.py) on the judge's case table: shapes that straddle the 16 x 64 tile and its halo,
windows 1..3, min_support at 1 / middle / maximum, and contents built to tell the rule from each wrong variant of it
(tests/test_depth_judge_cpu.py shows that they do).  Depth is integer millimetres and the rule pure integer arithmetic: there is
no tolerance."""
import numpy as np
import pytest
import torch

from tests import depth_judge as J

pytestmark = pytest.mark.gpu

SENT = -77


def _filter(depth_np, window, abs_mm, rel, ms, device):
    from captra_amd.nocs_otf import depth_support_filter
    src = torch.from_numpy(np.ascontiguousarray(depth_np)).to(device)
    keep = src.clone()
    out, removed = depth_support_filter(src, window, abs_mm, rel, ms)
    assert torch.equal(src, keep), "the input image was written"
    assert out.dtype == torch.int32 and removed.dtype == torch.int32 and out.is_cuda and removed.is_cuda
    return out.cpu().numpy(), removed.cpu().numpy()


@pytest.mark.parametrize("window", J.WINDOWS)
@pytest.mark.parametrize("shape", J.SMALL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_small_shapes_equal_the_judge(device, shape, window):
    """Every content at every min_support of this (shape, window)."""
    bad = []
    for name, depth, abs_mm, rel in J.contents(shape):
        for ms in J.supports(window):
            want, want_removed = J.judge(depth, window, abs_mm, rel, ms)
            got, got_removed = _filter(depth, window, abs_mm, rel, ms, device)
            assert got.shape == want.shape and got_removed.shape == want_removed.shape
            if not (np.array_equal(got, want) and np.array_equal(got_removed, want_removed)):
                bad.append((name, ms, int((got != want).sum()), got_removed.tolist(), want_removed.tolist()))
    assert not bad, bad


def test_large_shape_equals_the_judge(device):
    """(2, 480, 640), once: seeded uint16 depths with 20 % holes whose second image is the first one's mirror, window 3, the middle
    min_support -- 300 tiles per image, every tile boundary inside an image."""
    (depth, abs_mm, rel), = [(d.copy(), a, r) for n, d, a, r in J.contents(J.LARGE_SHAPE) if n == "random_u16"]
    depth[1] = depth[0, ::-1, ::-1]
    want, want_removed = J.judge(depth, 3, abs_mm, rel, 24)
    got, got_removed = _filter(depth, 3, abs_mm, rel, 24, device)
    assert 0.1 < want_removed[0] / (depth[0] > 0).sum() < 0.9              # the case decides something
    assert want_removed[0] == want_removed[1] and np.array_equal(want[1], want[0, ::-1, ::-1])       # (the judge itself: a mirror's result is the mirror)
    assert np.array_equal(got, want) and np.array_equal(got_removed, want_removed)


def test_removed_is_added_to_what_the_caller_left_there(device):
    """The C entry point increases `removed`: the wrapper zeroes it, a caller of the library may accumulate."""
    from captra_amd import _lib as L
    depth = np.zeros((2, 20, 70), np.int32)
    depth[0, 3, 3] = depth[1, 19, 69] = depth[1, 0, 64] = 900
    src = torch.from_numpy(depth).to(device)
    out = torch.full_like(src, SENT)
    removed = torch.tensor([5, 7], dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        L.call("captra_depth_support_filter", 2, 20, 70, 2, 10, 0, 1, L.ptr(src), L.ptr(out), L.ptr(removed))
    assert removed.cpu().tolist() == [6, 9] and not out.cpu().numpy().any()


def test_out_of_range_arguments_launch_nothing(device):
    from captra_amd import _lib as L
    src = torch.full((2, 8, 8), 1000, dtype=torch.int32, device=device)
    out = torch.full_like(src, SENT)
    removed = torch.full((2,), SENT, dtype=torch.int32, device=device)
    fn = L.lib().captra_depth_support_filter
    imax = 2 ** 31 - 1
    bad = [(-1, 8, 8, 2, 10, 0, 6), (2, -1, 8, 2, 10, 0, 6), (2, 8, -1, 2, 10, 0, 6), (2, 8, 8, 0, 10, 0, 1), (2, 8, 8, 4, 10, 0, 1),
           (2, 8, 8, -1, 10, 0, 1), (2, 8, 8, 2, -1, 0, 6), (2, 8, 8, 2, 10, -1, 6), (2, 8, 8, 2, 10, 1001, 6), (2, 8, 8, 2, 10, 0, 0),
           (2, 8, 8, 1, 10, 0, 9), (2, 8, 8, 2, 10, 0, 25), (2, 8, 8, 3, 10, 0, 49), (2, 8, 8, 2, 10, 0, -3), (2, 8, 8, 2, 10, 0, imax)]
    with torch.cuda.device(device):
        st = L.stream_ptr()
        for args in bad:
            assert fn(*args, L.ptr(src), L.ptr(out), L.ptr(removed), st) == -1, args
        assert fn(2, 8, 8, 2, 10, 0, 6, L.ptr(src), L.ptr(src), L.ptr(removed), st) == -1                    # in place
        assert fn(1, 8, 8, 2, 10, 0, 6, L.ptr(src), L.ptr(src) + 4 * 32, L.ptr(removed), st) == -1           # overlapping
        assert fn(2, 8, 8, 2, 10, 0, 6, L.ptr(src), None, L.ptr(removed), st) == -1
        for args in ((0, 8, 8), (2, 0, 8), (2, 8, 0)):                                                        # nothing to do: 0
            assert fn(*args, 2, 10, 0, 6, L.ptr(src), L.ptr(out), L.ptr(removed), st) == 0, args
        torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENT).all() and (removed.cpu().numpy() == SENT).all() and (src.cpu().numpy() == 1000).all()
    from captra_amd.nocs_otf import depth_support_filter
    with pytest.raises(ValueError, match="min_support"):
        depth_support_filter(src, 2, 10, 0, 25)
    with pytest.raises(ValueError, match="int32"):
        depth_support_filter(src.long(), 2, 10, 0, 6)


def test_single_image_form(device):
    """(H,W) in, (H,W) and a 0-dim count out: the first image of the batched call."""
    from captra_amd.nocs_otf import depth_support_filter
    name, depth, abs_mm, rel = J.contents((2, 33, 130))[-2]
    assert name == "random_ramp"
    want, want_removed = J.judge(depth[0], 2, abs_mm, rel, 12)
    out, removed = depth_support_filter(torch.from_numpy(depth[0].copy()).to(device), 2, abs_mm, rel, 12)
    assert tuple(out.shape) == (33, 130) and tuple(removed.shape) == () and 0 < int(removed) == int(want_removed[0])
    assert np.array_equal(out.cpu().numpy(), want)


def test_cpu_tensor_raises(device):
    from captra_amd.nocs_otf import depth_support_filter
    with pytest.raises(RuntimeError, match="CPU"):
        depth_support_filter(torch.zeros(1, 4, 4, dtype=torch.int32), 1, 0, 0, 1)
