"""The judge of the depth support filter (tests/depth_judge.py) held to cases worked out by hand from the rule as include/captra_hip.h
states it, the case table of the GPU test held to catching every wrong variant of the rule, and the synthetic scene with flying pixels
(captra_amd.synthetic.make_frame(..., flying=0.5)) pinned on the condition the loop test relies on: at window 3, abs_mm 10,
min_support 12 the rule removes every injected pixel and no other pixel that has depth."""
import numpy as np
import pytest

from tests import depth_judge as J

INT_MAX = J.INT_MAX


def _run(rows, window, abs_mm, rel, ms):
    out, removed = J.judge(np.array(rows, np.int64), window, abs_mm, rel, ms)
    assert out.dtype == np.int32 and removed.dtype == np.int32
    return out.tolist(), removed.tolist()


@pytest.mark.parametrize("window", J.WINDOWS)
def test_a_single_pixel_image_has_no_neighbour(window):
    assert _run([[500]], window, 10 ** 6, 1000, 1) == ([[0]], [1])
    assert _run([[0]], window, 10 ** 6, 1000, 1) == ([[0]], [0])


@pytest.mark.parametrize("window", J.WINDOWS)
def test_a_pixel_alone_among_holes_is_removed(window):
    img = np.zeros((7, 7), np.int64)
    img[3, 3] = 700
    out, removed = J.judge(img, window, 50, 0, 1)
    assert not out.any() and removed.tolist() == [1]


@pytest.mark.parametrize("window,possible", [(1, 3), (2, 8), (3, 15)])
def test_corner_of_a_constant_image(window, possible):
    """A corner pixel has (window + 1)^2 - 1 in-image neighbours: kept with exactly that many asked for, removed with one more --
    while the centre pixel (all (2 window + 1)^2 - 1 of them) stays."""
    img = np.full((9, 9), 1000, np.int64)
    out, removed = J.judge(img, window, 0, 0, possible)
    assert (out == 1000).all() and removed.tolist() == [0]
    out, removed = J.judge(img, window, 0, 0, possible + 1)
    corners = [(0, 0), (0, 8), (8, 0), (8, 8)]
    assert all(out[rc] == 0 for rc in corners) and out[4, 4] == 1000 and out[0, 4] == 1000
    assert removed.tolist() == [4]
    out, removed = J.judge(img, window, 0, 0, (2 * window + 1) ** 2 - 1)
    assert removed.tolist() == [81 - (9 - 2 * window) ** 2]          # everything nearer than `window` to an edge goes


def test_a_neighbour_at_the_bound_supports_and_one_past_it_does_not():
    assert _run([[1000, 1007]], 1, 7, 0, 1) == ([[1000, 1007]], [0])
    assert _run([[1000, 1008]], 1, 7, 0, 1) == ([[0, 0]], [2])
    assert _run([[1007, 1000, 993]], 1, 7, 0, 2) == ([[0, 1000, 0]], [2])      # the middle one has two at the bound, the ends one each


def test_the_relative_tolerance_is_floored_and_is_the_pixels_own():
    """rel_permille = 1: d = 1999 -> floor(1.999) = 1, tol = abs_mm + 1 = 5; d = 2005 -> tol = 4 + 2 = 6.  At a distance of 6 the lower
    pixel is not supported by the upper one, the upper one is supported by the lower one."""
    assert _run([[1999, 2004]], 1, 4, 1, 1) == ([[1999, 2004]], [0])
    assert _run([[1999, 2005]], 1, 4, 1, 1) == ([[0, 2005]], [1])
    assert _run([[999, 1003]], 1, 4, 1, 1) == ([[999, 1003]], [0])             # 999 -> floor 0, tol 4: distance 4
    assert _run([[999, 1004]], 1, 4, 1, 1) == ([[0, 1004]], [1])


def test_holes_and_negative_depths_pass_through_and_support_nobody():
    assert _run([[-5, 0, -1, 3, 3]], 1, 0, 0, 1) == ([[-5, 0, -1, 3, 3]], [0])
    assert _run([[-5, 5, 0]], 1, INT_MAX, 1000, 1) == ([[-5, 0, 0]], [1])
    assert _run([[-INT_MAX - 1, -INT_MAX - 1]], 1, INT_MAX, 1000, 1) == ([[-INT_MAX - 1, -INT_MAX - 1]], [0])


def test_the_largest_depth_beside_the_smallest_does_not_overflow():
    assert _run([[INT_MAX, 1]], 1, 0, 0, 1) == ([[0, 0]], [2])
    assert _run([[INT_MAX, 1]], 1, INT_MAX - 2, 0, 1) == ([[0, 0]], [2])              # distance 2^31 - 2, tol 2^31 - 3: d + tol is past an int
    assert _run([[INT_MAX, 1]], 1, INT_MAX - 1, 0, 1) == ([[INT_MAX, 1]], [0])
    assert _run([[INT_MAX, 1]], 1, INT_MAX, 1000, 1) == ([[INT_MAX, 1]], [0])         # tol 2^32 - 2 and 2^31
    assert _run([[INT_MAX, 1]], 1, 0, 1000, 1) == ([[INT_MAX, 0]], [1])               # tol 2^31 - 1 for the large one, 1 for the small one


def test_images_of_a_batch_do_not_see_each_other():
    plane, holes = np.full((4, 5), 800, np.int64), np.zeros((4, 5), np.int64)
    out, removed = J.judge(np.stack([plane, holes, plane]), 1, 0, 0, 4)
    assert removed.tolist() == [4, 0, 4]                                              # the corners, in both planes alike
    one, _ = J.judge(plane, 1, 0, 0, 4)
    assert (out[0] == one).all() and (out[2] == one).all() and not out[1].any()


@pytest.mark.parametrize("mutant", J.MUTANTS)
def test_the_case_table_catches_the_wrong_rule(mutant):
    """Each wrong variant of the rule gives another image or another count on at least one case of the table the GPU test uses."""
    for name, depth, window, abs_mm, rel, ms in J.small_cases():
        right = J.judge(depth, window, abs_mm, rel, ms)
        wrong = J.judge(depth, window, abs_mm, rel, ms, mutant=mutant)
        if not (np.array_equal(right[0], wrong[0]) and np.array_equal(right[1], wrong[1])):
            return
    pytest.fail(f"no case of the table tells the '{mutant}' rule from the right one")


def test_the_case_table_is_the_one_the_issue_sets():
    assert J.SMALL_SHAPES == ((1, 1, 1), (1, 1, 70), (1, 70, 1), (3, 17, 65), (2, 33, 130)) and J.LARGE_SHAPE == (2, 480, 640)
    assert [J.supports(w) for w in J.WINDOWS] == [(1, 4, 8), (1, 12, 24), (1, 24, 48)]
    names = {name for name, *_ in J.contents((2, 33, 130))}
    assert {"constant", "holes", "checkerboard", "isolated", "step", "extremes_floor", "random_u16", "mirror"} <= names
    u16 = dict((n, d) for n, d, *_ in J.contents(J.LARGE_SHAPE))["random_u16"]
    assert 0.19 < (u16 == 0).mean() < 0.21 and u16.max() > 65000 and u16.min() == 0


SCENE = dict(window=3, abs_mm=10, rel_permille=0, min_support=12)


@pytest.mark.parametrize("blob_px", [70, 90])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_the_scene_loses_every_flying_pixel_and_nothing_else(seed, blob_px):
    """make_frame(seed, blob_px, flying=0.5): 600-900 injected pixels per frame; the judge removes all of them and none of the other
    ~300 000 pixels that have depth.  A condition of the scene, not a tolerance: the loop test's part (b) stands on it."""
    from captra_amd.synthetic import make_frame
    depth, _, _, _, injected = make_frame(seed, blob_px=blob_px, flying=0.5, return_flying=True)
    out, removed = J.judge(depth.astype(np.int32), **SCENE)
    has = depth > 0
    genuine_removed = int((has & ~injected & (out == 0)).sum())
    print(f"seed {seed} blob_px {blob_px}: injected {int(injected.sum())}, removed {int(removed[0])}, injected removed "
          f"{int((injected & (out == 0)).sum())}, genuine removed {genuine_removed} of {int((has & ~injected).sum())}")
    assert injected.sum() > 400 and injected[has].sum() == injected.sum()
    assert (out[injected] == 0).all()
    assert genuine_removed == 0
    assert int(removed[0]) == int(injected.sum())
