"""CPU: the float64 judge of tests/iou_judge.py against the existing host path.  The numpy `pts_inside_box` in the kernel's place
must satisfy the judge's bounds on every generic pair, the ambiguous share must stay under the cap, and nothing outside the band
may differ -- this guards the yardstick that tests/test_iou_gpu.py applies to captra_box_iou."""
import numpy as np

from captra_amd.pose_utils.bbox_utils import iou_3d, pts_inside_box
from tests import iou_judge as J


def test_numpy_path_satisfies_the_judge_on_generic_pairs():
    pairs = J.generic_pairs()
    assert len(pairs) == 2 * 6 + 24
    for name, b1, b2 in pairs:
        r = J.bounds(b1, b2)
        n1, n2 = pts_inside_box(r["grid"], b1), pts_inside_box(r["grid"], b2)
        inter, union = int((n1 & n2).sum()), int((n1 | n2).sum())
        print(name, "union", r["union64"], "A", r["A"], "numpy", inter, union, "decided", r["inter"], r["union"])
        assert r["union64"] > 1000, name
        assert r["A"] <= J.CAP * r["union64"], (name, r["A"], r["union64"])
        assert r["inter"] <= inter <= r["inter"] + r["A"], name
        assert r["union"] <= union <= r["union"] + r["A"], name
        assert not (((n1 != r["in1"]) | (n2 != r["in2"])) & ~r["amb"]).any(), name       # no mismatch outside the band
        assert iou_3d(b1, b2) == inter / union


def test_axis_aligned_pairs_are_over_the_cap():
    """Why the canonical pairs are compared by tolerance instead: faces on grid planes make thousands of points ambiguous."""
    for name, b1, b2 in J.axis_aligned_pairs():
        r = J.bounds(b1, b2)
        assert r["A"] > J.CAP * r["union64"], name
