"""The track guard without a GPU: the judge's fixtures (tests/guard_judge.py) meet the preconditions that make every verdict immune
to rounding, the float32 mirror agrees with the float64 judge on all of them, the command line and the model carry the
configuration, and the header, the binding table and the library agree on captra_part_fit_guard."""
import argparse
import re
from pathlib import Path

import numpy as np
import pytest

from tests import guard_judge as G

ROOT = Path(__file__).resolve().parent.parent

# what tests/test_guard_gpu.py runs: shared, so that this file vouches for exactly those fixtures
LOST_BELOW = 0.45
L, D = 9, 20
CHECK_B, CHECK_P = (1, 3), (1, 4)
CHECK_N = (1, 3, 63, 64, 65, 255, 1025, 4096, 4097)
REFIT_CASES = ((1, 1, 257, 0, 0), (3, 4, 4096, 0, 1), (3, 4, 4096, 5, 0), (2, 4, 4097, 0, 0), (3, 1, 1025, 5, 0))   # B, P, N, b0, case seed


def test_lost_ratio_is_the_written_fraction():
    from captra_amd.pose_utils.pose_fit import lost_ratio
    assert lost_ratio(LOST_BELOW) == (L, D)
    assert lost_ratio(0.3) == (3, 10) and lost_ratio(0.5) == (1, 2) and lost_ratio((2, 7)) == (2, 7) and lost_ratio(1) == (1, 1)
    for bad in (-0.1, 1.5, (1, 0)):
        with pytest.raises(ValueError):
            lost_ratio(bad)


@pytest.mark.parametrize("N", CHECK_N)
def test_check_fixtures_preconditions_and_mirror(N):
    """Every fixture of the check at this N: preconditions (1), (2) in float64; the mirror gives the judge's counts and verdicts."""
    seen = set()
    for B in CHECK_B:
        for P in CHECK_P:
            for with_mean in (False, True):
                case = G.check_case(B, P, N, with_mean)
                ref = G.preconditions(case, L, D)
                mir = G.judge(case, L, D, dt=np.float32)
                for k in ("count", "inliers", "verdict"):
                    np.testing.assert_array_equal(mir[k], ref[k], err_msg=f"{k} B={B} P={P} N={N}")
                seen |= set(ref["verdict"].ravel().tolist())
                if B == 3 and P == 4 and N >= 63:
                    assert ref["count"][1].tolist() == [2, 3, 4, 0] and ref["count"][2].tolist() == [N, 0, 0, 0]
                    assert ref["verdict"][1].tolist() == [G.TOO_FEW, G.TOO_FEW, G.OK, G.TOO_FEW] and ref["verdict"][2, 0] == G.LOST
                    assert ref["inliers"][0, 3] < ref["count"][0, 3]                         # the pose with scale 0
                    assert np.isnan(G.J.members_of(case, 0, 0)[2]).any()                     # the member with a NaN target
    assert G.RECOVERED not in seen
    if N >= 63:
        assert {G.OK, G.TOO_FEW, G.LOST} <= seen


@pytest.mark.parametrize("B,P,N,b0,cseed", REFIT_CASES)
def test_refit_fixtures_preconditions_and_mirror(B, P, N, b0, cseed):
    """(1)-(3) for the re-fit's fixtures; every mode ends as the issue says: true pose ok, 30 degrees / 3 th off recovered, gross
    outliers lost with the re-fit rejected; the mirror agrees on every verdict."""
    case = G.refit_case(B, P, N, cseed)
    ref = G.preconditions(case, L, D, refit=True, b0=b0)
    mir = G.judge(case, L, D, refit=True, b0=b0, dt=np.float32)
    np.testing.assert_array_equal(mir["verdict"], ref["verdict"])
    np.testing.assert_array_equal(mir["inliers"], ref["inliers"])
    want = {"true": G.OK, "off": G.RECOVERED, "gross": G.LOST}
    for (b, p), mode in case["modes"].items():
        assert ref["verdict"][b, p] == want[mode], (b, p, mode)
    off = G.judge(case, L, D, refit=False)
    np.testing.assert_array_equal(off["verdict"], np.where(ref["verdict"] == G.RECOVERED, G.LOST, ref["verdict"]))


def test_parse_args_builds_the_guard_cfg():
    from captra_amd.configs import make_config
    from captra_amd.parse_args import add_args
    flags = ["--track_cfg/guard/refit", "True", "--track_cfg/guard/lost_below", "0.5", "--track_cfg/guard/inlier_th", "0.01",
             "--track_cfg/guard/min_members", "6", "--track_cfg/guard/num_hyps", "32", "--track_cfg/guard/seed", "3"]
    args = add_args(argparse.ArgumentParser()).parse_args(flags)
    over = {k: v for k, v in vars(args).items() if k.startswith("track_cfg/guard/")}
    assert over == {"track_cfg/guard/refit": True, "track_cfg/guard/lost_below": 0.5, "track_cfg/guard/inlier_th": 0.01,
                    "track_cfg/guard/min_members": 6, "track_cfg/guard/num_hyps": 32, "track_cfg/guard/seed": 3}
    cfg = make_config("1", **over)
    assert cfg["track_cfg"]["guard"] == {"refit": True, "lost_below": 0.5, "inlier_th": 0.01, "min_members": 6, "num_hyps": 32, "seed": 3}
    none = add_args(argparse.ArgumentParser()).parse_args([])
    assert all(v is None for k, v in vars(none).items() if k.startswith("track_cfg/guard/"))
    assert "guard" not in make_config("1")["track_cfg"]


def test_model_needs_lost_below():
    from captra_amd.configs import make_config
    from captra_amd import track_options
    from captra_amd.track_options import INIT_FIT_INLIER_TH
    cfg = make_config("1")
    assert track_options.guard_cfg(cfg) is None
    with pytest.raises(ValueError, match="lost_below"):
        track_options.guard_cfg(make_config("1", **{"track_cfg/guard/refit": True}))
    with pytest.raises(ValueError, match="lost_below"):
        from captra_amd.trainer import Trainer
        Trainer(make_config("1", experiment_dir="/tmp/captra_test_exp", **{"track_cfg/guard/refit": True}))
    cfg = make_config("1", **{"track_cfg/guard/lost_below": 0.5})
    g = track_options.guard_cfg(cfg)
    assert g == {"refit": False, "lost_below": (1, 2), "inlier_th": INIT_FIT_INLIER_TH * cfg["data_radius"], "min_members": 4,
                 "num_hyps": 64, "seed": 0}


def test_guard_symbol_in_header_binding_and_library():
    """Fails without the feature."""
    from captra_amd import _lib
    from captra_amd.pose_utils.pose_fit import part_fit_guard_cn  # noqa: F401
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "captra_hip.h").read_text(), flags=re.S)
    m = re.search(r"int\s+captra_part_fit_guard\s*\(([^)]*)\)", text)
    assert m, "captra_part_fit_guard is not declared in include/captra_hip.h"
    assert len(m.group(1).split(",")) == len(_lib._SIGNATURES["captra_part_fit_guard"])      # (the stream included)
    assert hasattr(_lib.lib(), "captra_part_fit_guard")
    # one copy of the inlier test, in pose_solve.h
    csrc = ROOT / "captra_amd" / "csrc"
    holders = [p.name for p in sorted(csrc.iterdir()) if p.suffix in (".h", ".hip") and re.search(r"bool\s+rs_inlier\s*\(", p.read_text())]
    assert holders == ["pose_solve.h"], holders
