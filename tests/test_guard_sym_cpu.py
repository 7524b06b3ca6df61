"""The axis-only inlier test of the symmetric categories without a GPU: the fixtures of tests/sym_judge.py meet the preconditions that
make every count and verdict immune to rounding, the float32 mirror agrees with the float64 judge on all of them, the full-rotation
judge (tests/guard_judge.py) calls the very same phi-rotated true poses lost, the command line and the model carry the two keys, and
the header, the binding table and the library agree on captra_part_fit_guard_sym / captra_part_fit_ransac_sym."""
import argparse
import logging
import re
from pathlib import Path

import numpy as np
import pytest

from tests import guard_judge as G
from tests import sym_judge as Y
from tests.test_guard_cpu import D, L

ROOT = Path(__file__).resolve().parent.parent

# what tests/test_guard_sym_gpu.py runs: shared, so that this file vouches for exactly those fixtures.  The smallest shapes that
# reach each path: a partial last pass; LDS staging at its limit; members re-read through the list; a lane offset in the draw key.
SHAPES = ((1, 1, 257, 0), (3, 4, 4096, 0), (2, 4, 4097, 0), (3, 1, 1025, 5))                         # B, P, N, b0
# B, P, N, b0, case seed, first mode: the single part of the first shape takes each of the three modes in turn
REFIT_CASES = ((1, 1, 257, 0, 0, 0), (1, 1, 257, 0, 0, 1), (1, 1, 257, 0, 0, 2), (3, 4, 4096, 0, 0, 0), (2, 4, 4097, 0, 0, 0), (3, 1, 1025, 5, 0, 0))
_CASES = {}


def cached(key, build):
    if key not in _CASES:
        _CASES[key] = build()
    return _CASES[key]


def check_fixture(B, P, N, with_mean):
    """(case, judge with its preconditions asserted, mirror)"""
    def build():
        c = Y.check_case(B, P, N, with_mean)
        return c, Y.preconditions(c, L, D), Y.judge(c, L, D, dt=np.float32)
    return cached(("check", B, P, N, with_mean), build)


def refit_fixture(B, P, N, b0, cseed, first):
    def build():
        c = Y.refit_case(B, P, N, cseed, first)
        return c, Y.preconditions(c, L, D, refit=True, b0=b0), Y.judge(c, L, D, refit=True, b0=b0, dt=np.float32)
    return cached(("refit", B, P, N, b0, cseed, first), build)


def test_mirror_follows_the_header_expression():
    """The fp32 mirror against a scalar transcription of include/captra_hip.h, bit for bit, and against float64 within fp32's reach."""
    f = np.float32
    rng = np.random.default_rng(3)
    S, T = (rng.random((50, 3)) - 0.5).astype(f), (rng.random((50, 3)) + 1.0).astype(f)
    R = G.J.random_rotation(rng)
    a, sc, tr = Y.params(R, 0.2, [0.4, 0.6, 1.5])
    got = Y.residual2(S, T, a, sc, tr, np.float32)
    for i in range(50):
        d = [f(T[i, k] - tr[k]) for k in range(3)]
        h = f(f(f(a[0] * d[0]) + f(a[1] * d[1])) + f(a[2] * d[2]))
        w = [f(d[k] - f(h * a[k])) for k in range(3)]
        rt = np.sqrt(f(f(f(w[0] * w[0]) + f(w[1] * w[1])) + f(w[2] * w[2])))
        hs, rs = f(sc * S[i, 1]), f(sc * np.sqrt(f(f(S[i, 0] * S[i, 0]) + f(S[i, 2] * S[i, 2]))))
        eh, er = f(h - hs), f(rt - rs)
        assert got[i] == f(f(eh * eh) + f(er * er))
    np.testing.assert_allclose(got, Y.residual2(S, T, a, sc, tr), rtol=1e-4)


def test_residual_is_invariant_under_the_in_plane_angle():
    """float64: composing the pose with R_y(phi) leaves every residual where it is (the second column is unchanged)."""
    rng = np.random.default_rng(5)
    S, T = (rng.random((40, 3)) - 0.5).astype(np.float32), (rng.random((40, 3)) + 1.0).astype(np.float32)
    R = G.J.random_rotation(rng)
    e = [Y.residual2(S, T, (R @ Y.rot_y(phi))[:, 1], np.float64(0.2), np.array([0.4, 0.6, 1.5])) for phi in (0.0, 0.7, 2.3)]
    np.testing.assert_allclose(e[1], e[0], rtol=1e-12)
    np.testing.assert_allclose(e[2], e[0], rtol=1e-12)


@pytest.mark.parametrize("B,P,N,b0", SHAPES)
def test_check_fixtures_preconditions_and_mirror(B, P, N, b0):
    """(1), (2) in float64 with and without pts_mean; the mirror gives the judge's counts and verdicts; parts of 0, 2, 3, 4 and N
    members, the pose with scale 0 and the member with a NaN target are there; a phi-rotated TRUE pose counts exactly its true
    inliers, where the full-rotation judge counts next to none and calls the part lost."""
    seen = set()
    for with_mean in (False, True):
        case, ref, mir = check_fixture(B, P, N, with_mean)
        for k in ("count", "inliers", "verdict"):
            np.testing.assert_array_equal(mir[k], ref[k], err_msg=f"{k} B={B} P={P} N={N}")
        seen |= set(ref["verdict"].ravel().tolist())
        old = G.judge(case, L, D)
        for (b, p), mode in case["modes"].items():
            if mode == "true" and ref["count"][b, p] >= 8:
                assert ref["verdict"][b, p] == Y.OK and ref["inliers"][b, p] == case["n_true"][b, p], (b, p)
                assert old["verdict"][b, p] == G.LOST and old["inliers"][b, p] <= 3, (b, p, old["inliers"][b, p])
        assert np.isnan(G.J.members_of(case, 0, 0)[2]).any()                     # the member with a NaN target
        assert ref["inliers"][0, P - 1] == 0 and ref["verdict"][0, P - 1] == Y.LOST  # the pose with scale 0
        if B >= 2 and P == 4:
            assert ref["count"][1].tolist() == [2, 3, 4, 0] and ref["verdict"][1].tolist() == [Y.TOO_FEW, Y.TOO_FEW, Y.OK, Y.TOO_FEW]
        if B >= 3:
            assert ref["count"][2, 0] > 0.99 * N and ref["verdict"][2, 0] == Y.LOST and ref["inliers"][2, 0] == 0
    assert Y.RECOVERED not in seen and Y.LOST in seen


@pytest.mark.parametrize("B,P,N,b0,cseed,first", REFIT_CASES)
def test_refit_fixtures_preconditions_and_mirror(B, P, N, b0, cseed, first):
    """(1)-(3) for the re-fit's fixtures; every mode ends as it should: phi-rotated true pose ok, 3 th along the y-axis recovered,
    gross outliers lost with the re-fit rejected; the mirror agrees; the fit alone is decidable on every part too."""
    case, ref, mir = refit_fixture(B, P, N, b0, cseed, first)
    for k in ("count", "inliers", "verdict"):
        np.testing.assert_array_equal(mir[k], ref[k], err_msg=k)
    want = {"true": Y.OK, "lost": Y.RECOVERED, "gross": Y.LOST}
    for (b, p), mode in case["modes"].items():
        assert ref["verdict"][b, p] == want[mode], (b, p, mode)
        if mode == "true":
            assert ref["inliers"][b, p] == case["n_true"][b, p]
    off = Y.judge(case, L, D, refit=False)
    np.testing.assert_array_equal(off["verdict"], np.where(ref["verdict"] == Y.RECOVERED, Y.LOST, ref["verdict"]))
    fit, pinned = Y.fit_preconditions(case, b0=b0)
    fmir = Y.judge_fit(case, b0=b0, dt=np.float32)
    for bp in pinned:
        assert fit["valid"][bp] and fmir["best"][bp] == fit["best"][bp] and fmir["num_inliers"][bp] == fit["num_inliers"][bp], bp
    for bp, mode in case["modes"].items():
        assert (bp in pinned) == (mode != "gross" and ref["count"][bp] >= 3), (bp, mode)


def test_every_shape_keeps_an_ok_a_recovered_and_a_rejected_part():
    for B, P, N, b0 in SHAPES:
        seen = set()
        for c in REFIT_CASES:
            if c[:4] == (B, P, N, b0):
                seen |= set(refit_fixture(*c)[1]["verdict"].ravel().tolist())
        assert {Y.OK, Y.RECOVERED, Y.LOST} <= seen, (B, P, N, seen)


# ---------------------------------------------------------------------------------------------------------------- configuration
def test_parse_args_carries_both_keys_only_when_written():
    from captra_amd.configs import make_config
    from captra_amd.parse_args import add_args
    args = add_args(argparse.ArgumentParser()).parse_args(["--track_cfg/guard/yaxis_only", "True", "--init_frame/yaxis_only", "True",
                                                           "--track_cfg/guard/lost_below", "0.5", "--init_frame/fit", "True"])
    assert getattr(args, "track_cfg/guard/yaxis_only") is True and getattr(args, "init_frame/yaxis_only") is True
    over = {k: v for k, v in vars(args).items() if v is not None and "/" in k}
    cfg = make_config("1", **over)
    assert cfg["track_cfg"]["guard"] == {"lost_below": 0.5, "yaxis_only": True}
    assert cfg["init_frame"]["yaxis_only"] is True and cfg["init_frame"]["fit"] is True
    none = vars(add_args(argparse.ArgumentParser()).parse_args([]))
    assert "track_cfg/guard/yaxis_only" not in none and "init_frame/yaxis_only" not in none
    cfg = make_config("1")
    assert "guard" not in cfg["track_cfg"] and "yaxis_only" not in cfg["init_frame"]


def test_guard_cfg_carries_the_key_only_when_on():
    from captra_amd.configs import make_config
    from captra_amd import track_options
    g = track_options.guard_cfg(make_config("1", **{"track_cfg/guard/lost_below": 0.5, "track_cfg/guard/yaxis_only": True}))
    assert g["yaxis_only"] is True
    for off in ({}, {"track_cfg/guard/yaxis_only": False}):
        g = track_options.guard_cfg(make_config("1", **{"track_cfg/guard/lost_below": 0.5, **off}))
        assert set(g) == {"refit", "lost_below", "inlier_th", "min_members", "num_hyps", "seed"}


def test_yaxis_only_on_a_category_that_is_not_symmetric_is_an_error():
    from captra_amd.configs import make_config
    from captra_amd.trainer import Trainer
    assert not make_config("6")["obj_sym"] and make_config("1")["obj_sym"]          # mug / bottle
    with pytest.raises(ValueError, match="yaxis_only"):
        Trainer(make_config("6", experiment_dir="/tmp/captra_test_exp", **{"track_cfg/guard/lost_below": 0.5, "track_cfg/guard/yaxis_only": True}))
    with pytest.raises(ValueError, match="yaxis_only"):
        Trainer(make_config("6", experiment_dir="/tmp/captra_test_exp", **{"init_frame/fit": True, "init_frame/yaxis_only": True}))


def test_full_rotation_test_on_a_symmetric_category_warns_once_per_model(caplog):
    from captra_amd.configs import make_config
    from captra_amd.trainer import Trainer

    def warnings_of(cat, **over):
        caplog.clear()
        with caplog.at_level(logging.WARNING, logger="captra_amd.model"):
            trainer = Trainer(make_config(cat, experiment_dir="/tmp/captra_test_exp", **over))
        return trainer.model, [r.getMessage() for r in caplog.records if "full-rotation" in r.getMessage()]

    model, msgs = warnings_of("1", **{"track_cfg/guard/lost_below": 0.5})
    assert len(msgs) == 1 and "track_cfg/guard/yaxis_only" in msgs[0] and "yaxis_only" not in model.guard
    model, msgs = warnings_of("1", **{"init_frame/fit": True})
    assert len(msgs) == 1 and "init_frame/yaxis_only" in msgs[0] and not model.fit_init_yaxis
    model, msgs = warnings_of("1", **{"init_frame/fit": True, "track_cfg/guard/lost_below": 0.5})
    assert len(msgs) == 1 and "init_frame/yaxis_only" in msgs[0] and "track_cfg/guard/yaxis_only" in msgs[0]
    model, msgs = warnings_of("1", **{"track_cfg/guard/lost_below": 0.5, "track_cfg/guard/yaxis_only": True, "init_frame/fit": True,
                                      "init_frame/yaxis_only": True})
    assert msgs == [] and model.guard["yaxis_only"] is True and model.fit_init_yaxis
    assert warnings_of("1")[1] == []                                                # neither feature on
    assert warnings_of("6", **{"track_cfg/guard/lost_below": 0.5})[1] == []         # not symmetric


def test_eval_heading_names_the_test():
    from captra_amd.eval import guard_table, guard_test_name
    rec = {k: np.zeros(1, np.int32) for k in ("count", "inliers", "rms", "verdict")}
    plain, sym = {"guard": [None, rec, rec]}, {"guard": [{"yaxis_only": np.True_}, rec, rec]}
    assert guard_test_name(plain) == "full-rotation" and guard_test_name(sym) == "axis-only"
    assert guard_table("x", plain) == guard_table("x", sym) and len(guard_table("x", sym)) == 1


def test_sym_symbols_in_header_binding_and_library():
    """Fails without the feature."""
    from captra_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "captra_hip.h").read_text(), flags=re.S)
    for name in ("captra_part_fit_guard", "captra_part_fit_ransac"):
        m, m0 = (re.search(r"int\s+" + n + r"\s*\(([^)]*)\)", text) for n in (name + "_sym", name))
        assert m, f"{name}_sym is not declared in include/captra_hip.h"
        # the argument list of the entry it stands beside, word for word
        assert re.sub(r"\s+", " ", m.group(1)) == re.sub(r"\s+", " ", m0.group(1))
        assert _lib._SIGNATURES[name + "_sym"] == _lib._SIGNATURES[name]
        assert hasattr(_lib.lib(), name + "_sym")
    # one copy of either test, in pose_solve.h
    csrc = ROOT / "captra_amd" / "csrc"
    holders = [p.name for p in sorted(csrc.iterdir()) if p.suffix in (".h", ".hip") and re.search(r"float\s+rs_residual2_sym\s*\(", p.read_text())]
    assert holders == ["pose_solve.h"], holders
