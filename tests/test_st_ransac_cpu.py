"""CPU: the float64 judge of the robust scale / translation fit (tests/st_ransac_judge.py) -- its estimator pinned to the oracle's
one-pass fit, what it is for (outliers), its in-plane invariance -- and the configuration surface of track_cfg/st_fit: flags,
track_options.st_fit_cfg, the table of captra_amd.eval."""
import argparse
import pickle
import re
from pathlib import Path

import numpy as np
import pytest

from tests import ransac_judge as J
from tests import st_ransac_judge as SJ

ROOT = Path(__file__).resolve().parent.parent


def _recipe_part(seed, count, sym, outliers=True):
    """One recipe cloud with its true rotation as the kernel would be given it: fp32, for sym composed with R_y(phi) before rounding
    and the outliers clear of the surface of revolution by 3 th (st_ransac_judge.batch_case's rules).  -> S, T, th, true_in, rot, (s, t)."""
    rng = np.random.default_rng(seed * 100 + count)
    S, T, th, tin, (R, s, t) = SJ.recipe_cloud(rng, count, outliers=outliers)
    T = T.astype(np.float64)
    if sym:
        out = np.nonzero(~tin)[0]
        while len(out):
            e = np.sqrt(SJ.residual2(S[out], T[out].astype(np.float32), R[:, 1], np.float64(s), t))
            out = out[e <= 3 * th]
            T[out] = t + (rng.random((len(out), 3)) - 0.5) * 100 * th
        R = R @ SJ.rot_y(rng.uniform(0.5, 2.5))
    return S, T.astype(np.float32), th, tin, R.astype(np.float32), (s, t), SJ.draw_triples(rng, count)


@pytest.mark.parametrize("sym", [False, True])
@pytest.mark.parametrize("count", [4, 40, 257])
def test_estimator_is_the_oracles_one_pass_fit(count, sym):
    """All members inliers: E in float64 = oracle.ops.part_fit_st.  The oracle computes in double and ROUNDS ITS OUTPUTS to fp32, so
    the bound is 1e-12 relative (two double evaluations of the same algebra) plus that rounding, half an fp32 ulp = 2^-24 relative
    per output."""
    from oracle import ops
    S, T, th, _, rot, _, _ = _recipe_part(3, count, sym, outliers=False)
    Rp, s, t = SJ.estimator(S, T, rot, sym)
    o_s, o_t, o_v = ops.part_fit_st(np.zeros((1, count), np.int32), S.T[None, None], T.T[None], rot[None, None], sym)
    assert o_v[0, 0] == (count > 3)
    assert abs(s - o_s[0, 0]) <= 1e-12 * abs(s) + 2.0 ** -24 * abs(s)
    assert (np.abs(t - o_t[0, 0]) <= 1e-12 * np.abs(t).max() + 2.0 ** -24 * np.abs(t)).all()
    # fit() on triples that cover only inliers ends in the same E on all members
    j = SJ.fit(S, T, rot, SJ.draw_triples(np.random.default_rng(1), count), th, sym)
    assert j["inliers"].all() and abs(j["pose"][0] - s) <= 1e-12 * abs(s)


@pytest.mark.parametrize("sym", [False, True])
@pytest.mark.parametrize("count", [c for c in J.RECIPE_COUNTS if c >= 40])
def test_robust_against_plain_on_the_recipe(count, sym):
    """30 % gross outliers, the true rotation given: the plain estimator misses the scale by more than 10 %, the judge by less
    than 1e-3 (relative), on every recipe part; the mirror selects the same inliers."""
    for seed in J.RECIPE_SEEDS:
        S, T, th, tin, rot, (s_true, t_true), triples = _recipe_part(seed, count, sym)
        j = SJ.check_precondition(S, T, rot, triples, th, tin, sym)
        s_plain, t_plain = SJ.plain(S, T, rot, sym)
        s_fit, t_fit = j["pose"]
        print(f"count {count} seed {seed} sym {sym}: plain {abs(s_plain - s_true) / s_true:.3f} ({np.abs(t_plain - t_true).max() / th:.1f} th), "
              f"robust {abs(s_fit - s_true) / s_true:.1e} ({np.abs(t_fit - t_true).max() / th:.1e} th)")
        assert abs(s_plain - s_true) / s_true > 0.10, (seed, s_plain, s_true)
        assert abs(s_fit - s_true) / s_true < 1e-3, (seed, s_fit, s_true)
        m = SJ.fit(S, T, rot, triples, th, sym, np.float32)
        assert (m["inliers"] == j["inliers"]).all()


@pytest.mark.parametrize("count", [40, 1500])
def test_in_plane_invariance(count):
    """sym: scale, translation and the inlier set do not depend on the in-plane angle of the given rotation."""
    S, T, th, tin, rot, _, triples = _recipe_part(5, count, True)
    R = rot.astype(np.float64)
    ref = SJ.fit(S, T, R, triples, th, True)
    for alpha in (0.3, 1.7, -2.9):
        got = SJ.fit(S, T, R @ SJ.rot_y(alpha), triples, th, True)
        assert (got["inliers"] == ref["inliers"]).all() and (got["inliers"] == tin).all()
        assert abs(got["pose"][0] - ref["pose"][0]) <= 1e-9 and np.abs(got["pose"][1] - ref["pose"][1]).max() <= 1e-9


def test_batch_case_has_every_kind_of_part():
    case = SJ.batch_case(257, 2257, False, True, False)
    ref = SJ.judge_batch(case)
    counts = [[int((case["labels"][b] == p).sum()) for p in range(3)] for b in range(3)]
    assert counts[1] == [2, 3, 4] and counts[2] == [257, 0, 0] and counts[0][2] >= 3
    v = ref["valid"]
    assert v.tolist() == [[True, True, False], [False, False, True], [True, False, False]]
    assert ref["num_inliers"][1].tolist() == [0, 3, 4] and ref["num_inliers"][0, 2] < 3          # 3 members: found, not valid
    for b, p in zip(*np.nonzero(~v)):
        assert ref["scale"][b, p] == case["prev_scale"][b, p] and (ref["trans"][b, p] == case["prev_trans"][b, p]).all()
    off = SJ.judge_batch(case, prev=False)
    assert (off["scale"][~v] == 1.0).all() and (off["trans"][~v] == 0.0).all()
    assert np.isnan(case["src"]).any() and np.isinf(case["tgt"]).any()


# ---------------------------------------------------------------------------------------------------------- configuration
def test_parse_args_builds_the_st_fit_cfg():
    from captra_amd.configs import make_config
    from captra_amd.parse_args import add_args
    flags = ["--track_cfg/st_fit/ransac", "True", "--track_cfg/st_fit/inlier_th", "0.01", "--track_cfg/st_fit/num_hyps", "32",
             "--track_cfg/st_fit/seed", "3"]
    args = add_args(argparse.ArgumentParser()).parse_args(flags)
    over = {k: v for k, v in vars(args).items() if k.startswith("track_cfg/st_fit/")}
    assert over == {"track_cfg/st_fit/ransac": True, "track_cfg/st_fit/inlier_th": 0.01, "track_cfg/st_fit/num_hyps": 32,
                    "track_cfg/st_fit/seed": 3}
    cfg = make_config("1", **over)
    assert cfg["track_cfg"]["st_fit"] == {"ransac": True, "inlier_th": 0.01, "num_hyps": 32, "seed": 3}
    none = add_args(argparse.ArgumentParser()).parse_args([])
    assert all(v is None for k, v in vars(none).items() if k.startswith("track_cfg/st_fit/"))
    assert "st_fit" not in make_config("1")["track_cfg"]


def test_st_fit_cfg_defaults_and_errors():
    from captra_amd.configs import make_config
    from captra_amd import track_options
    from captra_amd.track_options import INIT_FIT_INLIER_TH
    assert track_options.st_fit_cfg(make_config("1")) is None
    assert track_options.st_fit_cfg(make_config("1", **{"track_cfg/st_fit/ransac": False, "track_cfg/st_fit/num_hyps": 0})) is None
    cfg = make_config("1", **{"track_cfg/st_fit/ransac": True})
    assert track_options.st_fit_cfg(cfg) == {"inlier_th": INIT_FIT_INLIER_TH * cfg["data_radius"], "num_hyps": 64, "seed": 0}
    cfg = make_config("1", **{"track_cfg/st_fit/ransac": True, "init_frame/num_hyps": 48, "init_frame/seed": 9})
    assert track_options.st_fit_cfg(cfg) == {"inlier_th": INIT_FIT_INLIER_TH * cfg["data_radius"], "num_hyps": 48, "seed": 9}
    cfg = make_config("1", **{"track_cfg/st_fit/ransac": True, "track_cfg/st_fit/inlier_th": 0.01, "track_cfg/st_fit/num_hyps": 32,
                              "track_cfg/st_fit/seed": 3})
    assert track_options.st_fit_cfg(cfg) == {"inlier_th": 0.01 * cfg["data_radius"], "num_hyps": 32, "seed": 3}
    for key, bad in (("inlier_th", 0.0), ("inlier_th", -0.01), ("num_hyps", 0), ("num_hyps", -4), ("num_hyps", 257), ("seed", -1)):
        with pytest.raises(ValueError, match=key):
            track_options.st_fit_cfg(make_config("1", **{"track_cfg/st_fit/ransac": True, f"track_cfg/st_fit/{key}": bad}))
    from captra_amd.trainer import Trainer
    with pytest.raises(ValueError, match="num_hyps"):
        Trainer(make_config("1", experiment_dir="/tmp/captra_test_exp", **{"track_cfg/st_fit/ransac": True, "track_cfg/st_fit/num_hyps": 0}))
    on = Trainer(make_config("1", experiment_dir="/tmp/captra_test_exp", **{"track_cfg/st_fit/ransac": True})).model
    off = Trainer(make_config("1", experiment_dir="/tmp/captra_test_exp")).model
    assert on.st_fit is not None and on.net.st_fit is on.st_fit and off.st_fit is None and off.net.st_fit is None


def test_eval_prints_the_st_fit_table(tmp_path, capsys):
    """A hand-made result pickle with 'st_fit' -> the table; the same pickle without the key -> nothing new."""
    from captra_amd import eval as ev
    from tests.golden.make_golden_eval import make_inputs
    gc, pc, gt, pred = make_inputs(11 + 4, 4)
    base = {"pred": {"poses": [gt, pred, pred, pred], "corners": [None, pc, pc, pc]}, "gt": {"poses": [gt] * 4, "corners": gc},
            "frame_nums": [["0"], ["1"], ["2"], ["3"]]}
    rec = [None] + [{"inliers": np.array([100, 50, 0, 7], np.int32), "valid": np.array([1, 1, 0, v], np.int32)} for v in (1, 0, 1)]
    argv = ["--obj_category", "drawers", "--obj_config", "obj_info_sapien.yml"]
    out = {}
    for name, data in (("off", base), ("on", dict(base, st_fit=rec))):
        d = tmp_path / name / "results" / "data"
        d.mkdir(parents=True)
        with open(d / "inst0_track0.pkl", "wb") as f:
            pickle.dump(data, f)
        ev.main(argv + ["--experiment_dir", str(tmp_path / name)])
        out[name] = capsys.readouterr().out
    assert "st_fit" not in out["off"] and "robust" not in out["off"]
    assert out["on"].startswith(out["off"])
    table = out["on"][len(out["off"]):].splitlines()
    assert "track_cfg/st_fit" in table[0] and len(table) == 5
    assert re.search(r"part 0: kept 3; previous value 0; mean inliers 100\.0 \(of 3 frames\)", table[1])
    assert re.search(r"part 2: kept 0; previous value 3 \[1 2 3\]; mean inliers - ", table[3])
    assert re.search(r"part 3: kept 2; previous value 1 \[2\]; mean inliers 7\.0 ", table[4])
    # with the guard's record beside it: the fraction of the part's members
    lines = ev.st_fit_table("x", {"st_fit": rec, "guard": [None] + [{"count": np.array([200, 50, 0, 70], np.int32)}] * 3})
    assert "mean inlier fraction 0.500" in lines[0] and "mean inlier fraction 0.100" in lines[3] and "fraction" not in lines[2]


def test_symbol_in_header_binding_and_library():
    """Fails without the feature."""
    from captra_amd import _lib
    from captra_amd.pose_utils.pose_fit import part_fit_st_ransac, part_fit_st_ransac_track  # noqa: F401
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "captra_hip.h").read_text(), flags=re.S)
    m = re.search(r"int\s+captra_part_fit_st_ransac\s*\(([^)]*)\)", text)
    assert m, "captra_part_fit_st_ransac is not declared in include/captra_hip.h"
    assert len(m.group(1).split(",")) == len(_lib._SIGNATURES["captra_part_fit_st_ransac"])      # (the stream included)
    assert hasattr(_lib.lib(), "captra_part_fit_st_ransac")
    # one body: the new kernel instantiates rs_fit of pose_ransac.h with its solver, and carries no copy of the stages
    src = (ROOT / "captra_amd" / "csrc" / "pose_st_ransac.hip").read_text()
    assert "rs_fit<SYM>" in src and "RsGivenRot<SYM>" in src and "captra_allow_lds<kern>" in src and "atomicAdd" not in src
