"""The float64 judge of the consensus rotation read-out against its float32 mirror on the recipe, the batch fixture, the configuration
(parse_args, defaults, errors), the eval table, and the symbol in header, binding table and library.  No GPU."""
import argparse
import pickle
import re
from pathlib import Path

import numpy as np
import pytest

from tests import rot_consensus_judge as RJ

ROOT = Path(__file__).resolve().parents[1]


# ------------------------------------------------------------------------------------------------------------------- judge
@pytest.mark.parametrize("sym", [False, True])
@pytest.mark.parametrize("count", [40, 257, 4096])
def test_judge_and_mirror_agree_on_the_recipe(count, sym):
    """The preconditions hold, the mirror selects the judge's set and best, the plain mean is more than the metric's 5 degrees from
    R_true and the consensus within 0.5 degrees."""
    rng = np.random.default_rng(count + sym)
    raw, tin, Rt = RJ.recipe_part(rng, count, sym)
    ranks = rng.integers(0, count, 64)
    j = RJ.check_precondition(raw, ranks, RJ.TH_DEG, tin, sym)
    assert RJ.pinned_best(j, RJ.TH_DEG, sym)
    m = RJ.fit(raw, ranks, RJ.cos_th_of(RJ.TH_DEG), sym, np.float32)
    assert m["best"] == j["best"] and (m["inliers"] == j["inliers"]).all() and (m["score"] == j["score"]).all()
    assert m["dR"].dtype == np.float32 and np.abs(m["dR"] - j["dR"]).max() < 1e-5
    plain, robust = RJ.plain_mean_angle(raw, sym, Rt), RJ.plain_mean_angle(raw, sym, Rt, j["inliers"])
    print(f"count {count} sym {sym}: plain mean {plain:.2f} deg from R_true, consensus {robust:.2f} deg")
    assert plain > 5.0 and robust < 0.6
    R = j["dR"]
    assert np.abs(R.T @ R - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12


def test_votes_are_the_readouts():
    """ortho6d: x = a / |a|, z = x cross c normalised, y = z cross x; a degenerate input votes (1,0,0); the sym vote is a unit axis."""
    rng = np.random.default_rng(0)
    R = RJ.random_rotation(rng)
    raw = RJ.raw_of(rng, R, False).astype(np.float32)[:, None]
    V = RJ.votes(raw, False)[0]
    assert np.abs(V.T - R).max() < 1e-6
    assert (RJ.votes(np.zeros((3, 1), np.float32), True)[0, 0] == [1, 0, 0]).all()
    nan = RJ.votes(np.full((6, 1), np.nan, np.float32), False)[0]
    assert (nan[0] == [1, 0, 0]).all() and (nan[1] == 0).all() and (nan[2] == [1, 0, 0]).all()
    # the default frames
    assert (RJ.pool(np.zeros((0, 3, 3)), np.zeros(0, bool), False) == np.eye(3)).all()
    assert (RJ.pool(np.zeros((0, 1, 3)), np.zeros(0, bool), True)[:, 1] == [0, 1, 0]).all()


@pytest.mark.parametrize("sym", [False, True])
def test_batch_case_has_every_kind_of_part(sym):
    case = RJ.batch_case(257, 3257 + 10 * sym, sym)
    ref, mir = RJ.judge_batch(case), RJ.judge_batch(case, dt=np.float32)
    assert ref["count"][1].tolist() == [0, 1, 2] and ref["count"][2].tolist() == [257, 0, 0] and (ref["count"][0] >= 20).all()
    assert ref["num_inliers"][1].tolist() == [0, 1, 2]
    b, p = case["nan_part"]
    assert ref["num_inliers"][b, p] == (ref["count"][b, p] if sym else 0)
    if not sym:
        assert (ref["delta"][b, p] == np.eye(3)).all()
    assert np.isnan(case["raw"]).any() and np.isfinite(ref["rot"]).all() and np.isfinite(ref["delta"]).all()
    for k in ("count", "num_inliers", "best"):
        assert (ref[k] == mir[k]).all()
    assert np.abs(ref["rot"] - mir["rot"]).max() < 1e-5
    # kernel draws: the generator's first draw, also for parts of fewer than three members
    assert (RJ.hyp_ranks(5, 0, 1, 64, 40) == RJ.draw_ranks(5, 0, 1, 64, 40)[:, 0]).all()
    assert set(RJ.hyp_ranks(5, 1, 2, 64, 2)) == {0, 1} and (RJ.hyp_ranks(5, 1, 1, 64, 1) == 0).all()
    # a non-diagonal raw holds the same heads
    nd = RJ.batch_case(257, 3257 + 10 * sym, sym, diag=False)
    assert nd["raw"].shape == (9, 3, 3 if sym else 6, 257)
    assert (RJ.judge_batch(nd)["best"] == ref["best"]).all()


# ---------------------------------------------------------------------------------------------------------- configuration
def test_parse_args_builds_the_rot_pool_cfg():
    from captra_amd.configs import make_config
    from captra_amd.parse_args import add_args
    flags = ["--track_cfg/rot_pool/consensus", "True", "--track_cfg/rot_pool/angle_th", "20", "--track_cfg/rot_pool/num_hyps", "32",
             "--track_cfg/rot_pool/seed", "3"]
    args = add_args(argparse.ArgumentParser()).parse_args(flags)
    over = {k: v for k, v in vars(args).items() if k.startswith("track_cfg/rot_pool/")}
    assert over == {"track_cfg/rot_pool/consensus": True, "track_cfg/rot_pool/angle_th": 20.0, "track_cfg/rot_pool/num_hyps": 32,
                    "track_cfg/rot_pool/seed": 3}
    cfg = make_config("1", **over)
    assert cfg["track_cfg"]["rot_pool"] == {"consensus": True, "angle_th": 20.0, "num_hyps": 32, "seed": 3}
    none = add_args(argparse.ArgumentParser()).parse_args([])
    assert all(v is None for k, v in vars(none).items() if k.startswith("track_cfg/rot_pool/"))
    assert "rot_pool" not in make_config("1")["track_cfg"]


def test_rot_pool_cfg_defaults_and_errors():
    from captra_amd.configs import make_config
    from captra_amd import track_options
    assert track_options.rot_pool_cfg(make_config("1")) is None
    assert track_options.rot_pool_cfg(make_config("1", **{"track_cfg/rot_pool/consensus": False, "track_cfg/rot_pool/num_hyps": 0})) is None
    on = {"track_cfg/rot_pool/consensus": True, "track_cfg/rot_pool/angle_th": 15.0}
    assert track_options.rot_pool_cfg(make_config("1", **on)) == {"angle_th": 15.0, "num_hyps": 64, "seed": 0}
    cfg = make_config("1", **on, **{"init_frame/num_hyps": 48, "init_frame/seed": 9})
    assert track_options.rot_pool_cfg(cfg) == {"angle_th": 15.0, "num_hyps": 48, "seed": 9}
    cfg = make_config("1", **on, **{"track_cfg/rot_pool/num_hyps": 32, "track_cfg/rot_pool/seed": 3})
    assert track_options.rot_pool_cfg(cfg) == {"angle_th": 15.0, "num_hyps": 32, "seed": 3}
    with pytest.raises(ValueError, match="angle_th"):          # no default
        track_options.rot_pool_cfg(make_config("1", **{"track_cfg/rot_pool/consensus": True}))
    for key, bad in (("angle_th", 0.0), ("angle_th", -5.0), ("angle_th", 180.0), ("angle_th", float("nan")), ("num_hyps", 0), ("num_hyps", 257),
                     ("seed", -1)):
        with pytest.raises(ValueError, match=key):
            track_options.rot_pool_cfg(make_config("1", **{**on, f"track_cfg/rot_pool/{key}": bad}))
    from captra_amd.trainer import Trainer
    with pytest.raises(ValueError, match="angle_th"):
        Trainer(make_config("1", experiment_dir="/tmp/captra_test_exp", **{"track_cfg/rot_pool/consensus": True}))
    m_on = Trainer(make_config("1", experiment_dir="/tmp/captra_test_exp", **on)).model
    m_off = Trainer(make_config("1", experiment_dir="/tmp/captra_test_exp")).model
    assert m_on.rot_pool is not None and m_on.net.rot_pool is m_on.rot_pool and m_off.rot_pool is None and m_off.net.rot_pool is None


def test_wrapper_forms_cos_th_in_float64_and_needs_the_device():
    """degrees -> float32(cos(float64 radians)); a CPU tensor is refused: no eager fall-back."""
    import torch
    from captra_amd import _lib, fused
    assert RJ.cos_th_of(60.0) == np.float32(0.5) and RJ.cos_th_of(15.0) == np.float32(np.cos(np.pi / 12))
    with pytest.raises(_lib.CaptraHipError):
        fused.rot_pool_consensus(torch.zeros(1, 3, 8), torch.zeros(1, 8, dtype=torch.int32), torch.eye(3).reshape(1, 1, 3, 3), True, 15.0)


def test_eval_prints_the_rot_pool_table(tmp_path, capsys):
    """A hand-made result pickle with 'rot_pool' -> the table; the same pickle without the key -> nothing new."""
    from captra_amd import eval as ev
    from tests.golden.make_golden_eval import make_inputs
    gc, pc, gt, pred = make_inputs(11 + 4, 4)
    base = {"pred": {"poses": [gt, pred, pred, pred], "corners": [None, pc, pc, pc]}, "gt": {"poses": [gt] * 4, "corners": gc},
            "frame_nums": [["0"], ["1"], ["2"], ["3"]]}
    rec = [None] + [{"inliers": np.array([100, 50, 0, n], np.int32), "count": np.array([100, 200, 0, c], np.int32)}
                    for n, c in ((7, 70), (0, 0), (35, 70))]
    argv = ["--obj_category", "drawers", "--obj_config", "obj_info_sapien.yml"]
    out = {}
    for name, data in (("off", base), ("on", dict(base, rot_pool=rec))):
        d = tmp_path / name / "results" / "data"
        d.mkdir(parents=True)
        with open(d / "inst0_track0.pkl", "wb") as f:
            pickle.dump(data, f)
        ev.main(argv + ["--experiment_dir", str(tmp_path / name)])
        out[name] = capsys.readouterr().out
    assert "rot_pool" not in out["off"] and "consensus" not in out["off"]
    assert out["on"].startswith(out["off"])
    table = out["on"][len(out["off"]):].splitlines()
    assert "track_cfg/rot_pool" in table[0] and len(table) == 5
    assert re.search(r"part 0: frames 3; inlier fraction mean 1\.000 min 1\.000; without members 0$", table[1])
    assert re.search(r"part 1: frames 3; inlier fraction mean 0\.250 min 0\.250; without members 0$", table[2])
    assert re.search(r"part 2: frames 3; inlier fraction -; without members 3 \[1 2 3\]$", table[3])
    assert re.search(r"part 3: frames 3; inlier fraction mean 0\.300 min 0\.100; without members 1 \[2\]$", table[4])


def test_symbol_in_header_binding_and_library():
    """Fails without the feature."""
    from captra_amd import _lib, fused
    assert callable(fused.rot_pool_consensus)
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "captra_hip.h").read_text(), flags=re.S)
    m = re.search(r"int\s+captra_rot_pool_consensus\s*\(([^)]*)\)", text)
    assert m, "captra_rot_pool_consensus is not declared in include/captra_hip.h"
    assert len(m.group(1).split(",")) == len(_lib._SIGNATURES["captra_rot_pool_consensus"])      # (the stream included)
    assert hasattr(_lib.lib(), "captra_rot_pool_consensus")
    # one body: both kernels pool through rp_pool_compose of rot_pool.h, and neither carries a copy of the tail
    for name in ("pose_fit.hip", "rot_consensus.hip"):
        src = (ROOT / "captra_amd" / "csrc" / name).read_text()
        assert "rp_pool_compose(" in src and "k23" not in src, name
    src = (ROOT / "captra_amd" / "csrc" / "rot_consensus.hip").read_text()
    assert "rs_list_members(" in src and "rs_draw(" in src
