"""The held box's judge (tests/box_judge.py) against values worked out by hand: each case of the table is one a deliberate mistake gets
wrong, so the judge the GPU tests compare with is shown to tell the mistakes apart; and the case the option exists for -- a cuboid with
outliers, where the per-frame maximum is set by the outliers and the accumulated quantile is not."""
import numpy as np
import pytest

from tests import box_judge as J


def _one_part(points, n_pad=3):
    """points (M,3) -> labels (1,N), src (1,1,3,N) with n_pad points of another label (coordinates 0.9: they must not count)."""
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    labels = np.concatenate([np.zeros(len(pts), np.int32), np.full(n_pad, 1, np.int32)])[None]
    src = np.concatenate([pts, np.full((n_pad, 3), 0.9, np.float32)]).T[None, None]
    return labels, np.ascontiguousarray(src)


def _preloaded(bins, cells):
    H = np.zeros((1, 1, 3, bins), np.int32)
    for k in range(3):
        for j, v in cells.items():
            H[0, 0, k, j] = v
    return H


# name -> (arguments of judge_batch, the outputs worked out by hand, the mutation that must get it wrong)
def _table():
    t = {}
    # 0.0117 * 64 = 0.7488: bin 0 (truncated), upper edge 1/64; rounding would give bin 1
    labels, src = _one_part([[0.0117, -0.0117, 0.0117]] * 4)
    t["truncate"] = (dict(labels=labels, src=src, hist_in=None, verdict=None, bins=64, radial=False, permille=1000, min_points=4),
                     dict(extent=[1 / 64] * 3, frame=[1 / 64] * 3, added=4, total=4), "round_bin")
    # nine members in bin 0 and one in bin 5, 900 per mille of 10: need = 9, reached in bin 0; need = 10 only in bin 5
    labels, src = _one_part([[0.001, 0.001, 0.001]] * 9 + [[5.5 / 64] * 3])
    t["need"] = (dict(labels=labels, src=src, hist_in=None, verdict=None, bins=64, radial=False, permille=900, min_points=1),
                 dict(extent=[1 / 64] * 3, frame=[1 / 64] * 3, added=10, total=10), "need_off_by_one")
    # a lost frame (verdict 2) of 20 members in bin 40 beside a state of 20 values in bin 3: the state stays, the frame's own read-out is its own
    labels, src = _one_part([[40.5 / 64] * 3] * 20)
    t["lost"] = (dict(labels=labels, src=src, hist_in=_preloaded(64, {3: 20}), verdict=np.array([[2]]), bins=64, radial=False, permille=950,
                      min_points=16),
                 dict(extent=[4 / 64] * 3, frame=[41 / 64] * 3, added=20, total=20, hist={3: 20}), "accumulate_lost")
    # radial: (0.3, 0.4, 0) has r = 0.3 (bin 19 of 64: 19.2), |y| = 0.4 (bin 25: 25.6); with y folded in r would be 0.5 (bin 32)
    labels, src = _one_part([[0.3, 0.4, 0.0]] * 2)
    t["radius"] = (dict(labels=labels, src=src, hist_in=None, verdict=None, bins=64, radial=True, permille=1000, min_points=1),
                   dict(extent=[20 / 64, 26 / 64, 20 / 64], frame=[20 / 64, 26 / 64, 20 / 64], added=2, total=2), "radius_with_y")
    # 3 000 000 held values in bin 10: T * 950 = 2.85e9 > 2^31 -- a 32-bit product turns negative and the first bin "reaches" it
    labels, src = _one_part(np.zeros((0, 3)))
    t["wide_product"] = (dict(labels=labels, src=src, hist_in=_preloaded(64, {10: 3_000_000}), verdict=None, bins=64, radial=False,
                              permille=950, min_points=16),
                         dict(extent=[11 / 64] * 3, frame=[0.0] * 3, added=0, total=3_000_000, hist={10: 3_000_000}), "product_32bit")
    return t


TABLE = _table()


def _matches(out, want, bins):
    ok = (np.array_equal(out["extent"][0, 0], np.asarray(want["extent"], np.float32))
          and np.array_equal(out["frame"][0, 0], np.asarray(want["frame"], np.float32))
          and int(out["added"][0, 0]) == want["added"] and int(out["total"][0, 0]) == want["total"])
    if "hist" in want:
        ok = ok and np.array_equal(out["hist"], _preloaded(bins, want["hist"]))
    return ok


@pytest.mark.parametrize("name", sorted(TABLE))
def test_judge_gives_the_hand_computed_values(name):
    args, want, _ = TABLE[name]
    out = J.judge_batch(**args)
    assert _matches(out, want, args["bins"]), (name, out["extent"], out["frame"], out["added"], out["total"])
    assert out["hist"].dtype == np.int32 and out["extent"].dtype == np.float32 and out["frame"].dtype == np.float32


@pytest.mark.parametrize("name", sorted(TABLE))
def test_table_catches_each_mutation(name):
    args, want, mutation = TABLE[name]
    assert mutation in J.MUTATIONS
    wrong = J.judge_batch(**args, mutate=mutation)
    assert not _matches(wrong, want, args["bins"]), (name, mutation)
    # (every mistake the judge can be asked to make has its case)
    assert {m for _, _, m in TABLE.values()} == set(J.MUTATIONS)


def test_pieces_agree_with_the_batch_form():
    rng = np.random.default_rng(5)
    labels = rng.integers(-1, 3, size=(2, 200)).astype(np.int32)
    src = rng.uniform(-1.2, 1.2, size=(2, 2, 3, 200)).astype(np.float32)
    src[0, 0, 1, 5] = np.nan
    src[1, 1, 2, 7] = np.inf
    hist_in = rng.integers(-3, 50, size=(2, 2, 3, 128)).astype(np.int32)
    verdict = np.array([[0, 1], [2, 3]], np.int32)
    out = J.judge_batch(labels, src, hist_in, verdict, 128, False, 900, 16)
    for b in range(2):
        for q in range(2):
            F, added = J.frame_hist(labels[b], src[b, q], q, 128, False)
            assert added == int(((labels[b] == q) & np.isfinite(src[b, q]).all(0)).sum()) == int(F[0].sum()) == int(F[2].sum())
            H = J.accumulate(hist_in[b, q], F, verdict[b, q])
            assert (H == np.maximum(hist_in[b, q], 0) + (F if verdict[b, q] in (0, 3) else 0)).all()
            np.testing.assert_array_equal(out["hist"][b, q], H)
            np.testing.assert_array_equal(out["extent"][b, q], J.read_out(H, 900, 16)[0])
    assert J.accumulate(np.full((3, 64), J.INT_MAX - 10), np.full((3, 64), 25)).max() == J.INT_MAX


# ---- the cuboid with outliers --------------------------------------------------------------------------------------------------
def cuboid_frame(rng, half, n, sigma, outliers):
    """n points on the surface of the cuboid [-half, half] -- a face drawn uniformly among the six, a point uniformly on it --, Gaussian
    noise of sigma on every coordinate, the first round(outliers n) points replaced by uniform draws from the NOCS cube [-0.5, 0.5]^3."""
    half = np.asarray(half, np.float64)
    face = rng.integers(0, 3, size=n)
    pts = rng.uniform(-1, 1, size=(n, 3)) * half
    pts[np.arange(n), face] = rng.choice([-1.0, 1.0], size=n) * half[face]
    pts += rng.normal(0, sigma, size=(n, 3))
    k = int(round(outliers * n))
    pts[:k] = rng.uniform(-0.5, 0.5, size=(k, 3))
    return pts.astype(np.float32)


def test_cuboid_with_outliers_quantile_against_maximum():
    """Half-extents (0.11, 0.34, 0.11), 1300 points per frame, 4 mm noise, 2 % outliers, 0.95 quantile of 128 bins: the held extent is
    the truth's bin edge from frame 1 to frame 15 -- 15/128 for 0.11 (bin 14) and, the noise on the faces being half a bin wide,
    45/128 for 0.34 (0.34 + 1.1 sigma falls into bin 44) --, while every frame's maximum is set by the outliers."""
    half, bins = (0.11, 0.34, 0.11), 128
    rng = np.random.default_rng(1)
    labels = np.zeros(1300, np.int32)
    H = None
    for frame in range(1, 16):
        pts = cuboid_frame(rng, half, 1300, 0.004, 0.02)
        F, added = J.frame_hist(labels, pts.T, 0, bins, False)
        assert added == 1300
        H = J.accumulate(H, F)
        extent, total = J.read_out(H, 950, 16)
        assert total == 1300 * frame
        np.testing.assert_array_equal(extent, np.array([15, 45, 15], np.float32) / np.float32(bins), err_msg=f"frame {frame}")
        # the truth rounded up to its bin's edge, or one bin further where the noise carries the quantile across an edge
        edge = (np.floor(np.asarray(half) * bins) + 1) / bins
        assert ((extent >= edge - 1e-9) & (extent <= edge + 1 / bins + 1e-9)).all()
        assert (np.abs(pts).max(axis=0) > 0.4).all(), (frame, np.abs(pts).max(axis=0))
