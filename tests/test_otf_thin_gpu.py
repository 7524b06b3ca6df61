"""The re-crop's on-device thinning (captra_amd/csrc/otf_thin.hip: captra_otf_thin; crop.hip: captra_otf_candidates_thin,
captra_otf_finish_thin) called through the C entry points, against tests/otf_thin_judge.py -- integers and fp32 bits, no tolerance.
Every output buffer is prefilled with a sentinel: rows a kernel must not write are asserted untouched."""
import numpy as np
import pytest
import torch

from captra_amd import nocs_otf
from tests import otf_inputs as I, otf_judge as J, otf_thin_judge as TJ

pytestmark = pytest.mark.gpu

SENT = -77


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _counts2(member_counts):
    member_counts = np.asarray(member_counts, np.int32)
    return np.stack([member_counts, np.arange(len(member_counts), dtype=np.int32) + 5000], 1)


def _thin(device, member_counts, cap, num_points, b0, frame, seed, keys=None):
    """captra_otf_thin -> (table (B,T), thinned (B,)); both prefilled with SENT, with a guard row after the last that must keep it."""
    from captra_amd import _lib as L
    B, T = len(member_counts), 5 * num_points
    counts = _dev(_counts2(member_counts), device)
    table = torch.full((B + 1, T), SENT, dtype=torch.int32, device=device)
    thinned = torch.full((B + 1,), SENT, dtype=torch.int32, device=device)
    keys_d = None if keys is None else _dev(np.asarray(keys, np.uint32).view(np.int32), device)
    with torch.cuda.device(device):
        L.call("captra_otf_thin", B, cap, num_points, b0, frame, seed, L.ptr(counts), L.ptr(keys_d), L.ptr(table), L.ptr(thinned))
    table, thinned = table.cpu().numpy(), thinned.cpu().numpy()
    assert (table[B] == SENT).all() and thinned[B] == SENT
    return table[:B], thinned[:B]


def _assert_equals_judge(got, member_counts, cap, num_points, b0, frame, seed, keys=None):
    table, thinned = got
    B, T = len(member_counts), 5 * num_points
    want, flags = TJ.thin(member_counts, cap, num_points, b0, frame, seed, keys, table=np.full((B, T), SENT, np.int32))
    np.testing.assert_array_equal(thinned, flags)
    np.testing.assert_array_equal(table, want)


def test_thin_small_launch_equals_judge(device):
    """(a) T = 40, cap 3000: counts around T, around a pass of the workgroup (1024) and around cap; rows not thinned keep the sentinel."""
    counts = [0, 9, 40, 41, 1023, 1024, 1025, 2999, 3000, 3001]
    got = _thin(device, counts, 3000, 8, 0, 5, 1234)
    assert got[1].tolist() == [0, 0, 0, 1, 1, 1, 1, 1, 1, 0]
    assert (got[0][[0, 1, 2, 9]] == SENT).all()
    _assert_equals_judge(got, counts, 3000, 8, 0, 5, 1234)


def test_thin_full_size_table_equals_judge(device):
    """(b) T = 320, cap 65 536, counts 65 535 and 65 536: 64 passes of the workgroup in every stage of the select."""
    counts = [65535, 65536]
    _assert_equals_judge(_thin(device, counts, 65536, 64, 3, 9, 2 ** 63 + 5), counts, 65536, 64, 3, 9, 2 ** 63 + 5)


def _key_cases(c, T):
    same = np.full(c, 77, np.uint32)
    desc = np.arange(c, 0, -1).astype(np.uint32)
    tie = np.full(c, 5000, np.uint32) + np.arange(c, dtype=np.uint32)
    low = [j for j in range(c) if j not in (20, c - 30)][:T - 1]
    tie[low] = np.arange(T - 1, dtype=np.uint32)
    tie[[20, c - 30]] = 1000
    rng = np.random.default_rng(5)
    few = rng.integers(0, 7, c).astype(np.uint32) * np.uint32(0x01010101)        # seven distinct keys: long runs of ties in every byte
    return {"same": (same, list(range(T))), "descending": (desc, list(range(c - T, c))), "straddle": (tie, sorted(low + [20])),
            "zeros": (np.zeros(c, np.uint32), list(range(T))), "ones": (np.full(c, 0xFFFFFFFF, np.uint32), list(range(T))),
            "few_distinct": (few, None)}


@pytest.mark.parametrize("c", [100, 2500])
def test_thin_given_keys(device, c):
    """(c) keys given: all equal -> 0 .. T-1; descending -> the last T; two equal keys straddling rank T-1 / T -> the lower member;
    keys 0 and 0xFFFFFFFF; a handful of distinct keys.  One launch, one case per row; the keys' rows are `cap` apart."""
    num_points, cap = 8, 3000
    cases = _key_cases(c, 5 * num_points)
    keys = np.full((len(cases), cap), 0xDEADBEEF, np.uint32)
    for i, (k, _) in enumerate(cases.values()):
        keys[i, :c] = k
    counts = [c] * len(cases)
    got = _thin(device, counts, cap, num_points, 0, 0, 0, keys)
    for i, (name, (_, want)) in enumerate(cases.items()):
        if want is not None:
            assert got[0][i].tolist() == want, name
    _assert_equals_judge(got, counts, cap, num_points, 0, 0, 0, keys)


def test_thin_lane_replay_and_frame(device):
    """(d) rows [2, 5) launched with b0 = 2 equal rows 2..4 of the whole launch; the same frame twice gives the same bits, another
    frame another table."""
    counts = [300, 1500, 41, 2999, 777, 1024]
    whole = _thin(device, counts, 3000, 8, 0, 4, 99)
    lane = _thin(device, counts[2:5], 3000, 8, 2, 4, 99)
    np.testing.assert_array_equal(whole[0][2:5], lane[0])
    again = _thin(device, counts, 3000, 8, 0, 4, 99)
    assert whole[0].tobytes() == again[0].tobytes() and whole[1].tobytes() == again[1].tobytes()
    other = _thin(device, counts, 3000, 8, 0, 5, 99)
    assert all(not np.array_equal(whole[0][i], other[0][i]) for i in range(len(counts)))
    _assert_equals_judge(other, counts, 3000, 8, 0, 5, 99)


def test_thin_refuses_bad_arguments(device):
    """(e) -1 and nothing written; b = 0 returns 0 and writes nothing."""
    from captra_amd import _lib as L
    counts = _dev(_counts2([100, 100]), device)
    table = torch.full((2, 40), SENT, dtype=torch.int32, device=device)
    thinned = torch.full((2,), SENT, dtype=torch.int32, device=device)
    fn = L.lib().captra_otf_thin
    imax = 2 ** 31 - 1
    with torch.cuda.device(device):
        st = L.stream_ptr()
        for b, cap, n, b0 in ((-1, 3000, 8, 0), (2, 0, 8, 0), (2, 3000, 0, 0), (2, 3000, 8, -1), (2, 3000, 8, imax - 1), (2, 3000, imax // 5 + 1, 0)):
            assert fn(b, cap, n, b0, 0, 0, L.ptr(counts), None, L.ptr(table), L.ptr(thinned), st) == -1, (b, cap, n, b0)
        assert fn(0, 3000, 8, 0, 0, 0, L.ptr(counts), None, L.ptr(table), L.ptr(thinned), st) == 0
        assert fn(2, 3000, 8, imax - 2, 0, 0, L.ptr(counts), None, L.ptr(table), L.ptr(thinned), st) == 0          # b0 = INT_MAX - b: allowed
        torch.cuda.synchronize()
        assert thinned.cpu().tolist() == [1, 1]
        table.fill_(SENT); thinned.fill_(SENT)
        for b, cap, n, b0 in ((-1, 3000, 8, 0), (2, 0, 8, 0), (2, 3000, 8, -1)):
            assert fn(b, cap, n, b0, 0, 0, L.ptr(counts), None, L.ptr(table), L.ptr(thinned), st) == -1
        torch.cuda.synchronize()
    assert (table.cpu().numpy() == SENT).all() and (thinned.cpu().numpy() == SENT).all()


# ---- captra_otf_candidates_thin / captra_otf_finish_thin -------------------------------------------------------------------------
def _lists_and_readout(device, cap, stride, num_points, member_counts, table, thinned, thin_entry=True, seed=3):
    """The two calls on seeded member tables -> (cand, lens, info, (points_cn, labels, nocs_cn), picks, inputs)."""
    from captra_amd import _lib as L
    B, n = len(member_counts), num_points
    pts, obj = I.member_tables(B, cap, seed)
    p_d, o_d = _dev(pts, device), _dev(obj, device)
    counts_d = _dev(_counts2(member_counts), device)
    cand = torch.full((B + 1, stride, 3), 9.5e9, dtype=torch.float32, device=device)
    lens = torch.full((B + 1,), SENT, dtype=torch.int32, device=device)
    info = torch.tensor([0x7f7f7f7f, -5, 123456, -1, SENT], dtype=torch.int32, device=device)
    table_d, thinned_d = _dev(table, device), _dev(thinned, device)
    extra = (L.ptr(table_d), L.ptr(thinned_d)) if thin_entry else ()
    suffix = "_thin" if thin_entry else ""
    with torch.cuda.device(device):
        L.call("captra_otf_candidates" + suffix, B, cap, stride, n, L.ptr(p_d), L.ptr(counts_d), L.ptr(cand), L.ptr(lens), L.ptr(info), *extra)
    lens_h = lens.cpu().numpy()
    rng = np.random.default_rng([21, cap, stride, n])
    picks = np.stack([rng.integers(0, max(int(lens_h[b]), 1), n) for b in range(B)]).astype(np.int32)
    picks[:, 0], picks[:, -1] = 0, np.maximum(lens_h[:B], 1) - 1
    mean = rng.uniform(-0.3, 0.3, (B, 3)).astype(np.float32)
    rot, trans, scale = I.random_rotations(B, 4), rng.uniform(-0.3, 0.3, (B, 3)) + np.array([0.0, 0.0, -1.0]), rng.uniform(0.2, 0.5, B)
    outs = [torch.full((B + 1, 3, n), 9.5e9, dtype=torch.float32, device=device), torch.full((B + 1, n), SENT, dtype=torch.int64, device=device),
            torch.full((B + 1, 3, n), 9.5e9, dtype=torch.float32, device=device)]
    ins = [_dev(a, device) for a in (picks, mean, rot, trans, scale)]
    with torch.cuda.device(device):
        L.call("captra_otf_finish" + suffix, B, cap, stride, n, L.ptr(p_d), L.ptr(o_d), L.ptr(counts_d), *map(L.ptr, ins), *map(L.ptr, outs), *extra)
    outs = [o.cpu().numpy() for o in outs]
    assert (outs[0][B] == np.float32(9.5e9)).all() and (outs[1][B] == SENT).all() and (outs[2][B] == np.float32(9.5e9)).all()
    cand, info = cand.cpu().numpy(), info.cpu().numpy()
    assert (cand[B] == np.float32(9.5e9)).all() and lens_h[B] == SENT and info[4] == SENT
    return cand[:B], lens_h[:B], info[:4], [o[:B] for o in outs], picks, (pts, obj, mean, rot, trans, scale)


@pytest.mark.parametrize("stride,rare", [(100, False), (80, False), (64, True), (1100, False)], ids=["s100", "s80_is_T", "s64_below_T", "s1100"])
def test_thin_lists_and_readout_equal_judge(device, stride, rare):
    """(f) cand, lens, the info words, points / labels / NOCS for thinned and plain rows of one launch (T = 80, cap 2048): a thinned row
    is rare only at stride < T, where its list is the table's first `stride` entries; counts of 9 and cap + 1 stay rare."""
    cap, n = 2048, 16
    member_counts = [81, 500, 30, 2048, 80, 1000] + ([9, 2049] if rare else [])
    table, thinned = TJ.thin(member_counts, cap, n, 0, 2, 17, table=np.full((len(member_counts), 5 * n), 2 ** 30, np.int32))   # (a plain row's entries: far outside every buffer, never read)
    assert thinned.tolist()[:6] == [1, 1, 0, 1, 0, 1]
    cand, lens, info, outs, picks, (pts, obj, mean, rot, trans, scale) = _lists_and_readout(device, cap, stride, n, member_counts, table, thinned)
    rows = [TJ.candidates(pts[b], member_counts[b], cap, stride, n, table[b] if thinned[b] else None) for b in range(len(member_counts))]
    for b, (j_cand, j_len, _, _, _) in enumerate(rows):
        assert int(lens[b]) == j_len and cand[b].tobytes() == j_cand.tobytes(), b
        assert (0 <= picks[b]).all() and (picks[b] < 5 * n).all()
        want = TJ.finish(pts[b], obj[b], member_counts[b], picks[b], mean[b], rot[b], trans[b], scale[b], stride, cap, table[b] if thinned[b] else None)
        for g, wnt, what in zip(outs, want, ("points_cn", "labels", "nocs_cn")):
            assert g[b].dtype == wnt.dtype and g[b].tobytes() == wnt.tobytes(), (b, what)
    np.testing.assert_array_equal(info, TJ.info_words(rows))
    # a thinned row alone is rare exactly when T outgrows the stride; the plain rows of these launches are rare only through 9 / cap + 1
    assert bool(info[0]) == (rare or any(c > stride and not t for c, t in zip(member_counts, thinned)))
    assert int(info[2]) == int(thinned.sum()) == 4 and int(info[1]) == (cap if rare else 5 * n)      # (rare: the count of cap + 1 reports cap)


@pytest.mark.parametrize("launch", [l for l in I.CANDIDATE_LAUNCHES if l[0] in ("s40_rare", "s1100_plain", "s1100_cap_below_stride_rare")], ids=lambda l: l[0])
def test_thin_entry_points_with_no_row_thinned_equal_the_plain_ones(device, launch):
    """(f) thinned all zero: the plain entry points' outputs on the same buffers, bit for bit (the table is never read: its entries
    would index far outside every buffer)."""
    _, cap, stride, n, member_counts, _ = launch
    B = len(member_counts)
    table, thinned = np.full((B, 5 * n), 2 ** 30, np.int32), np.zeros(B, np.int32)
    a = _lists_and_readout(device, cap, stride, n, member_counts, table, thinned, thin_entry=True)
    b = _lists_and_readout(device, cap, stride, n, member_counts, table, thinned, thin_entry=False)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and a[2][2] == 0
    for x, y in zip(a[3], b[3]):
        assert x.tobytes() == y.tobytes()


def test_thin_chain_crop_thin_candidates_sampler_finish(device):
    """(g) captra_crop_box -> captra_crop_ball -> captra_otf_thin -> captra_otf_candidates_thin -> captra_fps_gather_ragged ->
    captra_otf_finish_thin on the 48 x 64 image with num_points 16 (T = 80), each stage fed the previous kernel's device buffers: every
    sampled point is a judged ball member, and the picks are the CPU oracle's furthest-point sampling of the judge's list."""
    from captra_amd import _lib as L, fused
    from oracle import ops as O
    c = I.chain_inputs()
    want_case = I.chain_case()
    B, cap, n, stride = 3, I.H * I.W, 16, 80
    kk = nocs_otf._intrinsics_on_device(I.K, torch.device(device))
    depth, mask = _dev(c["depth"], device), _dev(c["mask"], device)
    box = torch.empty(B, 4, dtype=torch.int32, device=device)
    ctr = torch.empty(B, 3, dtype=torch.float64, device=device)
    rad = torch.empty(B, dtype=torch.float64, device=device)
    pts = torch.zeros(B, cap, 3, dtype=torch.float64, device=device)
    obj = torch.zeros(B, cap, dtype=torch.uint8, device=device)
    pix = torch.zeros(B, cap, dtype=torch.int32, device=device)
    counts = torch.zeros(B, 2, dtype=torch.int32, device=device)
    table = torch.full((B, 5 * n), SENT, dtype=torch.int32, device=device)
    thinned = torch.full((B,), SENT, dtype=torch.int32, device=device)
    cand = torch.full((B, stride, 3), 9.5e9, dtype=torch.float32, device=device)
    lens = torch.full((B,), SENT, dtype=torch.int32, device=device)
    info = torch.full((4,), SENT, dtype=torch.int32, device=device)
    trans, scale = _dev(c["trans"], device), _dev(c["scale"], device)
    with torch.cuda.device(device):
        L.call("captra_crop_box", B, I.H, I.W, I.CHAIN_FACTOR, L.ptr(trans), L.ptr(scale), kk.data_ptr(), L.ptr(box), L.ptr(ctr), L.ptr(rad))
        L.call("captra_crop_ball", B, I.H, I.W, cap, L.ptr(depth), L.ptr(mask), L.ptr(box), L.ptr(ctr), L.ptr(rad), kk.data_ptr() + 72,
               L.ptr(pts), L.ptr(obj), L.ptr(pix), L.ptr(counts))
        L.call("captra_otf_thin", B, cap, n, 7, 3, 2024, L.ptr(counts), None, L.ptr(table), L.ptr(thinned))
        L.call("captra_otf_candidates_thin", B, cap, stride, n, L.ptr(pts), L.ptr(counts), L.ptr(cand), L.ptr(lens), L.ptr(info), L.ptr(table), L.ptr(thinned))
    res = fused.fps_gather(cand, n, n_per_cloud=lens)
    assert res is not None
    picks = res[0].contiguous()
    ins = [_dev(a, device) for a in (c["mean"], c["rot"], c["gt_trans"], c["gt_scale"])]
    outs = [torch.empty(B, 3, n, dtype=torch.float32, device=device), torch.empty(B, n, dtype=torch.int64, device=device),
            torch.empty(B, 3, n, dtype=torch.float32, device=device)]
    with torch.cuda.device(device):
        L.call("captra_otf_finish_thin", B, cap, stride, n, L.ptr(pts), L.ptr(obj), L.ptr(counts), L.ptr(picks), *map(L.ptr, ins), *map(L.ptr, outs),
               L.ptr(table), L.ptr(thinned))
    picks_h, table_h, thinned_h = picks.cpu().numpy(), table.cpu().numpy(), thinned.cpu().numpy()
    outs = [o.cpu().numpy() for o in outs]
    judged = I.judge_ball(want_case)
    member_counts = [j[3] for j in judged]
    assert any(cnt > 5 * n for cnt in member_counts) and all(10 <= cnt <= cap for cnt in member_counts)
    want_table, want_flags = TJ.thin(member_counts, cap, n, 7, 3, 2024, table=np.full((B, 5 * n), SENT, np.int32))
    np.testing.assert_array_equal(thinned_h, want_flags)
    np.testing.assert_array_equal(table_h, want_table)
    rows = []
    for b, (j_pts, j_obj, _, count, _) in enumerate(judged):
        row = want_table[b] if want_flags[b] else None
        rows.append(TJ.candidates(j_pts, count, cap, stride, n, row))
        j_cand, j_len = rows[-1][:2]
        assert int(lens[b]) == j_len and cand[b].cpu().numpy().tobytes() == j_cand.tobytes(), b
        # the picks: the oracle's furthest-point sampling of the judge's list
        o_idx = O.furthest_point_sample(j_cand[None, :j_len], n)[0]
        np.testing.assert_array_equal(picks_h[b], o_idx)
        want = TJ.finish(j_pts, j_obj, count, picks_h[b], c["mean"][b], c["rot"][b], c["gt_trans"][b], c["gt_scale"][b], stride, cap, row)
        for g, wnt, what in zip(outs, want, ("points_cn", "labels", "nocs_cn")):
            assert g[b].tobytes() == wnt.tobytes(), (b, what)
        # every sampled point is a judged ball member: the member its pick names
        members = (row[picks_h[b]] if row is not None else picks_h[b] % count).astype(np.int64)
        assert (members < count).all()
        assert np.array_equal((j_pts[members].astype(np.float32) - c["mean"][b][None, :]).astype(np.float32), outs[0][b].T), b
    np.testing.assert_array_equal(info.cpu().numpy(), TJ.info_words(rows))
    assert info.cpu().numpy()[0] == 0
