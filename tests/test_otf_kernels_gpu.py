"""The re-crop's kernels (captra_amd/csrc/crop.hip: captra_crop_box, captra_crop_ball, captra_crop_ball_det, captra_otf_candidates,
captra_otf_finish) called directly through their C entry points, against the float64 judge of tests/otf_judge.py BIT FOR BIT -- no
tolerance anywhere: the kernels are written operation by operation under -ffp-contract=off.  Inputs: tests/otf_inputs.py, small
images at the sizes where the ordered compaction, the `cap` clamp, the per-instance offsets and the list arithmetic change path.
tests/test_otf_judge_cpu.py pins the judge and asserts that no input has a pixel within rounding of its sphere.  Every output buffer
is prefilled with a sentinel: rows a kernel must not write are asserted untouched."""
import numpy as np
import pytest
import torch

from captra_amd import nocs_otf
from tests import otf_inputs as I, otf_judge as J

pytestmark = pytest.mark.gpu

PTS_SENTINEL, OBJ_SENTINEL, PIX_SENTINEL, CNT_SENTINEL = -7.25e77, 0xEE, -9, -77
BALL_CASES = I.ball_cases()


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _crop_ball(device, case):
    """captra_crop_ball (captra_crop_ball_det where the case carries detections) on a case -> pts (B,cap,3), obj, pix (B,cap), counts (B,2)."""
    from captra_amd import _lib as L
    B, h, w, cap = len(case["depth"]), case["h"], case["w"], case["cap"]
    depth, mask, box = _dev(case["depth"], device), _dev(case["mask"], device), _dev(case["box"], device)
    ctr, rad, kinv = _dev(case["center"], device), _dev(case["radius"], device), _dev(case["kinv"], device)
    pts = torch.full((B, cap, 3), PTS_SENTINEL, dtype=torch.float64, device=device)
    obj = torch.full((B, cap), OBJ_SENTINEL, dtype=torch.uint8, device=device)
    pix = torch.full((B, cap), PIX_SENTINEL, dtype=torch.int32, device=device)
    counts = torch.full((B, 2), CNT_SENTINEL, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        if case["det"] is None:
            L.call("captra_crop_ball", B, h, w, cap, L.ptr(depth), L.ptr(mask), L.ptr(box), L.ptr(ctr), L.ptr(rad), L.ptr(kinv),
                   L.ptr(pts), L.ptr(obj), L.ptr(pix), L.ptr(counts))
        else:
            dm, sel = _dev(case["det"]["masks"], device), _dev(case["det"]["sel"], device)
            L.call("captra_crop_ball_det", B, h, w, cap, case["det"]["ndet"], L.ptr(depth), L.ptr(mask), L.ptr(dm), L.ptr(sel), L.ptr(box),
                   L.ptr(ctr), L.ptr(rad), L.ptr(kinv), L.ptr(pts), L.ptr(obj), L.ptr(pix), L.ptr(counts))
    return pts.cpu().numpy(), obj.cpu().numpy(), pix.cpu().numpy(), counts.cpu().numpy()


def _assert_ball_equals_judge(got, case):
    pts, obj, pix, counts = got
    cap = case["cap"]
    for b, (j_pts, j_obj, j_pix, count, valid) in enumerate(I.judge_ball(case)):
        tag = (case["name"], b)
        assert (int(counts[b, 0]), int(counts[b, 1])) == (count, valid), tag            # the TRUE count, beyond cap as well
        k = min(count, cap)
        assert len(j_pts) == k
        np.testing.assert_array_equal(pix[b, :k], j_pix, err_msg=str(tag))
        np.testing.assert_array_equal(obj[b, :k], j_obj, err_msg=str(tag))
        assert pts[b, :k].tobytes() == j_pts.tobytes(), tag
        # rows at and beyond min(count, cap) -- up to the next instance's first row -- are untouched
        assert (pts[b, k:] == PTS_SENTINEL).all() and (obj[b, k:] == OBJ_SENTINEL).all() and (pix[b, k:] == PIX_SENTINEL).all(), tag


@pytest.mark.parametrize("case", [c for c in BALL_CASES if c["det"] is None], ids=[c["name"] for c in BALL_CASES if c["det"] is None])
def test_crop_ball_equals_judge(device, case):
    """Box totals of 1 .. 3072 pixels around a wave (64) and a pass of the workgroup (1024), every pixel a member / a ball that cuts
    the box / negative depths / no depth at all, empty boxes, tables smaller than the member count, three different instances of
    one launch, and a pixel exactly on the sphere (in) and one double inside it (out)."""
    _assert_ball_equals_judge(_crop_ball(device, case), case)


def test_crop_ball_det_equals_judge(device):
    """sel = -1, 0, ndet - 1 and two indices >= ndet: the selected detection's mask, else the pre-fetched one; everything but obj equals
    the plain kernel's output on the same frames."""
    case = next(c for c in BALL_CASES if c["det"] is not None)
    sel, ndet = case["det"]["sel"], case["det"]["ndet"]
    assert sel.tolist()[:3] == [-1, 0, ndet - 1] and (sel[3:] >= ndet).all()
    got = _crop_ball(device, case)
    _assert_ball_equals_judge(got, case)
    plain = _crop_ball(device, {**case, "det": None})
    for a, b in zip((got[0], got[2], got[3]), (plain[0], plain[2], plain[3])):
        assert a.tobytes() == b.tobytes()
    for b, s in enumerate(sel):
        assert (got[1][b] == plain[1][b]).all() == (not 0 <= s < ndet), b


# ---- captra_crop_box ----------------------------------------------------------------------------------------------------------
def _crop_box(device, h, w, trans, scale, factor, intrinsics):
    from captra_amd import _lib as L
    B = len(scale)
    t_d, s_d = _dev(np.asarray(trans, np.float32), device), _dev(np.asarray(scale, np.float32), device)
    kk = nocs_otf._intrinsics_on_device(intrinsics, torch.device(device))
    box = torch.full((B + 1, 4), CNT_SENTINEL, dtype=torch.int32, device=device)
    ctr = torch.full((B + 1, 3), PTS_SENTINEL, dtype=torch.float64, device=device)
    rad = torch.full((B + 1,), PTS_SENTINEL, dtype=torch.float64, device=device)
    with torch.cuda.device(device):
        L.call("captra_crop_box", B, h, w, float(factor), L.ptr(t_d), L.ptr(s_d), kk.data_ptr(), L.ptr(box), L.ptr(ctr), L.ptr(rad))
    box, ctr, rad = box.cpu().numpy(), ctr.cpu().numpy(), rad.cpu().numpy()
    assert (box[B] == CNT_SENTINEL).all() and (ctr[B] == PTS_SENTINEL).all() and rad[B] == PTS_SENTINEL      # nothing past instance B - 1
    return box[:B], ctr[:B], rad[:B]


@pytest.mark.parametrize("h,w,intrinsics", [(I.H, I.W, I.K), (480, 640, nocs_otf.NOCS_REAL_INTRINSICS)], ids=["48x64", "480x640"])
def test_crop_box_equals_host_projection(device, h, w, intrinsics):
    """== nocs_otf.proj_corners_batch and the float64 casts, bit for bit: poses around the frustum, the radius on the 0.05 floor and
    one fp32 step either side of it, scales of -0.0 / 0 / 1e-30, balls a millimetre from the camera plane, across it and behind the
    camera.  Every projected value is far inside int32 (asserted on the host values), so numpy's truncation is the kernel's."""
    saw = set()
    for trans, scale, factor in I.box_poses(h, w):
        assert (I.plane_gap(trans, scale, factor) >= 1e-3).all() and I.projected_extent(trans, scale, factor, intrinsics) < 2.0 ** 30
        box, ctr, rad = _crop_box(device, h, w, trans, scale, factor, intrinsics)
        c64, r_in = trans.astype(np.float64), np.float64(factor) * scale.astype(np.float64)
        want = nocs_otf.proj_corners_batch(h, w, c64, r_in, intrinsics).reshape(-1, 4)
        np.testing.assert_array_equal(box, want)
        assert ctr.tobytes() == c64.tobytes() and rad.tobytes() == np.maximum(r_in, 0.05).tobytes()
        saw |= {"floor"} if (r_in == 0.05).any() else set()
        saw |= {"below"} if (r_in < 0.05).any() else set()
        saw |= {"empty"} if ((want[:, 2] < want[:, 0]) | (want[:, 3] < want[:, 1])).any() else set()
        saw |= {"clamped"} if ((want[:, 0] == 0) & (want[:, 1] == 0) & (want[:, 2] == h - 1) & (want[:, 3] == w - 1)).any() else set()
    assert saw == {"floor", "below", "empty", "clamped"}


def test_crop_box_on_the_poses_of_a_lost_track(device):
    """NaN / inf / huge translations and scales, z >= 0, a corner of the cube ON the camera plane: outside the contract (numpy's
    cast of such values is undefined too), so what is asserted is the documented pass-through of centre and radius (a NaN radius
    is 0.05) and the SAFETY property -- every box is empty or inside the image -- and only then captra_crop_ball runs on those boxes
    once and must equal the judge."""
    trans, scale, factor = I.lost_poses()
    B = len(scale)
    box, ctr, rad = _crop_box(device, I.H, I.W, trans, scale, factor, I.K)
    assert ctr.tobytes() == trans.astype(np.float64).tobytes()
    r_in = np.float64(factor) * scale.astype(np.float64)
    with np.errstate(invalid="ignore"):
        want_rad = np.where(r_in > 0.05, r_in, 0.05)
    assert rad.tobytes() == want_rad.tobytes(), (rad, want_rad)
    assert np.isnan(r_in).any() and np.isinf(want_rad).any() and (want_rad > 1e29).any() and np.isnan(ctr).any() and np.isinf(ctr).any()
    empty = (box[:, 2] < box[:, 0]) | (box[:, 3] < box[:, 1])
    inside = (box[:, 0] >= 0) & (box[:, 1] >= 0) & (box[:, 2] <= I.H - 1) & (box[:, 3] <= I.W - 1)
    assert (empty | inside).all(), box[~(empty | inside)]
    depth, mask = I.frame(80, "half")
    case = I.ball_case("lost", [depth] * B, [mask] * B, box, ctr, rad, I.H * I.W)
    _assert_ball_equals_judge(_crop_ball(device, case), case)


# ---- captra_otf_candidates ----------------------------------------------------------------------------------------------------
def _padded_tables(device, pts, obj, slack):
    """The member tables on the device with `slack` poisoned rows after the last instance's (a list arithmetic that left its
    instance's table would read poison -- or the next instance's rows --, never another allocation's memory)."""
    B, cap, _ = pts.shape
    p = torch.full((B * cap + slack, 3), 3.0e33, dtype=torch.float64, device=device)
    o = torch.full((B * cap + slack,), 0x55, dtype=torch.uint8, device=device)
    p[:B * cap] = _dev(pts.reshape(-1, 3), device)
    o[:B * cap] = _dev(obj.reshape(-1), device)
    return p, o


@pytest.mark.parametrize("launch", I.CANDIDATE_LAUNCHES, ids=[l[0] for l in I.CANDIDATE_LAUNCHES])
def test_otf_candidates_equals_judge(device, launch):
    """cand (zeros beyond the list included), lens and the info word (prefilled with garbage: the launcher zeroes it) for member
    counts of 0 .. cap + 1 around the doubling rule, one block in x (stride 40) and two (stride 1100), cap above and BELOW the
    stride: a count beyond the table is a rare row whose list never leaves the table."""
    from captra_amd import _lib as L
    name, cap, stride, num_points, member_counts, any_rare = launch
    B = len(member_counts)
    pts, obj = I.member_tables(B, cap, 1)
    p_d, _ = _padded_tables(device, pts, obj, max(stride, cap) + 8)
    counts = np.stack([np.asarray(member_counts, np.int32), np.arange(B, dtype=np.int32) + 5000], 1)
    cand = torch.full((B + 1, stride, 3), 9.5e9, dtype=torch.float32, device=device)
    lens = torch.full((B + 1,), CNT_SENTINEL, dtype=torch.int32, device=device)
    info = torch.tensor([0x7f7f7f7f, -5, 123456, -1, CNT_SENTINEL], dtype=torch.int32, device=device)
    counts_d = _dev(counts, device)
    with torch.cuda.device(device):
        L.call("captra_otf_candidates", B, cap, stride, num_points, L.ptr(p_d), L.ptr(counts_d), L.ptr(cand), L.ptr(lens), L.ptr(info))
    cand, lens, info = cand.cpu().numpy(), lens.cpu().numpy(), info.cpu().numpy()
    want = [J.candidates(pts[b], member_counts[b], cap, stride, num_points) for b in range(B)]
    for b, (j_cand, j_len, j_rare, j_longest) in enumerate(want):
        assert int(lens[b]) == j_len, (name, b, member_counts[b])
        assert cand[b].tobytes() == j_cand.tobytes(), (name, b, member_counts[b])
    assert any(w[2] for w in want) == any_rare
    assert int(info[0]) == int(any_rare) and int(info[1]) == max(w[3] for w in want), (name, info)
    assert info[2] == 0 and info[3] == 0 and info[4] == CNT_SENTINEL
    assert (cand[B] == np.float32(9.5e9)).all() and lens[B] == CNT_SENTINEL


# ---- captra_otf_finish --------------------------------------------------------------------------------------------------------
def _finish(device, cap, stride, n, p_d, o_d, counts, picks, mean, rot, trans, scale):
    from captra_amd import _lib as L
    B = len(scale)
    points_cn = torch.full((B + 1, 3, n), 9.5e9, dtype=torch.float32, device=device)
    labels = torch.full((B + 1, n), CNT_SENTINEL, dtype=torch.int64, device=device)
    nocs_cn = torch.full((B + 1, 3, n), 9.5e9, dtype=torch.float32, device=device)
    ins = [_dev(a, device) for a in (counts, picks, mean, rot, trans, scale)]          # (held: a temporary's block is reused by the next one)
    with torch.cuda.device(device):
        L.call("captra_otf_finish", B, cap, stride, n, L.ptr(p_d), L.ptr(o_d), *map(L.ptr, ins), L.ptr(points_cn), L.ptr(labels), L.ptr(nocs_cn))
    points_cn, labels, nocs_cn = points_cn.cpu().numpy(), labels.cpu().numpy(), nocs_cn.cpu().numpy()
    assert (points_cn[B] == np.float32(9.5e9)).all() and (labels[B] == CNT_SENTINEL).all() and (nocs_cn[B] == np.float32(9.5e9)).all()
    return points_cn[:B], labels[:B], nocs_cn[:B]


@pytest.mark.parametrize("n", I.FINISH_N)
@pytest.mark.parametrize("table", I.FINISH_TABLES, ids=[t[0] for t in I.FINISH_TABLES])
def test_otf_finish_equals_judge(device, table, n):
    """points - mean (fp32 subtraction), labels and the float64 NOCS product, (B,3,n) layouts with B = 3 different instances, n around
    a block of 256, picks anywhere in [0, stride) (reduced modulo the clamped count) and rows of all 0 / all stride - 1, member counts
    below, at and beyond stride and cap."""
    name, cap, stride, member_counts = table
    pts, obj = I.member_tables(3, cap, 2)
    p_d, o_d = _padded_tables(device, pts, obj, max(stride, cap) + 8)
    counts = np.stack([np.asarray(member_counts, np.int32), np.full(3, 4242, np.int32)], 1)
    for edge_rows in (False, True):
        picks, mean, rot, trans, scale = I.finish_inputs(cap, stride, n, 5, edge_rows)
        got = _finish(device, cap, stride, n, p_d, o_d, counts, picks, mean, rot, trans, scale)
        for b in range(3):
            want = J.finish(pts[b], obj[b], member_counts[b], picks[b], mean[b], rot[b], trans[b], scale[b], stride, cap)
            for g, wnt, what in zip(got, want, ("points_cn", "labels", "nocs_cn")):
                assert g[b].dtype == wnt.dtype and g[b].tobytes() == wnt.tobytes(), (name, n, edge_rows, b, what)
        assert 0 < int((got[1] == 0).sum()) < got[1].size or n == 1


# ---- the chain ----------------------------------------------------------------------------------------------------------------
def test_chain_box_ball_candidates_sampler_finish(device):
    """captra_crop_box -> captra_crop_ball -> captra_otf_candidates -> captra_fps_gather_ragged -> captra_otf_finish on the small image,
    each stage fed the previous kernel's device buffers, against the judge fed the sampler's own picks.  No row is rare."""
    from captra_amd import _lib as L, fused
    c = I.chain_inputs()
    want_case = I.chain_case()
    B, cap, n, stride = 3, I.H * I.W, I.CHAIN_N, I.CHAIN_STRIDE
    kk = nocs_otf._intrinsics_on_device(I.K, torch.device(device))
    depth, mask = _dev(c["depth"], device), _dev(c["mask"], device)
    box = torch.empty(B, 4, dtype=torch.int32, device=device)
    ctr = torch.empty(B, 3, dtype=torch.float64, device=device)
    rad = torch.empty(B, dtype=torch.float64, device=device)
    pts = torch.full((B, cap, 3), PTS_SENTINEL, dtype=torch.float64, device=device)
    obj = torch.full((B, cap), OBJ_SENTINEL, dtype=torch.uint8, device=device)
    pix = torch.full((B, cap), PIX_SENTINEL, dtype=torch.int32, device=device)
    counts = torch.full((B, 2), CNT_SENTINEL, dtype=torch.int32, device=device)
    cand = torch.full((B, stride, 3), 9.5e9, dtype=torch.float32, device=device)
    lens = torch.full((B,), CNT_SENTINEL, dtype=torch.int32, device=device)
    info = torch.full((4,), CNT_SENTINEL, dtype=torch.int32, device=device)
    trans, scale = _dev(c["trans"], device), _dev(c["scale"], device)
    with torch.cuda.device(device):
        L.call("captra_crop_box", B, I.H, I.W, I.CHAIN_FACTOR, L.ptr(trans), L.ptr(scale), kk.data_ptr(), L.ptr(box), L.ptr(ctr), L.ptr(rad))
        L.call("captra_crop_ball", B, I.H, I.W, cap, L.ptr(depth), L.ptr(mask), L.ptr(box), L.ptr(ctr), L.ptr(rad), kk.data_ptr() + 72,
               L.ptr(pts), L.ptr(obj), L.ptr(pix), L.ptr(counts))
        L.call("captra_otf_candidates", B, cap, stride, n, L.ptr(pts), L.ptr(counts), L.ptr(cand), L.ptr(lens), L.ptr(info))
    res = fused.fps_gather(cand, n, n_per_cloud=lens)
    assert res is not None
    picks = res[0].contiguous()
    np.testing.assert_array_equal(box.cpu().numpy(), want_case["box"])
    assert ctr.cpu().numpy().tobytes() == want_case["center"].tobytes() and rad.cpu().numpy().tobytes() == want_case["radius"].tobytes()
    ball = (pts.cpu().numpy(), obj.cpu().numpy(), pix.cpu().numpy(), counts.cpu().numpy())
    _assert_ball_equals_judge(ball, want_case)
    assert info.cpu().numpy().tolist() == [0, max(J.list_length(int(k), n) for k in ball[3][:, 0]), 0, 0]
    picks_h = picks.cpu().numpy()
    got = _finish(device, cap, stride, n, pts, obj, ball[3], picks_h, c["mean"], c["rot"], c["gt_trans"], c["gt_scale"])
    for b, (j_pts, j_obj, _, count, _) in enumerate(I.judge_ball(want_case)):
        j_cand, j_len, j_rare, _ = J.candidates(j_pts, count, cap, stride, n)
        assert not j_rare and int(lens[b]) == j_len and cand[b].cpu().numpy().tobytes() == j_cand.tobytes(), b
        assert (0 <= picks_h[b]).all() and (picks_h[b] < j_len).all() and picks_h[b, 0] == 0
        want = J.finish(j_pts, j_obj, count, picks_h[b], c["mean"][b], c["rot"][b], c["gt_trans"][b], c["gt_scale"][b], stride, cap)
        for g, wnt, what in zip(got, want, ("points_cn", "labels", "nocs_cn")):
            assert g[b].tobytes() == wnt.tobytes(), (b, what)
