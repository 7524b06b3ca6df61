"""The held box's judge: captra_part_box_hist (include/captra_hip.h) restated in numpy -- Python integers for the counts, float32 for
the three operations of the radius -- so that every output of the kernel is compared bit for bit.  `mutate` names a deliberate
mistake; tests/test_box_judge_cpu.py shows that the judge's table tells each of them from the truth."""
import numpy as np

BINS = (64, 128, 256, 512)
INT_MAX = 2 ** 31 - 1
MUTATIONS = ("round_bin", "need_off_by_one", "accumulate_lost", "radius_with_y", "product_32bit")
ACCUMULATING = (0, 3)            # GUARD_VERDICTS: ok, recovered


def _check(bins, permille, min_points):
    assert bins in BINS and 500 <= permille <= 1000 and min_points >= 1, (bins, permille, min_points)


def axis_values(xyz, radial, mutate=None):
    """xyz (M,3) float32, all finite -> (M,3) float32: |x|, |y|, |z|, or with radial r, |y|, r with r = sqrt(x x + z z) in float32,
    one rounding per operation."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    a = np.abs(xyz)
    if radial:
        with np.errstate(over="ignore", invalid="ignore"):
            x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
            s = np.float32(x * x) + np.float32(z * z)
            if mutate == "radius_with_y":
                s = np.float32(s) + np.float32(y * y)
            r = np.sqrt(np.float32(s)).astype(np.float32)
        a = np.stack([r, a[:, 1], r], axis=1)
    return a.astype(np.float32)


def bin_of(a, bins, mutate=None):
    """The bin of values a >= 0 (float32; Inf allowed): bins - 1 when a >= 1 or not finite, else (int)(a * bins), which is exact."""
    a = np.asarray(a, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        prod = (a * np.float32(bins)).astype(np.float32)
        inside = np.isfinite(a) & (a < 1)
        j = np.where(inside, prod, 0).astype(np.float64)
    j = np.floor(j + 0.5) if mutate == "round_bin" else np.floor(j)
    j = np.minimum(j, bins - 1).astype(np.int64)
    return np.where(inside, j, bins - 1)


def frame_hist(labels, src, q, bins, radial, mutate=None):
    """labels (N,) ints, src (3,N) float32 = part q's NOCS map -> (F (3,bins) int64, the member count)."""
    labels, src = np.asarray(labels).reshape(-1), np.asarray(src, np.float32).reshape(3, -1)
    member = (labels == q) & np.isfinite(src).all(axis=0)
    a = axis_values(src[:, member].T, radial, mutate)
    F = np.zeros((3, bins), np.int64)
    for k in range(3):
        np.add.at(F[k], bin_of(a[:, k], bins, mutate), 1)
    return F, int(member.sum())


def accumulate(hist_in, F, verdict=None, mutate=None):
    """hist_in (3,bins) ints or None, F (3,bins), verdict an int code or None -> hist_out (3,bins) int64 in [0, 2^31 - 1]."""
    H = np.zeros_like(F, dtype=np.int64) if hist_in is None else np.maximum(np.asarray(hist_in, np.int64), 0)
    counts = verdict is None or int(verdict) in ACCUMULATING or (mutate == "accumulate_lost" and int(verdict) == 2)
    return np.minimum(H + (np.asarray(F, np.int64) if counts else 0), INT_MAX)


def read_out(H, permille, min_points, mutate=None):
    """H (3,bins) non-negative ints -> (extent (3,) float32, T of axis 0 clamped to 2^31 - 1)."""
    bins = H.shape[1]
    ext = np.zeros(3, np.float32)
    totals = []
    for k in range(3):
        row = [int(v) for v in H[k]]
        T = sum(row)
        totals.append(T)
        if T < min_points:
            continue
        prod = T * permille
        if mutate == "product_32bit":
            prod = ((prod + 2 ** 31) % 2 ** 32) - 2 ** 31             # what a 32-bit signed product keeps
        need = (prod + 999) // 1000 + (1 if mutate == "need_off_by_one" else 0)
        cum, j = 0, 0
        for j, v in enumerate(row):
            cum += v
            if cum >= need:
                break
        ext[k] = np.float32(j + 1) / np.float32(bins)
    return ext, min(totals[0], INT_MAX)


def judge_batch(labels, src, hist_in, verdict, bins, radial, permille, min_points, mutate=None):
    """labels (B,N), src (B,P,3,N), hist_in (B,P,3,bins) or None, verdict (B,P) or None
    -> {'hist' (B,P,3,bins) int32, 'extent', 'frame' (B,P,3) float32, 'added', 'total' (B,P) int32}."""
    _check(bins, permille, min_points)
    labels, src = np.asarray(labels), np.asarray(src, np.float32)
    B, P = src.shape[:2]
    out = {"hist": np.zeros((B, P, 3, bins), np.int32), "extent": np.zeros((B, P, 3), np.float32), "frame": np.zeros((B, P, 3), np.float32),
           "added": np.zeros((B, P), np.int32), "total": np.zeros((B, P), np.int32)}
    for b in range(B):
        for q in range(P):
            F, added = frame_hist(labels[b], src[b, q], q, bins, radial, mutate)
            H = accumulate(None if hist_in is None else hist_in[b, q], F, None if verdict is None else verdict[b, q], mutate)
            out["hist"][b, q] = H
            out["extent"][b, q], out["total"][b, q] = read_out(H, permille, min_points, mutate)
            out["frame"][b, q], _ = read_out(F, permille, min_points, mutate)
            out["added"][b, q] = added
    return out
