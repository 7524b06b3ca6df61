"""The judge of captra_depth_support_filter (include/captra_hip.h): the rule restated in numpy int64 with shifted arrays -- one whole-image
comparison per offset of the window, not the kernel's loop over a pixel's neighbours --, the deliberately wrong variants of it that the
case table must tell from it, and that table: the shapes, windows, supports and contents the GPU test holds the kernel to.

The rule: a pixel with d > 0 has tol = abs_mm + floor(d rel_permille / 1000); the OTHER pixels of the (2 window + 1)^2 square around it
that lie inside its own image are its neighbours; a neighbour d' supports it when d' > 0 and |d' - d| <= tol; with fewer than min_support
supporters the pixel becomes 0; d <= 0 is copied; removed[i] counts the pixels of image i set to 0."""
import numpy as np

INT_MAX = 2 ** 31 - 1
MUTANTS = ("self", "strict", "wrap_row", "wrap_image", "halo_valid", "tol_neighbour")


def judge(depth, window, abs_mm, rel_permille, min_support, mutant=None):
    """-> (out int32 of depth's shape, removed int32 (B,)); depth (B,H,W) or (H,W) integers.  `mutant`: one of MUTANTS, a wrong rule."""
    assert mutant is None or mutant in MUTANTS, mutant
    d = np.asarray(depth).astype(np.int64)
    if d.ndim == 2:
        out, removed = judge(d[None], window, abs_mm, rel_permille, min_support, mutant)
        return out[0], removed
    B, H, W = d.shape
    if mutant == "wrap_image":
        # the batch as ONE tall image: the rows below an image are the next image's
        out, _ = judge(d.reshape(1, B * H, W), window, abs_mm, rel_permille, min_support)
        out = out.reshape(B, H, W)
        return out, ((d > 0) & (out == 0)).sum(axis=(1, 2)).astype(np.int32)
    k = int(window)
    tol = abs_mm + (d * rel_permille) // 1000
    support = np.zeros(d.shape, np.int64)
    if mutant == "wrap_row":
        # every image as one long row: a column past the row's end is the next row's first
        pad = k * W + k
        flat = np.zeros((B, H * W + 2 * pad), np.int64)
        flat[:, pad:pad + H * W] = d.reshape(B, H * W)
        shifted = lambda dy, dx: flat[:, pad + dy * W + dx: pad + dy * W + dx + H * W].reshape(B, H, W)
        inside = None
    else:
        padded = np.zeros((B, H + 2 * k, W + 2 * k), np.int64)
        padded[:, k:k + H, k:k + W] = d
        shifted = lambda dy, dx: padded[:, k + dy:k + dy + H, k + dx:k + dx + W]
        inside = np.zeros((B, H + 2 * k, W + 2 * k), bool)
        inside[:, k:k + H, k:k + W] = True
    for dy in range(-k, k + 1):
        for dx in range(-k, k + 1):
            if dy == 0 and dx == 0 and mutant != "self":
                continue
            nb = shifted(dy, dx)
            t = abs_mm + (nb * rel_permille) // 1000 if mutant == "tol_neighbour" else tol
            diff = np.abs(nb - d)
            ok = (nb > 0) & ((diff < t) if mutant == "strict" else (diff <= t))
            if mutant == "halo_valid":
                ok = ok | ~inside[:, k + dy:k + dy + H, k + dx:k + dx + W]
            support += ok
    drop = (d > 0) & (support < min_support)
    return np.where(drop, 0, d).astype(np.int32), drop.sum(axis=(1, 2)).astype(np.int32)


# ---- the case table ------------------------------------------------------------------------------------------------------
SMALL_SHAPES = ((1, 1, 1), (1, 1, 70), (1, 70, 1), (3, 17, 65), (2, 33, 130))      # straddle the 16 x 64 tile and its halo
LARGE_SHAPE = (2, 480, 640)
WINDOWS = (1, 2, 3)


def supports(window):
    """min_support at 1, at a middle value and at its maximum."""
    most = (2 * window + 1) ** 2 - 1
    return (1, most // 2, most)


def _isolated(shape):
    """A lone pixel at each image corner and on both sides of each boundary of the 16 x 64 tiles (all far enough apart to be alone
    in a window of 3 only where the shape allows: the judge decides, not this function)."""
    B, H, W = shape
    d = np.zeros(shape, np.int32)
    rows = sorted({r for r in (0, H - 1, 15, 16, 31, 32) if 0 <= r < H})
    cols = sorted({c for c in (0, W - 1, 63, 64, 127, 128) if 0 <= c < W})
    for i, r in enumerate(rows):
        for j, c in enumerate(cols):
            if (i + j) % 2 == 0 or H == 1 or W == 1:
                d[:, r, c] = 1000 + 37 * (i + j)
    return d


def _step(shape, abs_mm):
    """Columns in threes: 1000, 1000 + tol (a supporter, exactly at the bound), 1000 + tol + 1 (none); every fourth row a step higher."""
    B, H, W = shape
    r, c = np.mgrid[0:H, 0:W]
    d = 1000 + np.choose(c % 3, [0, abs_mm, abs_mm + 1]) + np.where(r % 4 == 3, abs_mm, 0)
    return np.broadcast_to(d, shape).astype(np.int32)


def _extremes(shape, abs_mm):
    """The extreme values of the hand-worked table, laid through the image in an order that puts each next to each: the largest int
    beside 1, negatives and zeros, and around the floor of d rel_permille / 1000 at d = 2000 (rel_permille = 1: 1999 -> tol = abs_mm + 1,
    2000 -> abs_mm + 2; 2000 beside 1998 - abs_mm is supported by the pixel's own tol, not by the neighbour's)."""
    vals = np.array([INT_MAX, 1, -5, 0, 1999, 2000 + abs_mm, 2000, 1998 - abs_mm, INT_MAX, INT_MAX - 1, -INT_MAX - 1, 2001 + abs_mm,
                     1999, 1, 2, INT_MAX - abs_mm - 1, 2000, 1998 - abs_mm, 2000], np.int64)
    return np.resize(vals, shape).astype(np.int32)


def contents(shape, seed=0):
    """-> list of (name, depth (B,H,W) int32, abs_mm, rel_permille)."""
    B, H, W = shape
    rng = np.random.default_rng([seed, B, H, W])
    r, c = np.mgrid[0:H, 0:W]
    out = [("constant", np.full(shape, 1000, np.int32), 0, 0),
           ("holes", np.zeros(shape, np.int32), 5, 0),
           ("checkerboard", np.broadcast_to(np.where((r + c) % 2 == 0, 1000, 0), shape).astype(np.int32), 0, 0),
           ("isolated", _isolated(shape), 10, 0),
           ("step", _step(shape, 7), 7, 0),
           ("extremes_floor", _extremes(shape, 3), 3, 1),
           ("extremes_wide", _extremes(shape, 3), INT_MAX, 1000),             # tol up to 2^32 - 2: the 64-bit sum
           ("extremes_tight", _extremes(shape, 0), 0, 0)]
    u16 = rng.integers(0, 65536, size=shape).astype(np.int32)
    u16[rng.random(shape) < 0.2] = 0
    out.append(("random_u16", u16, 12000, 200))           # tol about a quarter of the range: the middle min_support decides
    ramp = (1200 + 3 * r + 2 * c + rng.integers(-6, 7, size=shape)).astype(np.int32)
    ramp[rng.random(shape) < 0.2] = 0
    out.append(("random_ramp", ramp, 8, 2))
    # image 0: holes above, a plane below; every odd image is its neighbour's mirror (plane above): a plane's last rows lie against the
    # next image's first rows of plane, which must not support them
    half = np.where(r >= H // 2, 1500, 0).astype(np.int32)
    out.append(("mirror", np.stack([half if i % 2 == 0 else half[::-1, ::-1] for i in range(B)]), 0, 0))
    return out


def small_cases():
    """Every (shape, window, min_support, content) of the small shapes -> (name, depth, window, abs_mm, rel_permille, min_support)."""
    for shape in SMALL_SHAPES:
        for name, depth, abs_mm, rel in contents(shape):
            for window in WINDOWS:
                for ms in supports(window):
                    yield f"{name}{shape} w{window} s{ms}", depth, window, abs_mm, rel, ms
