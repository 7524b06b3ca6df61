"""Numpy restatement of the re-crop's on-device thinning (include/captra_hip.h: captra_otf_thin, captra_otf_candidates_thin,
captra_otf_finish_thin; captra_amd/csrc/otf_thin.hip, crop.hip).  uint64 arithmetic with wrap-around, one numpy ufunc per operation; the
lists and the read-out are built on tests/otf_judge.py's functions.  No torch, nothing of the kernels: the kernels are compared with
it bit for bit (tests/test_otf_thin_gpu.py), and tests/test_otf_thin_judge_cpu.py holds the judge itself to the rule's properties."""
from __future__ import annotations

import numpy as np

from tests import otf_judge as J

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_M1, _M2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)
_S30, _S27, _S31, _S32 = np.uint64(30), np.uint64(27), np.uint64(31), np.uint64(32)


def mix(z):
    """splitmix64's finaliser on uint64 (scalars or arrays), products and sums modulo 2^64."""
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> _S30)) * _M1
        z = (z ^ (z >> _S27)) * _M2
    return z ^ (z >> _S31)


def row_key(seed: int, traj: int, frame: int):
    """row = mix(mix(seed + golden) ^ (traj << 32 | frame)); traj = b0 + i."""
    with np.errstate(over="ignore"):
        key = mix(np.uint64(seed % (1 << 64)) + GOLDEN)
    ctr = np.uint64(((int(traj) & 0xFFFFFFFF) << 32) | (int(frame) & 0xFFFFFFFF))
    return mix(key ^ ctr)


def member_keys(seed: int, traj: int, frame: int, count: int) -> np.ndarray:
    """u(j) = mix(row ^ j) >> 32 for j in [0, count): (count,) uint32."""
    j = np.arange(int(count), dtype=np.uint64)
    return (mix(row_key(seed, traj, frame) ^ j) >> _S32).astype(np.uint32)


def select(u, keep: int) -> np.ndarray:
    """The `keep` members with the smallest (u(j), j), in ascending member number: (keep,) int32."""
    u = np.asarray(u, np.uint32)
    j = np.arange(len(u))
    return np.sort(np.lexsort((j, u))[:int(keep)]).astype(np.int32)


def is_thinned(count: int, cap: int, num_points: int) -> bool:
    return 5 * int(num_points) < int(count) <= int(cap)


def thin_row(count: int, cap: int, num_points: int, seed: int, traj: int, frame: int, keys=None):
    """One instance of captra_otf_thin: -> its table row (5 num_points,) int32, or None when the row is not thinned (the kernel then
    writes nothing).  keys: (>= count,) uint32 used as u(j) as they are."""
    if not is_thinned(count, cap, num_points):
        return None
    u = member_keys(seed, traj, frame, count) if keys is None else np.asarray(keys, np.uint32)[:int(count)]
    return select(u, 5 * int(num_points))


def thin(counts, cap: int, num_points: int, b0: int, frame: int, seed: int, keys=None, table=None):
    """captra_otf_thin on a launch of len(counts) rows: -> (table (B, T) int32 -- `table` (what the buffer held) with the thinned rows
    replaced --, thinned (B,) int32)."""
    counts = np.asarray(counts).reshape(-1)
    B, T = len(counts), 5 * int(num_points)
    out = np.zeros((B, T), np.int32) if table is None else np.array(table, np.int32).reshape(B, T)
    flags = np.zeros(B, np.int32)
    for i in range(B):
        row = thin_row(int(counts[i]), cap, num_points, seed, int(b0) + i, frame, None if keys is None else np.asarray(keys)[i])
        if row is not None:
            out[i], flags[i] = row, 1
    return out, flags


def candidates(pts, count, cap, stride, num_points, table_row=None):
    """One instance of captra_otf_candidates_thin: table_row None (thinned[i] == 0) -> otf_judge.candidates plus 0; else the list is
    members table_row[0 .. min(T, stride)), zeros beyond, rare only when T > stride, longest = T.  -> (cand, len, rare, longest, thinned)."""
    if table_row is None:
        return J.candidates(pts, count, cap, stride, num_points) + (0,)
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    T = 5 * int(num_points)
    keep = min(T, int(stride))
    cand = np.zeros((int(stride), 3), np.float32)
    cand[:keep] = pts[np.asarray(table_row, np.int64)[:keep]].astype(np.float32)
    return cand, keep, T > int(stride), T, 1


def info_words(rows):
    """The launch's info word from candidates()' results of its rows: [any rare, longest list, thinned rows, 0]."""
    return np.array([int(any(r[2] for r in rows)), max([r[3] for r in rows] + [0]), sum(r[4] for r in rows), 0], np.int32)


def finish(pts, obj, count, picks, mean, rot, trans, scale, stride, cap=None, table_row=None):
    """One instance of captra_otf_finish_thin: a pick p of a thinned row is member table_row[p]; the rest is otf_judge.finish (a row
    of table_row[picks] as picks, with the count and the stride out of the way, reads exactly those members)."""
    if table_row is None:
        return J.finish(pts, obj, count, picks, mean, rot, trans, scale, stride, cap)
    rows = len(np.asarray(pts).reshape(-1, 3))
    members = np.asarray(table_row, np.int64)[np.asarray(picks, np.int64).reshape(-1)]
    return J.finish(pts, obj, rows, members, mean, rot, trans, scale, rows, rows)
