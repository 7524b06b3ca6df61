// Thinning of an over-long candidate list of the on-the-fly re-crop on the device, for gfx950 (include/captra_hip.h: captra_otf_thin).
// The reference thins a list of more than T = 5 num_points ball members with numpy.random.permutation (nocs_data_process.py:92-109,
// data_utils.py:138-157): MT19937 behind a sequential Fisher-Yates shuffle, which has no parallel form -- so the host draws it and a
// thinned instance is a rare-path instance of the sync-free loop (csrc/crop.hip, otf_candidates_kernel).  This is the opt-in rule that
// needs no host: member j of trajectory b0 + i at frame f carries the 32-bit key
//     u(j) = mix(mix(mix(seed + 0x9E3779B97F4A7C15) ^ ((b0 + i) << 32 | f)) ^ j) >> 32        (mix = rs_mix, csrc/pose_ransac.h)
// and the T members with the smallest (u(j), j) are kept, written in ASCENDING member number (row-major pixel order, as every
// unthinned list is).  A pure function of (seed, trajectory, frame, member, count): the same in a lane and in the whole batch, the
// same in a replay.
//
// One workgroup of 1024 per trajectory; it leaves at once when its row is not thinned.  A 65 536-entry key table does not fit LDS and
// a full sort is not needed: the keys are RECOMPUTED in every pass (one 64-bit mix), the T-th smallest key is found by a radix select
// -- four passes over the members, each a 256-bin LDS histogram of the next 8 key bits of the members that share the prefix found so
// far -- and one ordered compaction (wave ballot + LDS wave offsets, as crop_ball_kernel) writes the members whose key is below the
// threshold plus the first (T - those) whose key equals it.
#include "common.h"
#include "pose_ransac.h"

#include <limits.h>

namespace {

constexpr int TH_T = 1024;
constexpr int TH_WAVES = TH_T / 64;

__global__ __launch_bounds__(TH_T) void otf_thin_kernel(int cap, int t_keep, int b0, unsigned frame, unsigned long long seed,
                                                        const int *__restrict__ counts, const unsigned *__restrict__ keys_all,
                                                        int *__restrict__ table_all, int *__restrict__ thinned) {
    __shared__ int hist[256];
    __shared__ int eq_tot[TH_WAVES], sel_tot[TH_WAVES];
    __shared__ unsigned sh_bin;
    __shared__ int sh_rank;
    const int i = blockIdx.x;
    const int c = counts[i * 2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (!(c > t_keep && c <= cap)) {                            // (uniform over the workgroup: no barrier is skipped by a part of it)
        if (tid == 0) thinned[i] = 0;
        return;
    }
    const unsigned *keys = keys_all != nullptr ? keys_all + (size_t)i * cap : nullptr;
    const unsigned long long key = rs_mix(seed + 0x9E3779B97F4A7C15ull);
    const unsigned long long row = rs_mix(key ^ (((unsigned long long)(unsigned)(b0 + i) << 32) | (unsigned long long)frame));
    auto u_of = [&](int j) -> unsigned { return keys != nullptr ? keys[j] : (unsigned)(rs_mix(row ^ (unsigned long long)(unsigned)j) >> 32); };

    // ---- radix select: the key of rank t_keep - 1 (0-based) among the c members, most significant byte first
    unsigned prefix = 0u, known = 0u;                           // the threshold's bits found so far / which bits those are
    int rank = t_keep - 1;                                      // rank of the threshold among the members that share `prefix`
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        for (unsigned j = tid; j < (unsigned)c; j += TH_T) {          // (unsigned: a count near INT_MAX does not wrap)
            const unsigned u = u_of((int)j);
            if ((u & known) == prefix) atomicAdd(&hist[(u >> shift) & 255u], 1);
        }
        __syncthreads();
        if (wave == 0) {
            // lane l owns bins 4 l .. 4 l + 3; an inclusive scan of the lanes' sums finds the one lane whose bins hold `rank`
            const int h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
            const int sum = (h0 + h1) + (h2 + h3);
            int incl = sum;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int o = __shfl_up(incl, off, 64);
                if (lane >= off) incl += o;
            }
            const int excl = incl - sum;
            if (rank >= excl && rank < incl) {
                int r = rank - excl, bin = 4 * lane;
                if (r >= h0) { r -= h0; ++bin;
                    if (r >= h1) { r -= h1; ++bin;
                        if (r >= h2) { r -= h2; ++bin; } } }
                sh_bin = (unsigned)bin;
                sh_rank = r;
            }
        }
        __syncthreads();
        prefix |= sh_bin << shift;
        known |= 255u << shift;
        rank = sh_rank;
    }
    const unsigned thr = prefix;
    const int need_eq = rank + 1;                               // members with u == thr that are kept: the first need_eq in member order

    // ---- ordered compaction: ascending member number
    int *table = table_all + (size_t)i * t_keep;
    int base = 0, eq_base = 0;
    for (unsigned j0 = 0; j0 < (unsigned)c; j0 += TH_T) {
        const unsigned j = j0 + tid;
        bool less = false, eq = false;
        if (j < (unsigned)c) {
            const unsigned u = u_of((int)j);
            less = u < thr;
            eq = u == thr;
        }
        const unsigned long long below = (1ull << lane) - 1ull;
        const unsigned long long me = __ballot(eq);
        if (lane == 0) eq_tot[wave] = __popcll(me);
        __syncthreads();
        int eq_before = eq_base, eq_all = 0;
#pragma unroll
        for (int w = 0; w < TH_WAVES; ++w) {
            const int e = eq_tot[w];
            eq_before += w < wave ? e : 0;
            eq_all += e;
        }
        const bool sel = less || (eq && eq_before + __popcll(me & below) < need_eq);
        const unsigned long long ms = __ballot(sel);
        if (lane == 0) sel_tot[wave] = __popcll(ms);
        __syncthreads();
        int before = base, all = 0;
#pragma unroll
        for (int w = 0; w < TH_WAVES; ++w) {
            const int e = sel_tot[w];
            before += w < wave ? e : 0;
            all += e;
        }
        if (sel) {
            const int pos = before + __popcll(ms & below);
            if (pos < t_keep) table[pos] = (int)j;
        }
        base += all;
        eq_base += eq_all;
    }
    if (tid == 0) thinned[i] = 1;
}

}  // namespace

extern "C" int captra_otf_thin(int b, int cap, int num_points, int b0, unsigned frame, unsigned long long seed, const int *counts,
                               const unsigned *keys, int *table, int *thinned, captra_stream_t stream) {
    if (b < 0 || cap < 1 || num_points < 1 || b0 < 0 || b0 > INT_MAX - b || num_points > INT_MAX / 5) return -1;
    if (b == 0) return 0;
    CAPTRA_LAUNCH("crop_ball", otf_thin_kernel, dim3(b), dim3(TH_T), 0, (hipStream_t)stream, cap, 5 * num_points, b0, frame, seed, counts,
                  keys, table, thinned);
    return captra_last_error();
}
