// Robust rotation read-out of the tracking step: consensus over RotationNet's per-point votes, per (trajectory, part), on device
// for gfx950.  Semantics: include/captra_hip.h, captra_rot_pool_consensus.
//
// captra_rot_pool_compose (pose_fit.hip) takes the plain mean of the votes of every point labelled with the part; a minority of
// votes that agree with each other (a second surface seen through a detector's mask) drags that mean.  A vote is a complete rotation
// hypothesis already, so the RANSAC here has no solver: H votes are drawn, each is scored by the number of member votes within an
// angle of it, and the first best one's inliers are pooled -- by rp_pool_compose (rot_pool.h), the plain read-out's own pooling
// loop, reduction and tail under the predicate `member && inlier`, so a part whose members all agree gets the plain read-out's bits.
//
// One workgroup of RS_THREADS per (b, p):
//   1. the member list (rs_list_members, pose_ransac.h) -- only the draws need it: rank -> point index;
//   2. thread h < H computes the vote of its drawn member into LDS (H x 9 floats);
//   3. scores: a lane holds the votes of RC_PPL points in registers (N = 4096: every point of the cloud at once, each vote computed
//      once; a larger N takes further rounds of RS_THREADS * RC_PPL points, adding to the same scores), reads a hypothesis from LDS
//      (all lanes the same address: a broadcast) and the wave counts the inliers by __ballot / __popcll; lane j keeps the count of
//      hypothesis h0 + j and adds it to the hypothesis's score in LDS once per 64 hypotheses (integer adds: any order, same sum);
//   4. the first best hypothesis (largest score, then smallest h);
//   5. rp_pool_compose: the first RP_THREADS threads recompute the votes from raw with the plain kernel's stride and re-evaluate the
//      inlier test against `best` -- the same fp32 operations as in 3, so the same answer.
#include "pose_ransac.h"
#include "rot_pool.h"

#include <limits.h>

namespace {

constexpr int RC_PPL = 4;       // points per lane of a scoring round

struct RcLds {
    float hv[RS_MAX_H * 9];
    int score[RS_MAX_H];
    double red[10 * RP_WAVES];
    int wcnt[RS_WAVES];
    int best;
    unsigned short idx[RS_MAX_N];
};

// Is vote v an inlier of hypothesis h?  Separately rounded fp32 operations; a NaN compares false.
// SYM: d = h . v > cos_th;  else tr = ((x_h.x_v) + (y_h.y_v)) + (z_h.z_v) = trace(V_h^T V_v) = 1 + 2 cos(angle) > 1 + 2 cos_th (= thr)
template <bool SYM>
__device__ __forceinline__ bool rc_inlier(const float *h, const float *v, float thr) {
    const float d0 = (h[0] * v[0] + h[1] * v[1]) + h[2] * v[2];
    if constexpr (SYM) {
        return d0 > thr;
    } else {
        const float d1 = (h[3] * v[3] + h[4] * v[4]) + h[5] * v[5];
        const float d2 = (h[6] * v[6] + h[7] * v[7]) + h[8] * v[8];
        return (d0 + d1) + d2 > thr;
    }
}

template <bool SYM>
struct RcInliers {          // the pooling predicate: a member that is an inlier of the winning vote
    float h[9], thr;
    __device__ __forceinline__ bool operator()(bool in, const float *v) const { return in && rc_inlier<SYM>(h, v, thr); }
};

template <bool SYM>
__global__ __launch_bounds__(RS_THREADS) void rot_pool_consensus_kernel(int p, int n, int diag, int b0, int num_hyps, float cos_th,
                                                                        const float *__restrict__ raw, const int *__restrict__ labels,
                                                                        const float *__restrict__ prev_rot,
                                                                        const int *__restrict__ sample_rank, unsigned long long seed,
                                                                        float *__restrict__ rot, float *__restrict__ delta,
                                                                        int *__restrict__ count_out, int *__restrict__ num_inliers,
                                                                        int *__restrict__ best_out) {
    __shared__ RcLds L;
    constexpr int NV = SYM ? 3 : 9;
    const int q = blockIdx.x;
    const int bi = q / p, pi = q % p;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *src = rp_head(raw, q, p, pi, n, SYM ? 1 : 0, diag);
    const int *lab = labels + (size_t)bi * n;
    const float thr = SYM ? cos_th : 1.f + 2.f * cos_th;

    if (tid < RS_MAX_H) L.score[tid] = 0;
    if (tid == 0) L.best = 0;
    // ---- 1. members (ends with a barrier)
    const int count = rs_list_members(lab, pi, n, L.idx, L.wcnt);

    if (count > 0) {        // (uniform over the workgroup: the barriers below are met by all or none)
        // ---- 2. hypothesis h is the vote of member rank r_h
        if (tid < num_hyps) {
            const int h = tid;
            unsigned r;
            if (sample_rank != nullptr) {
                r = (unsigned)sample_rank[(size_t)q * num_hyps + h] % (unsigned)count;
            } else {
                const unsigned long long key = rs_mix(seed + 0x9E3779B97F4A7C15ull);
                r = rs_draw(key, b0 + bi, pi, h, 0) % (unsigned)count;
            }
            float v[9];
            rp_vote(src, n, (int)L.idx[r], SYM ? 1 : 0, v);
#pragma unroll
            for (int i = 0; i < NV; ++i) L.hv[h * 9 + i] = v[i];
        }
        __syncthreads();

        // ---- 3. scores
        for (int base = 0; base < n; base += RS_THREADS * RC_PPL) {
            float v[RC_PPL][9];
            bool have[RC_PPL];
#pragma unroll
            for (int k = 0; k < RC_PPL; ++k) {
                const int e = base + k * RS_THREADS + tid;
                have[k] = e < n && lab[e < n ? e : 0] == pi;
                rp_vote(src, n, e < n ? e : 0, SYM ? 1 : 0, v[k]);
            }
            for (int h0 = 0; h0 < num_hyps; h0 += 64) {
                const int h1 = h0 + 64 < num_hyps ? h0 + 64 : num_hyps;
                int mine = 0;
                for (int h = h0; h < h1; ++h) {
                    float hp[NV];
#pragma unroll
                    for (int i = 0; i < NV; ++i) hp[i] = L.hv[h * 9 + i];
                    int pc = 0;
#pragma unroll
                    for (int k = 0; k < RC_PPL; ++k) pc += __popcll(__ballot(have[k] && rc_inlier<SYM>(hp, v[k], thr)));
                    mine = (lane == h - h0) ? pc : mine;
                }
                if (h0 + lane < h1) atomicAdd(&L.score[h0 + lane], mine);
            }
        }
        __syncthreads();

        // ---- 4. the first best hypothesis (largest score, then smallest h)
        if (wave == 0) {
            const int best = rs_first_best(L.score, num_hyps);
            if (lane == 0) L.best = best;
        }
        __syncthreads();
    }
    const int best = L.best;
    if (tid == 0) {
        if (count_out != nullptr) count_out[q] = count;
        if (num_inliers != nullptr) num_inliers[q] = L.score[best];
        if (best_out != nullptr) best_out[q] = best;
    }

    // ---- 5. the masked mean of the winner's inliers, the frame and prev_rot * dR (count == 0: no point is a member, the slot of
    // `best` is never consulted with a true `in`; zeros keep the predicate's operands defined)
    RcInliers<SYM> pool;
#pragma unroll
    for (int i = 0; i < 9; ++i) pool.h[i] = (count > 0 && i < NV) ? L.hv[best * 9 + i] : 0.f;
    pool.thr = thr;
    rp_pool_compose(q, pi, n, SYM ? 1 : 0, src, lab, prev_rot, rot, delta, L.red, pool);
}

template <bool SYM>
int rot_pool_consensus_launch(int b, int p, int n, int diag_only, int b0, int num_hyps, float cos_th, const float *raw, const int *labels,
                              const float *prev_rot, const int *sample_rank, unsigned long long seed, float *rot, float *delta, int *count,
                              int *num_inliers, int *best, captra_stream_t stream) {
    CAPTRA_LAUNCH(SYM ? "rot_pool_consensus_sym" : "rot_pool_consensus", rot_pool_consensus_kernel<SYM>, dim3(b * p), dim3(RS_THREADS), 0,
                  (hipStream_t)stream, p, n, diag_only, b0, num_hyps, cos_th, raw, labels, prev_rot, sample_rank, seed, rot, delta, count,
                  num_inliers, best);
    return captra_last_error();
}

}  // namespace

extern "C" int captra_rot_pool_consensus(int b, int p, int n, int sym, int diag_only, int b0, int num_hyps, float cos_th, const float *raw,
                                         const int *labels, const float *prev_rot, const int *sample_rank, unsigned long long seed,
                                         float *rot, float *delta, int *count, int *num_inliers, int *best, captra_stream_t stream) {
    if (b < 0 || p < 1 || p > RS_MAX_P || n < 1 || n > RS_MAX_N || num_hyps < 1 || num_hyps > RS_MAX_H) return -1;
    if ((sym != 0 && sym != 1) || (diag_only != 0 && diag_only != 1) || b0 < 0 || b0 > INT_MAX - b) return -1;
    if (!(cos_th > -1.f && cos_th < 1.f)) return -1;       // (a NaN fails both comparisons)
    if (b == 0) return 0;
    return sym ? rot_pool_consensus_launch<true>(b, p, n, diag_only, b0, num_hyps, cos_th, raw, labels, prev_rot, sample_rank, seed, rot,
                                                 delta, count, num_inliers, best, stream)
               : rot_pool_consensus_launch<false>(b, p, n, diag_only, b0, num_hyps, cos_th, raw, labels, prev_rot, sample_rank, seed, rot,
                                                  delta, count, num_inliers, best, stream);
}
