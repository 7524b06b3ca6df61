// Holding a track's size: the running mean of a rigid part's NOCS scale as frame-to-frame state, and the step's translation fitted
// with that scale GIVEN, per (trajectory, part), on device for gfx950.  Semantics: include/captra_hip.h, captra_part_fit_st_size.
//
// One workgroup of RS_THREADS per (b, p) on the skeleton of pose_ransac.h (member list in LDS, staged coordinates, counter-based
// draws with b0 + b in the key, the two inlier tests, first best, fixed-order double sums).  Robust mode computes the step's free
// fit itself -- rs_fit with RsGivenRot, exactly as part_fit_st_ransac_kernel (pose_st_ransac.hip) calls it, so the free outputs
// are that kernel's bits --, thread 0 takes the decision on the size state and broadcasts it through LDS, a workgroup that is not
// held leaves there, a held one runs rs_fit a second time on the same staged members with RsGivenRotScale: the launch REPLACES the
// step's captra_part_fit_st_ransac.  Plain mode is handed the one-pass fit's outputs and adds the decision and, where held, the
// given-scale estimator over all members (the refit's sums with every member counted as an inlier).
#include "pose_ransac.h"

#include <limits.h>

namespace {

// the size state's options, as the entry point checked them (max_frames / reset_after: 0 = not given)
struct SzOpts {
    int min_frames, max_frames, reset_after;
    float max_ratio;
};

// what thread 0 decided, for the whole workgroup
struct SzDecision {
    int held;
    float mean;
};

// The solver on ALL `count` members: the refit of rs_fit (pose_ransac.h) with every member counted as an inlier -- the same two
// passes, the same wg_sum order.  Every thread calls it; thread 0 gets tr (fp32) and whether it is finite.
template <class Solver>
__device__ __forceinline__ bool sz_fit_all(const RsMembers &mem, int count, RsLds &L, const Solver &solve, float ft[3]) {
    const int tid = threadIdx.x;
    double r1[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int m = tid; m < count; m += RS_THREADS) {
        float s[3], t[3];
        mem.load(m, s, t);
        r1[0] += 1.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            r1[1 + a] += (double)s[a];
            r1[4 + a] += (double)t[a];
        }
    }
    wg_sum<WG_SUM_SERIAL, RS_WAVES>(r1, L.red);
    const double cnt = r1[0];
    const double sb[3] = {r1[1] / cnt, r1[2] / cnt, r1[3] / cnt}, tb[3] = {r1[4] / cnt, r1[5] / cnt, r1[6] / cnt};
    double r2[15];
#pragma unroll
    for (int i = 0; i < 15; ++i) r2[i] = 0.0;
    for (int m = tid; m < count; m += RS_THREADS) {
        float s[3], t[3];
        mem.load(m, s, t);
        double sc[3], tc[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            sc[a] = (double)s[a] - sb[a];
            tc[a] = (double)t[a] - tb[a];
        }
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int c = 0; c < 3; ++c) r2[a * 3 + c] += tc[a] * sc[c];
        r2[9] += sc[0] * sc[0]; r2[10] += sc[0] * sc[1]; r2[11] += sc[0] * sc[2];
        r2[12] += sc[1] * sc[1]; r2[13] += sc[1] * sc[2]; r2[14] += sc[2] * sc[2];
    }
    wg_sum<WG_SUM_SERIAL, RS_WAVES>(r2, L.red);
    bool ok = false;
    if (tid == 0) {
        double R[9], sca, tr[3];
        solve(r2, r2 + 9, sb, tb, R, &sca, tr);
        for (int a = 0; a < 3; ++a) ft[a] = (float)tr[a];
        ok = isfinite((ft[0] + ft[1]) + ft[2]);
    }
    return ok;
}

template <bool SYM, bool ROBUST>
__global__ __launch_bounds__(RS_THREADS) void part_fit_st_size_kernel(
    int p, int n, int b0, int num_hyps, float th, int tgt_per_part, const int *__restrict__ labels, const float *__restrict__ src,
    const float *__restrict__ tgt, const float *__restrict__ tgt_mean, const float *__restrict__ rot, const float *__restrict__ prev_scale,
    const float *__restrict__ prev_trans, const int *__restrict__ sample_rank, unsigned long long seed,
    const float *__restrict__ scale_free_in, const float *__restrict__ trans_free_in, const int *__restrict__ valid_free_in,
    const float *__restrict__ size_mean, const int *__restrict__ size_n, const int *__restrict__ size_miss, SzOpts opt,
    float *__restrict__ scale, float *__restrict__ trans, int *__restrict__ valid, float *__restrict__ scale_free,
    float *__restrict__ trans_free, int *__restrict__ valid_free, int *__restrict__ best_out, int *__restrict__ num_inliers,
    float *__restrict__ mean_out, int *__restrict__ n_out, int *__restrict__ miss_out, int *__restrict__ held_out,
    int *__restrict__ accepted_out, int *__restrict__ held_best, int *__restrict__ held_inliers) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rs_dyn[];
    __shared__ RsLds lds;
    __shared__ SzDecision dec;

    const int q = blockIdx.x;
    const int bi = q / p, pi = q % p;
    RsMembers mem = rs_members(src + (size_t)q * 3 * n, tgt + (size_t)(tgt_per_part ? q : bi) * 3 * n, n, tgt_mean, bi, rs_dyn);

    RsGivenRot<SYM> free_solve;      // the workgroup's rotation, as stored
    double rsum = 0;
    for (int i = 0; i < 9; ++i) {
        free_solve.R0[i] = rot[(size_t)q * 9 + i];
        rsum += free_solve.R0[i];
    }

    const int count = rs_list_members(labels + (size_t)bi * n, pi, n, mem.idx, lds.wcnt);
    rs_stage_members(mem, count);
    RsResult res;
    if constexpr (ROBUST) rs_fit<SYM>(mem, count, q, b0 + bi, pi, num_hyps, th, sample_rank, seed, nullptr, lds, res, free_solve);

    float tf[3] = {0.f, 0.f, 0.f};       // thread 0: the free fit's translation, as written
    if (threadIdx.x == 0) {
        // ---- the free fit: this kernel's own (part_fit_st_ransac_kernel's rule and bits), or the caller's
        float sf;
        int vf;
        if constexpr (ROBUST) {
            const bool ok = res.ok && count > 3 && isfinite(rsum);
            sf = ok ? res.sc : (prev_scale ? prev_scale[q] : 1.f);
#pragma unroll
            for (int a = 0; a < 3; ++a) tf[a] = ok ? res.tr[a] : (prev_trans ? prev_trans[(size_t)q * 3 + a] : 0.f);
            vf = ok ? 1 : 0;
            scale_free[q] = sf;
#pragma unroll
            for (int a = 0; a < 3; ++a) trans_free[(size_t)q * 3 + a] = tf[a];
            valid_free[q] = vf;
            if (best_out != nullptr) best_out[q] = res.best;
            if (num_inliers != nullptr) num_inliers[q] = res.ninl;
        } else {
            sf = scale_free_in[q];
#pragma unroll
            for (int a = 0; a < 3; ++a) tf[a] = trans_free_in[(size_t)q * 3 + a];
            vf = valid_free_in[q];
        }

        // ---- the decision, in double on the fp32 values as stored
        float mean_f = size_mean[q];
        int n_in = size_n[q];
        const int miss_in = size_miss[q];
        if (!(n_in > 0 && isfinite(mean_f) && mean_f > 0.f)) {      // an empty or insane state counts as empty; its mean is +0
            n_in = 0;
            mean_f = 0.f;
        }
        const double mean_in = mean_f, s = sf, ratio = opt.max_ratio;
        const bool finite = vf != 0 && isfinite(sf) && sf > 0.f;
        const bool established = n_in >= opt.min_frames;
        bool accept = finite && (!established || (s <= ratio * mean_in && s * ratio >= mean_in));
        float mean_o = mean_f;
        int n_o = n_in, miss_o = miss_in;
        if (!accept && finite) {
            miss_o = miss_in < INT_MAX ? miss_in + 1 : INT_MAX;
            if (opt.reset_after > 0 && miss_o >= opt.reset_after) {      // the state restarts from this frame
                mean_o = sf;
                n_o = 1;
                miss_o = 0;
                accept = true;
            }
        } else if (accept) {
            const int cap = opt.max_frames > 0 ? opt.max_frames - 1 : INT_MAX - 1;
            const int k = n_in < cap ? n_in : cap;
            mean_o = k == 0 ? sf : (float)(mean_in + (s - mean_in) / (double)(k + 1));
            n_o = k + 1;
            miss_o = 0;
        }
        const int held = (n_o >= opt.min_frames && isfinite(rsum)) ? 1 : 0;
        mean_out[q] = mean_o;
        n_out[q] = n_o;
        miss_out[q] = miss_o;
        held_out[q] = held;
        accepted_out[q] = accept ? 1 : 0;
        if (!held) {
            scale[q] = sf;
#pragma unroll
            for (int a = 0; a < 3; ++a) trans[(size_t)q * 3 + a] = tf[a];
            valid[q] = vf;
            if (held_best != nullptr) held_best[q] = 0;
            if (held_inliers != nullptr) held_inliers[q] = 0;
        }
        dec.held = held;
        dec.mean = mean_o;
    }
    __syncthreads();
    if (!dec.held) return;       // (uniform) not held: the cost is the free fit's

    // ---- held: the translation with the scale given, on the same staged members
    RsGivenRotScale<SYM> solve;
    for (int i = 0; i < 9; ++i) solve.R0[i] = free_solve.R0[i];
    solve.s = dec.mean;
    bool ok = false;
    float ft[3] = {0.f, 0.f, 0.f};
    int hb = 0, hn = 0;
    if constexpr (ROBUST) {
        RsResult hres;
        rs_fit<SYM>(mem, count, q, b0 + bi, pi, num_hyps, th, sample_rank, seed, nullptr, lds, hres, solve);
        ok = hres.ok && count > 3;       // (hres.ok: inliers >= 3 and every output finite; the sum of rot is finite: held)
#pragma unroll
        for (int a = 0; a < 3; ++a) ft[a] = hres.tr[a];
        hb = hres.best;
        hn = hres.ninl;
    } else {
        if (count > 3) ok = sz_fit_all(mem, count, lds, solve, ft);      // (uniform)
        hn = count;
    }
    if (threadIdx.x == 0) {
        scale[q] = dec.mean;
#pragma unroll
        for (int a = 0; a < 3; ++a) trans[(size_t)q * 3 + a] = ok ? ft[a] : tf[a];
        valid[q] = ok ? 1 : 0;
        if (held_best != nullptr) held_best[q] = hb;
        if (held_inliers != nullptr) held_inliers[q] = hn;
    }
}

template <bool SYM, bool ROBUST>
int part_fit_st_size_launch(int b, int p, int n, int b0, int num_hyps, float inlier_th, const int *labels, const float *src, const float *tgt,
                            int tgt_per_part, const float *tgt_mean, const float *rot, const float *prev_scale, const float *prev_trans,
                            const int *sample_rank, unsigned long long seed, const float *scale_free_in, const float *trans_free_in,
                            const int *valid_free_in, const float *size_mean, const int *size_n, const int *size_miss, SzOpts opt,
                            float *scale, float *trans, int *valid, float *scale_free, float *trans_free, int *valid_free, int *best,
                            int *num_inliers, float *mean_out, int *n_out, int *miss_out, int *held, int *accepted, int *held_best,
                            int *held_inliers, captra_stream_t stream) {
    constexpr auto kern = part_fit_st_size_kernel<SYM, ROBUST>;
    if (int e = captra_allow_lds<kern>(RS_LDS_MAX)) return e;
    CAPTRA_LAUNCH(ROBUST ? (SYM ? "part_fit_st_size_ransac_sym" : "part_fit_st_size_ransac") : (SYM ? "part_fit_st_size_sym" : "part_fit_st_size"),
                  kern, dim3(b * p), dim3(RS_THREADS), rs_lds_bytes(n), (hipStream_t)stream, p, n, b0, num_hyps, inlier_th, tgt_per_part,
                  labels, src, tgt, tgt_mean, rot, prev_scale, prev_trans, sample_rank, seed, scale_free_in, trans_free_in, valid_free_in,
                  size_mean, size_n, size_miss, opt, scale, trans, valid, scale_free, trans_free, valid_free, best, num_inliers, mean_out,
                  n_out, miss_out, held, accepted, held_best, held_inliers);
    return captra_last_error();
}

}  // namespace

extern "C" int captra_part_fit_st_size(int b, int p, int n, int sym, int b0, int num_hyps, float inlier_th, const int *labels,
                                       const float *src, const float *tgt, int tgt_per_part, const float *tgt_mean, const float *rot,
                                       const float *prev_scale, const float *prev_trans, const int *sample_rank, unsigned long long seed,
                                       const float *scale_free_in, const float *trans_free_in, const int *valid_free_in,
                                       const float *size_mean, const int *size_n, const int *size_miss, int min_frames, float max_ratio,
                                       int max_frames, int reset_after, float *scale, float *trans, int *valid, float *scale_free,
                                       float *trans_free, int *valid_free, int *best, int *num_inliers, float *mean_out, int *n_out,
                                       int *miss_out, int *held, int *accepted, int *held_best, int *held_inliers,
                                       captra_stream_t stream) {
    if (b < 0 || p < 1 || p > RS_MAX_P || n < 1 || n > RS_MAX_N || num_hyps < 0 || num_hyps > RS_MAX_H) return -1;
    if ((sym != 0 && sym != 1) || b0 < 0 || b0 > INT_MAX - b) return -1;
    if (min_frames < 1 || !(max_ratio > 1.f) || !isfinite(max_ratio) || max_frames < 0 || reset_after < 0) return -1;
    if (!labels || !src || !tgt || !rot || !size_mean || !size_n || !size_miss || !scale || !trans || !valid || !mean_out || !n_out ||
        !miss_out || !held || !accepted)
        return -1;
    const bool robust = num_hyps > 0;
    const bool any_in = scale_free_in || trans_free_in || valid_free_in, all_in = scale_free_in && trans_free_in && valid_free_in;
    if (robust ? (any_in || !scale_free || !trans_free || !valid_free) : !all_in) return -1;
    if (b == 0) return 0;
    const SzOpts opt = {min_frames, max_frames, reset_after, max_ratio};
#define SZ_ARGS                                                                                                                          \
    b, p, n, b0, num_hyps, inlier_th, labels, src, tgt, tgt_per_part, tgt_mean, rot, prev_scale, prev_trans, sample_rank, seed,          \
        scale_free_in, trans_free_in, valid_free_in, size_mean, size_n, size_miss, opt, scale, trans, valid, scale_free, trans_free,     \
        valid_free, best, num_inliers, mean_out, n_out, miss_out, held, accepted, held_best, held_inliers, stream
    if (robust) return sym ? part_fit_st_size_launch<true, true>(SZ_ARGS) : part_fit_st_size_launch<false, true>(SZ_ARGS);
    return sym ? part_fit_st_size_launch<true, false>(SZ_ARGS) : part_fit_st_size_launch<false, false>(SZ_ARGS);
#undef SZ_ARGS
}
