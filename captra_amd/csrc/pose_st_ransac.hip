// Robust scale / translation fit of the tracking step: RANSAC with the rotation GIVEN, per (trajectory, part), on device for gfx950.
//
// The counterpart the name of the reference's part_fit_st_no_ransac (pose_utils/pose_fit.py:38-53) promises and its code does not
// have: RotationNet's rotation is taken as it is, and scale and translation are fitted to the part's NOCS <-> camera correspondences
// by three-member hypotheses, an inlier count, the first best one and a refit on its inliers -- instead of one least-squares sum
// that takes a mislabelled or depth-edge point at full weight.  Semantics: include/captra_hip.h, captra_part_fit_st_ransac.
//
// One workgroup of RS_THREADS per (b, p), the skeleton of captra_part_fit_ransac (pose_ransac.h: member list in LDS, staged
// coordinates, counter-based draws with b0 + b in the key, the two inlier tests, first best, fixed-order double sums); what differs
// is the solver rs_fit is instantiated with: RsGivenRot (the algebra of part_fit_st_kernel, pose_fit.hip, on a set of pairs) in
// place of the Umeyama similarity fit, in the hypotheses and in the refit alike.
#include "pose_ransac.h"

#include <limits.h>

namespace {

template <bool SYM>
__global__ __launch_bounds__(RS_THREADS) void part_fit_st_ransac_kernel(int p, int n, int b0, int num_hyps, float th, int tgt_per_part,
                                                                        const int *__restrict__ labels, const float *__restrict__ src,
                                                                        const float *__restrict__ tgt, const float *__restrict__ tgt_mean,
                                                                        const float *__restrict__ rot, const float *__restrict__ prev_scale,
                                                                        const float *__restrict__ prev_trans,
                                                                        const int *__restrict__ sample_rank, unsigned long long seed,
                                                                        float *__restrict__ scale, float *__restrict__ trans,
                                                                        int *__restrict__ valid, int *__restrict__ best_out,
                                                                        int *__restrict__ num_inliers) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rs_dyn[];
    __shared__ RsLds lds;

    const int q = blockIdx.x;
    const int bi = q / p, pi = q % p;
    RsMembers mem = rs_members(src + (size_t)q * 3 * n, tgt + (size_t)(tgt_per_part ? q : bi) * 3 * n, n, tgt_mean, bi, rs_dyn);

    RsGivenRot<SYM> solve;      // the workgroup's rotation, as stored
    double rsum = 0;
    for (int i = 0; i < 9; ++i) {
        solve.R0[i] = rot[(size_t)q * 9 + i];
        rsum += solve.R0[i];
    }

    const int count = rs_list_members(labels + (size_t)bi * n, pi, n, mem.idx, lds.wcnt);
    rs_stage_members(mem, count);
    RsResult res;
    rs_fit<SYM>(mem, count, q, b0 + bi, pi, num_hyps, th, sample_rank, seed, nullptr, lds, res, solve);

    if (threadIdx.x == 0) {
        // count > 3 is the one-pass fit's rule (pose_fit.hip): the option does not change which parts count as fitted by size
        const bool ok = res.ok && count > 3 && isfinite(rsum);
        scale[q] = ok ? res.sc : (prev_scale ? prev_scale[q] : 1.f);
#pragma unroll
        for (int a = 0; a < 3; ++a) trans[(size_t)q * 3 + a] = ok ? res.tr[a] : (prev_trans ? prev_trans[(size_t)q * 3 + a] : 0.f);
        valid[q] = ok ? 1 : 0;
        if (best_out != nullptr) best_out[q] = res.best;
        if (num_inliers != nullptr) num_inliers[q] = res.ninl;
    }
}

template <bool SYM>
int part_fit_st_ransac_launch(int b, int p, int n, int b0, int num_hyps, float inlier_th, const int *labels, const float *src, const float *tgt,
                              int tgt_per_part, const float *tgt_mean, const float *rot, const float *prev_scale, const float *prev_trans,
                              const int *sample_rank, unsigned long long seed, float *scale, float *trans, int *valid, int *best,
                              int *num_inliers, captra_stream_t stream) {
    constexpr auto kern = part_fit_st_ransac_kernel<SYM>;
    if (int e = captra_allow_lds<kern>(RS_LDS_MAX)) return e;
    CAPTRA_LAUNCH(SYM ? "part_fit_st_ransac_sym" : "part_fit_st_ransac", kern, dim3(b * p), dim3(RS_THREADS), rs_lds_bytes(n), (hipStream_t)stream,
                  p, n, b0, num_hyps, inlier_th, tgt_per_part, labels, src, tgt, tgt_mean, rot, prev_scale, prev_trans, sample_rank, seed, scale,
                  trans, valid, best, num_inliers);
    return captra_last_error();
}

}  // namespace

extern "C" int captra_part_fit_st_ransac(int b, int p, int n, int sym, int b0, int num_hyps, float inlier_th, const int *labels,
                                         const float *src, const float *tgt, int tgt_per_part, const float *tgt_mean, const float *rot,
                                         const float *prev_scale, const float *prev_trans, const int *sample_rank, unsigned long long seed,
                                         float *scale, float *trans, int *valid, int *best, int *num_inliers, captra_stream_t stream) {
    if (b < 0 || p < 1 || p > RS_MAX_P || n < 1 || n > RS_MAX_N || num_hyps < 1 || num_hyps > RS_MAX_H) return -1;
    if ((sym != 0 && sym != 1) || b0 < 0 || b0 > INT_MAX - b) return -1;
    if (b == 0) return 0;
    return sym ? part_fit_st_ransac_launch<true>(b, p, n, b0, num_hyps, inlier_th, labels, src, tgt, tgt_per_part, tgt_mean, rot, prev_scale,
                                                 prev_trans, sample_rank, seed, scale, trans, valid, best, num_inliers, stream)
               : part_fit_st_ransac_launch<false>(b, p, n, b0, num_hyps, inlier_th, labels, src, tgt, tgt_per_part, tgt_mean, rot, prev_scale,
                                                  prev_trans, sample_rank, seed, scale, trans, valid, best, num_inliers, stream);
}
