// RANSAC similarity fit (rotation + scale + translation) between NOCS coordinates and camera points, per (trajectory, part),
// on device for gfx950.
//
// Replaces pose_fit of the reference's datasets/nocs_data/preproc_nocs/align_pose.py:49-93 (host numpy: 64 three-point Umeyama
// hypotheses, the inlier count of each at a distance threshold, the first best one, a refit on its inliers) -- the estimator
// that needs no previous pose.  Semantics: include/captra_hip.h, captra_part_fit_ransac.
//
// One workgroup of RS_THREADS per (b, p):
//   1. compact the members (label == p) in ascending point index into a u16 list in LDS; for N <= RS_LDS_N their six
//      coordinates follow them into LDS (the target with its mean added once), above that they are re-read through the list;
//   2. thread h solves hypothesis h in double: centre the three pairs, kabsch3 on tgt_c^T src_c, scale, translation; the
//      parameters (s R, t) go to LDS as fp32;
//   3. score: a work item is (256 members, 16 hypotheses); a wave holds four members per lane in registers and walks its
//      hypotheses, whose parameters are wave-uniform LDS reads; a member is an inlier when the squared fp32 residual is below
//      th^2, counted by ballot + population count, added to score[h] as an INTEGER (any order gives the same sum);
//   4. best = first h with the largest score; two double block reductions over its inliers (count and centroids, then the
//      centred cross-covariance and source covariance) and one thread finishes the same Umeyama solve.
// The inlier test is one fp32 expression of (member, hypothesis) alone, evaluated by the same inline function in 3. and 4.:
// the inlier set is a pure function of the inputs, whatever the wave that meets the member.  captra_part_fit_ransac_sym is the
// same kernel instantiated with the axis-only test of the symmetric categories (pose_solve.h: RsTest<true>), whose per-hypothesis
// parameters are (second column of R, s, t); the output rotation is still the full Kabsch rotation of the refit.
#include "pose_ransac.h"

namespace {

template <bool SYM>
__global__ __launch_bounds__(RS_THREADS) void part_fit_ransac_kernel(int p, int n, int num_hyps, float th, int tgt_per_part,
                                                                     const int *__restrict__ labels, const float *__restrict__ src,
                                                                     const float *__restrict__ tgt, const float *__restrict__ tgt_mean,
                                                                     const int *__restrict__ sample_rank, unsigned long long seed,
                                                                     float *__restrict__ rot, float *__restrict__ scale,
                                                                     float *__restrict__ trans, int *__restrict__ valid,
                                                                     int *__restrict__ best_out, int *__restrict__ num_inliers,
                                                                     int *__restrict__ samples_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rs_dyn[];
    __shared__ RsLds lds;

    const int q = blockIdx.x;
    const int bi = q / p, pi = q % p;
    RsMembers mem = rs_members(src + (size_t)q * 3 * n, tgt + (size_t)(tgt_per_part ? q : bi) * 3 * n, n, tgt_mean, bi, rs_dyn);

    const int count = rs_list_members(labels + (size_t)bi * n, pi, n, mem.idx, lds.wcnt);  // 1. (pose_ransac.h)
    rs_stage_members(mem, count);
    RsResult res;
    rs_fit<SYM>(mem, count, q, bi, pi, num_hyps, th, sample_rank, seed, samples_out, lds, res);  // 2.-4.

    if (threadIdx.x == 0) {
        for (int i = 0; i < 9; ++i) rot[(size_t)q * 9 + i] = res.R[i];
        scale[q] = res.sc;
        for (int a = 0; a < 3; ++a) trans[(size_t)q * 3 + a] = res.tr[a];
        valid[q] = res.ok ? 1 : 0;
        if (best_out != nullptr) best_out[q] = res.best;
        if (num_inliers != nullptr) num_inliers[q] = res.ninl;
    }
}

}  // namespace

template <bool SYM>
static int part_fit_ransac_launch(int b, int p, int n, int num_hyps, float inlier_th, const int *labels, const float *src, const float *tgt,
                                  int tgt_per_part, const float *tgt_mean, const int *sample_rank, unsigned long long seed, float *rot,
                                  float *scale, float *trans, int *valid, int *best, int *num_inliers, int *samples_out,
                                  captra_stream_t stream) {
    if (b < 0 || p < 1 || p > RS_MAX_P || n < 1 || n > RS_MAX_N || num_hyps < 1 || num_hyps > RS_MAX_H) return -1;
    if (b == 0) return 0;
    constexpr auto kern = part_fit_ransac_kernel<SYM>;
    if (int e = captra_allow_lds<kern>(RS_LDS_MAX)) return e;
    CAPTRA_LAUNCH(SYM ? "part_fit_ransac_sym" : "part_fit_ransac", kern, dim3(b * p), dim3(RS_THREADS), rs_lds_bytes(n), (hipStream_t)stream,
                  p, n, num_hyps, inlier_th, tgt_per_part, labels, src, tgt, tgt_mean, sample_rank, seed, rot, scale, trans, valid, best,
                  num_inliers, samples_out);
    return captra_last_error();
}

extern "C" int captra_part_fit_ransac(int b, int p, int n, int num_hyps, float inlier_th, const int *labels, const float *src,
                                      const float *tgt, int tgt_per_part, const float *tgt_mean, const int *sample_rank,
                                      unsigned long long seed, float *rot, float *scale, float *trans, int *valid, int *best,
                                      int *num_inliers, int *samples_out, captra_stream_t stream) {
    return part_fit_ransac_launch<false>(b, p, n, num_hyps, inlier_th, labels, src, tgt, tgt_per_part, tgt_mean, sample_rank, seed, rot,
                                         scale, trans, valid, best, num_inliers, samples_out, stream);
}

// the axis-only inlier test of the symmetric categories in the scores and in the winner's inlier set; everything else as above
extern "C" int captra_part_fit_ransac_sym(int b, int p, int n, int num_hyps, float inlier_th, const int *labels, const float *src,
                                          const float *tgt, int tgt_per_part, const float *tgt_mean, const int *sample_rank,
                                          unsigned long long seed, float *rot, float *scale, float *trans, int *valid, int *best,
                                          int *num_inliers, int *samples_out, captra_stream_t stream) {
    return part_fit_ransac_launch<true>(b, p, n, num_hyps, inlier_th, labels, src, tgt, tgt_per_part, tgt_mean, sample_rank, seed, rot,
                                        scale, trans, valid, best, num_inliers, samples_out, stream);
}
