// Track health: does the pose that leaves a step still explain the frame's NOCS <-> camera correspondences, and where it does not,
// a re-fit of the part by the RANSAC similarity fit -- per (trajectory, part), on device for gfx950, inside the step's launch
// sequence.  No reference counterpart: the reference's loop runs open loop after frame 0.  Semantics: include/captra_hip.h,
// captra_part_fit_guard.
//
// One workgroup of RS_THREADS per (b, p):
//   1. the members (label == p) in ascending point index into the u16 list in LDS (pose_ransac.h);
//   2. check: every member's squared fp32 residual under the tracked pose's twelve parameters (fp32(scale rot), trans), by the
//      one inlier test of the RANSAC fit (pose_solve.h); inliers counted by ballot + population count (integers: any order gives
//      the same sum), their squared residuals summed in double (each thread its members in ascending order, then the fixed tree
//      of the workgroup sum, wave_ops.h); the members are read through the list, once each -- nothing is staged for a part that is not lost;
//   3. verdict from integers alone: count < min_members, inliers * D < L * count;
//   4. only for a lost part with refit = 1: the coordinates into LDS and the RANSAC fit's own stages (pose_ransac.h, the same
//      device functions as captra_part_fit_ransac: same members, same draws with b0 + b in the key, same bits); accepted when it
//      is valid and its best hypothesis scores strictly more inliers than the tracked pose had.
// captra_part_fit_guard_sym is the same kernel instantiated with the axis-only test of the symmetric categories (pose_solve.h:
// RsTest<true>): step 2 forms the seven parameters (second column of rot, scale, trans), and the re-fit scores by the same test.
// Everything a verdict depends on is uniform over the workgroup (block-wide integer sums), so whole workgroups leave after 3.
#include "pose_ransac.h"

namespace {

enum { GUARD_OK = 0, GUARD_TOO_FEW = 1, GUARD_LOST = 2, GUARD_RECOVERED = 3 };

template <bool SYM>
__global__ __launch_bounds__(RS_THREADS) void part_fit_guard_kernel(int p, int n, int b0, const int *__restrict__ labels,
                                                                    const float *__restrict__ src, const float *__restrict__ pts,
                                                                    const float *__restrict__ pts_mean, const float *__restrict__ rot,
                                                                    const float *__restrict__ scale, const float *__restrict__ trans,
                                                                    float th, int lost_num, int lost_den, int min_members, int refit,
                                                                    int num_hyps, unsigned long long seed, int *__restrict__ count_out,
                                                                    int *__restrict__ inliers_out, float *__restrict__ rms_out,
                                                                    int *__restrict__ verdict_out, float *__restrict__ rot_out,
                                                                    float *__restrict__ scale_out, float *__restrict__ trans_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rs_dyn[];
    __shared__ RsLds lds;

    const int q = blockIdx.x;
    const int bi = q / p, pi = q % p;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    RsMembers mem = rs_members(src + (size_t)q * 3 * n, pts + (size_t)bi * 3 * n, n, pts_mean, bi, rs_dyn);

    // ---- 1. members
    const int count = rs_list_members(labels + (size_t)bi * n, pi, n, mem.idx, lds.wcnt);

    // ---- 2. the tracked pose against them
    using Test = RsTest<SYM>;
    const float sc = scale[q];
    float hp[Test::NPAR];
    if constexpr (SYM) {        // (a, scale, trans): the y-axis as the pose holds it, taken as a unit vector
#pragma unroll
        for (int a = 0; a < 3; ++a) hp[a] = rot[(size_t)q * 9 + a * 3 + 1];
        hp[3] = sc;
#pragma unroll
        for (int a = 0; a < 3; ++a) hp[4 + a] = trans[(size_t)q * 3 + a];
    } else {
#pragma unroll
        for (int i = 0; i < 9; ++i) hp[i] = sc * rot[(size_t)q * 9 + i];
#pragma unroll
        for (int a = 0; a < 3; ++a) hp[9 + a] = trans[(size_t)q * 3 + a];
    }
    const float th2 = th * th;
    int mine = 0;
    double sq[1] = {0.0};
    for (int base = 0; base < count; base += RS_THREADS) {      // (uniform trip count: the ballot is met by whole waves)
        const int m = base + tid;
        bool in = false;
        float e2 = 0.f;
        if (m < count) {
            float s[3], t[3];
            mem.load(m, s, t);
            const float rho = SYM ? rs_sym_radius(s) : 0.f;
            e2 = Test::residual2(s, rho, t, hp);
            in = Test::inlier(s, rho, t, hp, th2);
        }
        mine += __popcll(__ballot(in));
        if (in) sq[0] += (double)e2;
    }
    if (lane == 0) lds.wcnt[wave] = mine;
    wg_sum<WG_SUM_SERIAL, RS_WAVES>(sq, lds.red);                             // (its barriers also publish wcnt)
    int inliers = 0;
#pragma unroll
    for (int w = 0; w < RS_WAVES; ++w) inliers += lds.wcnt[w];

    // ---- 3. verdict
    int verdict = GUARD_OK;
    if (count < min_members) verdict = GUARD_TOO_FEW;
    else if ((long long)inliers * lost_den < (long long)lost_num * count) verdict = GUARD_LOST;

    // ---- 4. re-fit of a lost part
    RsResult res;
    if (refit && verdict == GUARD_LOST) {       // (uniform)
        rs_stage_members(mem, count);
        rs_fit<SYM>(mem, count, q, b0 + bi, pi, num_hyps, th, nullptr, seed, nullptr, lds, res);
    }

    if (tid == 0) {
        const bool take = res.ok && res.ninl > inliers;
        count_out[q] = count;
        inliers_out[q] = inliers;
        rms_out[q] = inliers > 0 ? (float)sqrt(sq[0] / (double)inliers) : 0.f;
        verdict_out[q] = take ? GUARD_RECOVERED : verdict;
        if (rot_out != nullptr)
            for (int i = 0; i < 9; ++i) rot_out[(size_t)q * 9 + i] = take ? res.R[i] : rot[(size_t)q * 9 + i];
        if (scale_out != nullptr) scale_out[q] = take ? res.sc : sc;
        if (trans_out != nullptr)
            for (int a = 0; a < 3; ++a) trans_out[(size_t)q * 3 + a] = take ? res.tr[a] : trans[(size_t)q * 3 + a];
    }
}

}  // namespace

template <bool SYM>
static int part_fit_guard_launch(int b, int p, int n, int b0, const int *labels, const float *src, const float *pts, const float *pts_mean,
                                 const float *rot, const float *scale, const float *trans, float inlier_th, int lost_num, int lost_den,
                                 int min_members, int refit, int num_hyps, unsigned long long seed, int *count, int *inliers, float *rms,
                                 int *verdict, float *rot_out, float *scale_out, float *trans_out, captra_stream_t stream) {
    if (b < 0 || p < 1 || p > RS_MAX_P || n < 1 || n > RS_MAX_N || num_hyps < 1 || num_hyps > RS_MAX_H) return -1;
    if (b0 < 0 || b0 > 0x7fffffff - b || lost_num < 0 || lost_den < 1 || (refit != 0 && refit != 1)) return -1;
    if (refit && (rot_out == nullptr || scale_out == nullptr || trans_out == nullptr)) return -1;
    if (b == 0) return 0;
    // (monitoring touches the member list alone: it asks for that much LDS and no more, so that workgroups share a CU)
    constexpr auto kern = part_fit_guard_kernel<SYM>;
    if (int e = captra_allow_lds<kern>(RS_LDS_MAX)) return e;
    CAPTRA_LAUNCH(SYM ? "part_fit_guard_sym" : "part_fit_guard", kern, dim3(b * p), dim3(RS_THREADS), refit ? rs_lds_bytes(n) : rs_idx_bytes(n),
                  (hipStream_t)stream, p, n, b0, labels, src, pts, pts_mean, rot, scale, trans, inlier_th, lost_num, lost_den, min_members, refit,
                  num_hyps, seed, count, inliers, rms, verdict, rot_out, scale_out, trans_out);
    return captra_last_error();
}

extern "C" int captra_part_fit_guard(int b, int p, int n, int b0, const int *labels, const float *src, const float *pts,
                                     const float *pts_mean, const float *rot, const float *scale, const float *trans, float inlier_th,
                                     int lost_num, int lost_den, int min_members, int refit, int num_hyps, unsigned long long seed,
                                     int *count, int *inliers, float *rms, int *verdict, float *rot_out, float *scale_out,
                                     float *trans_out, captra_stream_t stream) {
    return part_fit_guard_launch<false>(b, p, n, b0, labels, src, pts, pts_mean, rot, scale, trans, inlier_th, lost_num, lost_den, min_members,
                                        refit, num_hyps, seed, count, inliers, rms, verdict, rot_out, scale_out, trans_out, stream);
}

// the axis-only inlier test of the symmetric categories in the check AND in the re-fit: both counts of the acceptance rule by one test
extern "C" int captra_part_fit_guard_sym(int b, int p, int n, int b0, const int *labels, const float *src, const float *pts,
                                         const float *pts_mean, const float *rot, const float *scale, const float *trans, float inlier_th,
                                         int lost_num, int lost_den, int min_members, int refit, int num_hyps, unsigned long long seed,
                                         int *count, int *inliers, float *rms, int *verdict, float *rot_out, float *scale_out,
                                         float *trans_out, captra_stream_t stream) {
    return part_fit_guard_launch<true>(b, p, n, b0, labels, src, pts, pts_mean, rot, scale, trans, inlier_th, lost_num, lost_den, min_members,
                                       refit, num_hyps, seed, count, inliers, rms, verdict, rot_out, scale_out, trans_out, stream);
}
