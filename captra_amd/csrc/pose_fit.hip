// On-device masked Procrustes pose fit for gfx950.
//
// Replaces part_fit_st_no_ransac (reference pose_utils/pose_fit.py:38-53) ->
// transform_pts_mask (pose_utils/procrustes.py:132-164) [-> transform_pts_2d_mask :213-228 ->
// rotate_pts_2d_batch :167-204] -> scale_pts_mask :117-120, translate_pts_mask :123-129, and
// rotate_pts_batch (:25-56).  The reference runs ~30 small ATen kernels per frame and moves the
// 2x2 / 3x3 cross-covariance to the HOST for torch.svd (procrustes.py:27,170), a blocking
// device->host->device round trip inside the frame loop.  Here one workgroup per
// (trajectory, part) does two reduction passes over the N points and solves the tiny problems
// in closed form on device; nothing leaves the GPU.
//
// Algebra (mask m_n = [label_n == part], c = sum m):
//   s_bar = sum m s / max(c,1), t_bar likewise                         (procrustes.py:137-138)
//   C   = sum m (t - t_bar)(s - s_bar)^T   (3x3),  Css = sum m (s - s_bar)(s - s_bar)^T
//   sym: the 2-D fit of procrustes.py:213-228 works on the (x,z) columns of s and of
//        t R; its cross-covariance is the (x,z) block of R^T C, its rotation
//        U diag(1,det(UV^T)) V^T is the rotation by atan2(M10-M01, M00+M11); R' = R * embed_y(R2)
//   scale = <R', C> / (sum m |R'(s - s_bar)|^2 + 1e-6)                  (procrustes.py:117-120)
//   trans = t_bar - scale * R' s_bar  (0 when c == 0)                   (procrustes.py:123-129)
//   valid = c > 3 and everything finite                                 (pose_fit.py:46, 26-35)
#include "common.h"
#include "pose_solve.h"
#include "rot_pool.h"
#include "wave_ops.h"

#include <math.h>

namespace {

constexpr int PF_THREADS = 256;

__global__ __launch_bounds__(PF_THREADS) void part_fit_st_kernel(int p, int n, int sym, int tgt_per_part,
                                                                 const int *__restrict__ labels,
                                                                 const float *__restrict__ src,
                                                                 const float *__restrict__ tgt,
                                                                 const float *__restrict__ rot,
                                                                 const float *__restrict__ given_scale,
                                                                 float *__restrict__ scale,
                                                                 float *__restrict__ trans,
                                                                 int *__restrict__ valid,
                                                                 const float *__restrict__ tgt_mean,
                                                                 const float *__restrict__ prev_scale,
                                                                 const float *__restrict__ prev_trans) {
    __shared__ double smem[15 * 4];
    const int q = blockIdx.x;
    const int bi = q / p, pi = q % p;
    const float *S = src + (size_t)q * 3 * n;
    const float *T = tgt + (size_t)(tgt_per_part ? q : bi) * 3 * n;
    // tgt_mean (B,3): the target is tgt + mean, formed here with the same single fp32 addition as the `points + points_mean`
    // tensor the reference builds (networks.py:219)
    const float tm[3] = {tgt_mean ? tgt_mean[bi * 3 + 0] : 0.f, tgt_mean ? tgt_mean[bi * 3 + 1] : 0.f, tgt_mean ? tgt_mean[bi * 3 + 2] : 0.f};
    const int *lab = labels + (size_t)bi * n;
    const int tid = threadIdx.x;

    // pass 1: count and centroids
    // (every point is loaded, members or not, and a non-member adds +0: the loads of the 16 iterations no longer wait for the
    // label they used to hide behind -- same sums bit for bit, since x + 0 = x -- and the loop pipelines)
    float fc = 0.f, fs[3] = {0.f, 0.f, 0.f}, ft[3] = {0.f, 0.f, 0.f};
#pragma unroll 4
    for (int i = tid; i < n; i += PF_THREADS) {
        const bool in = lab[i] == pi;
        fc += in ? 1.f : 0.f;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float sv = S[(size_t)a * n + i], tv = tgt_mean ? T[(size_t)a * n + i] + tm[a] : T[(size_t)a * n + i];
            fs[a] += in ? sv : 0.f;
            ft[a] += in ? tv : 0.f;
        }
    }
    double r1[7] = {fc, fs[0], fs[1], fs[2], ft[0], ft[1], ft[2]};
    wg_sum<WG_SUM_PAIRS, 4>(r1, smem);
    const double cnt = r1[0];
    const double den = cnt > 1.0 ? cnt : 1.0;
    const double sb[3] = {r1[1] / den, r1[2] / den, r1[3] / den};
    const double tb[3] = {r1[4] / den, r1[5] / den, r1[6] / den};
    const float sbf[3] = {(float)sb[0], (float)sb[1], (float)sb[2]};
    const float tbf[3] = {(float)tb[0], (float)tb[1], (float)tb[2]};

    // pass 2: centred cross-covariance C[a][c] = sum (t_a - tb_a)(s_c - sb_c), ss = sum |s - sb|^2
    float fC[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    float fS[6] = {0, 0, 0, 0, 0, 0};  // sum sc sc^T: xx xy xz yy yz zz
#pragma unroll 4
    for (int i = tid; i < n; i += PF_THREADS) {
        const bool in = lab[i] == pi;
        float sc[3], tc[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            sc[a] = S[(size_t)a * n + i] - sbf[a];
            tc[a] = (tgt_mean ? T[(size_t)a * n + i] + tm[a] : T[(size_t)a * n + i]) - tbf[a];
        }
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float v = tc[a] * sc[c];
                fC[a * 3 + c] += in ? v : 0.f;
            }
        const float q0 = sc[0] * sc[0], q1 = sc[0] * sc[1], q2 = sc[0] * sc[2], q3 = sc[1] * sc[1], q4 = sc[1] * sc[2], q5 = sc[2] * sc[2];
        fS[0] += in ? q0 : 0.f; fS[1] += in ? q1 : 0.f; fS[2] += in ? q2 : 0.f;
        fS[3] += in ? q3 : 0.f; fS[4] += in ? q4 : 0.f; fS[5] += in ? q5 : 0.f;
    }
    double r2[15];
#pragma unroll
    for (int i = 0; i < 9; ++i) r2[i] = fC[i];
#pragma unroll
    for (int i = 0; i < 6; ++i) r2[9 + i] = fS[i];
    wg_sum<WG_SUM_PAIRS, 4>(r2, smem);

    if (tid == 0) {
        double R[9], Rf[9];
        for (int i = 0; i < 9; ++i) Rf[i] = R[i] = rot[(size_t)q * 9 + i];
        if (sym) ps_rot_about_y(R, r2, Rf);       // R' = R embed_y(the 2-D fit)
        const double sca = given_scale ? (double)given_scale[q] : ps_scale(Rf, r2, r2 + 9);
        double tr[3];
        ps_trans(Rf, sca, sb, tb, tr);
        for (int a = 0; a < 3; ++a) tr[a] = cnt > 0.0 ? tr[a] : 0.0;
        const float scf = (float)sca;
        const float trf[3] = {(float)tr[0], (float)tr[1], (float)tr[2]};
        double rsum = 0;
        for (int i = 0; i < 9; ++i) rsum += R[i];
        const float tsum = (trf[0] + trf[1]) + trf[2];
        const bool ok = (cnt > 3.0) && isfinite(scf) && isfinite(tsum) && isfinite(rsum);
        // prev_*: an invalid fit (<= 3 points, non-finite) keeps the previous scale / translation (networks.py:230-232)
        scale[q] = (ok || !prev_scale) ? scf : prev_scale[q];
#pragma unroll
        for (int a = 0; a < 3; ++a) trans[(size_t)q * 3 + a] = (ok || !prev_trans) ? trf[a] : prev_trans[(size_t)q * 3 + a];
        valid[q] = ok;
    }
}

// ---- 3x3 orthogonal Procrustes: jacobi_eig3 / kabsch3 live in pose_solve.h (shared with pose_ransac.hip) ---------------------
__global__ __launch_bounds__(PF_THREADS) void procrustes_rot3_kernel(int n, const float *__restrict__ src,
                                                                     const float *__restrict__ tgt,
                                                                     float *__restrict__ rot) {
    __shared__ double smem[9 * 4];
    const int bi = blockIdx.x;
    const float *S = src + (size_t)bi * n * 3, *T = tgt + (size_t)bi * n * 3;
    double m[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = threadIdx.x; i < n; i += PF_THREADS) {
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int c = 0; c < 3; ++c) m[a * 3 + c] += (double)T[(size_t)i * 3 + a] * (double)S[(size_t)i * 3 + c];
    }
    wg_sum<WG_SUM_PAIRS, 4>(m, smem);
    if (threadIdx.x == 0) {
        double R[9];
        kabsch3(m, R);
        for (int i = 0; i < 9; ++i) rot[(size_t)bi * 9 + i] = (float)R[i];
    }
}

// ---------------------------------------------------------------------------------------------
// Rotation read-out of the tracking step in one launch (one workgroup per (trajectory, part)):
//   per point:  unit y-axis (symmetric, 3 outputs)  or  ortho6d -> rotation matrix (6 outputs)
//               blocks.py:147-156 (RotationRegressor.forward), rotations.py:302-343
//   pooled   =  masked mean over the points labelled with the part; (0,1,0) / identity when none
//               networks.py:127-138
//   dR       =  from_3d(pooled) (y-axis -> frame)  or  Gram-Schmidt on the columns of pooled
//               part_dof_utils.py:137-141, rotations.py:356-387
//   R        =  R_prev * dR                          part_dof_utils.py:124-134
// Only head p on cloud (b,p) is evaluated (the reference computes all P x P and keeps the diagonal,
// networks.py:200-203).  The reference runs ~60 tiny ATen kernels for this.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PF_THREADS) void rot_pool_compose_kernel(int p, int n, int sym, int diag, const float *__restrict__ raw,
                                                                      const int *__restrict__ labels,
                                                                      const float *__restrict__ prev_rot,
                                                                      float *__restrict__ rot, float *__restrict__ delta) {
    __shared__ double smem[10 * 4];
    const int q = blockIdx.x;            // = b * P + part: cloud q, head `part`
    const int bi = q / p, pi = q % p;
    // the pooling loop, its reduction and the tail live in rot_pool.h (shared with rot_consensus.hip); here every member pools
    rp_pool_compose(q, pi, n, sym, rp_head(raw, q, p, pi, n, sym, diag), labels + (size_t)bi * n, prev_rot, rot, delta, smem, RpAllMembers());
}

}  // namespace

extern "C" int captra_rot_pool_compose(int b, int p, int n, int sym, int diag_only, const float *raw, const int *labels,
                                       const float *prev_rot, float *rot, float *delta, captra_stream_t stream) {
    if (b < 0 || p < 1 || n < 0) return -1;
    if (b == 0) return 0;
    CAPTRA_LAUNCH("rot_pool_compose", rot_pool_compose_kernel, dim3(b * p), dim3(PF_THREADS), 0, (hipStream_t)stream, p, n, sym,
                  diag_only, raw, labels, prev_rot, rot, delta);
    return captra_last_error();
}

extern "C" int captra_part_fit_st(int b, int p, int n, int sym, const int *labels, const float *src,
                                  const float *tgt, int tgt_per_part, const float *rot, const float *given_scale,
                                  float *scale, float *trans, int *valid, captra_stream_t stream) {
    if (b < 0 || p < 1 || n < 0) return -1;
    if (b == 0) return 0;
    CAPTRA_LAUNCH("part_fit_st", part_fit_st_kernel, dim3(b * p), dim3(PF_THREADS), 0, (hipStream_t)stream, p, n,
                  sym, tgt_per_part, labels, src, tgt, rot, given_scale, scale, trans, valid, (const float *)nullptr,
                  (const float *)nullptr, (const float *)nullptr);
    return captra_last_error();
}

// The track loop's form of captra_part_fit_st (networks.py:219-232 in one launch): the target is pts (B,3,N) + pts_mean (B,3)
// -- formed in the kernel, no (B,3,N) temporary -- and a part whose fit is invalid keeps prev_scale (B,P) / prev_trans (B,P,3).
extern "C" int captra_part_fit_st_track(int b, int p, int n, int sym, const int *labels, const float *src, const float *pts,
                                        const float *pts_mean, const float *rot, const float *prev_scale, const float *prev_trans,
                                        float *scale, float *trans, int *valid, captra_stream_t stream) {
    if (b < 0 || p < 1 || n < 0) return -1;
    if (b == 0) return 0;
    CAPTRA_LAUNCH("part_fit_st", part_fit_st_kernel, dim3(b * p), dim3(PF_THREADS), 0, (hipStream_t)stream, p, n,
                  sym, 0, labels, src, pts, rot, (const float *)nullptr, scale, trans, valid, pts_mean, prev_scale, prev_trans);
    return captra_last_error();
}

extern "C" int captra_procrustes_rot3(int nb, int n, const float *src, const float *tgt, float *rot,
                                      captra_stream_t stream) {
    if (nb < 0 || n < 0) return -1;
    if (nb == 0) return 0;
    CAPTRA_LAUNCH("procrustes_rot3", procrustes_rot3_kernel, dim3(nb), dim3(PF_THREADS), 0, (hipStream_t)stream, n,
                  src, tgt, rot);
    return captra_last_error();
}
