// The rotation read-out's per-point vote, its masked pooling and its tail, shared by pose_fit.hip (captra_rot_pool_compose: every
// member pools) and rot_consensus.hip (captra_rot_pool_consensus: the inliers of the winning vote pool).  Both kernels go through
// rp_pool_compose with RP_THREADS accumulating threads, the same stride, the same double sums and the same reduction order, so
// the same set of pooled points gives the same bits whichever kernel pooled it.
#pragma once
#include "common.h"
#include "wave_ops.h"

#include <math.h>

namespace {

constexpr int RP_THREADS = 256;      // accumulating threads (the first RP_THREADS of the workgroup; pose_fit.hip's PF_THREADS)
constexpr int RP_WAVES = RP_THREADS / 64;

__device__ __forceinline__ void normalize3(const float v[3], float out[3]) {  // rotations.py:302-314
    const float mag = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    if (mag > 1e-8f) {
        const float d = fmaxf(mag, 1e-8f);
        out[0] = v[0] / d; out[1] = v[1] / d; out[2] = v[2] / d;
    } else {
        out[0] = 1.f; out[1] = 0.f; out[2] = 0.f;
    }
}
__device__ __forceinline__ void cross3(const float u[3], const float v[3], float out[3]) {
    out[0] = u[1] * v[2] - u[2] * v[1];
    out[1] = u[2] * v[0] - u[0] * v[2];
    out[2] = u[0] * v[1] - u[1] * v[0];
}

// raw -> the outputs of head `pi` on cloud q.  diag: raw holds only head `part` on cloud (b, part) -- (B*P, R, N); else all P heads
// per cloud -- (B*P, P, R, N)
__device__ __forceinline__ const float *rp_head(const float *raw, int q, int p, int pi, int n, int sym, int diag) {
    const int R = sym ? 3 : 6;
    return raw + (diag ? (size_t)q : (size_t)q * p + pi) * R * n;
}

// The per-point prediction of point e: sym -> v[0..3) the unit axis; else the ortho6d frame's columns x = v[0..3), y = v[3..6),
// z = v[6..9)
__device__ __forceinline__ void rp_vote(const float *__restrict__ src, int n, int e, int sym, float v[9]) {
    if (sym) {
        const float a[3] = {src[e], src[n + e], src[2 * (size_t)n + e]};
        normalize3(a, v);
    } else {
        const float a[3] = {src[e], src[n + e], src[2 * (size_t)n + e]};
        const float c[3] = {src[3 * (size_t)n + e], src[4 * (size_t)n + e], src[5 * (size_t)n + e]};
        float zr[3];
        normalize3(a, v);
        cross3(v, c, zr);
        normalize3(zr, v + 6);
        cross3(v + 6, v, v + 3);
    }
}

struct RpAllMembers {       // the plain read-out: every point labelled with the part pools
    __device__ __forceinline__ bool operator()(bool in, const float *) const { return in; }
};

// Masked mean of the votes of the points e with pool(label == pi, vote), the frame of the mean ((0,1,0) / identity when nothing
// pooled), rot = prev_rot * dR and, when non-NULL, delta = dR.  Every thread of the workgroup calls it (two barriers inside); the
// first RP_THREADS accumulate, thread 0 finishes.  smem: [10][RP_WAVES] doubles.
template <class Pool>
__device__ __forceinline__ void rp_pool_compose(int q, int pi, int n, int sym, const float *__restrict__ src, const int *__restrict__ lab,
                                                const float *__restrict__ prev_rot, float *__restrict__ rot, float *__restrict__ delta,
                                                double *smem, const Pool &pool) {
    double acc[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) acc[i] = 0.0;
    // (every point is loaded and normalised, a non-member adds +0.0 through a select -- no NaN of a degenerate non-member can
    // leak in: the loads no longer wait for the label, the loop pipelines, the sums are the same bit for bit)
#pragma unroll 4
    for (int e = threadIdx.x < RP_THREADS ? (int)threadIdx.x : n; e < n; e += RP_THREADS) {
        float v[9];
        rp_vote(src, n, e, sym, v);
        const bool in = pool(lab[e] == pi, v);
        acc[9] += in ? 1.0 : 0.0;
        if (sym) {
            acc[0] += in ? (double)v[0] : 0.0; acc[1] += in ? (double)v[1] : 0.0; acc[2] += in ? (double)v[2] : 0.0;
        } else {
            // row-major 3x3 with columns x, y, z
            acc[0] += in ? (double)v[0] : 0.0; acc[1] += in ? (double)v[3] : 0.0; acc[2] += in ? (double)v[6] : 0.0;
            acc[3] += in ? (double)v[1] : 0.0; acc[4] += in ? (double)v[4] : 0.0; acc[5] += in ? (double)v[7] : 0.0;
            acc[6] += in ? (double)v[2] : 0.0; acc[7] += in ? (double)v[5] : 0.0; acc[8] += in ? (double)v[8] : 0.0;
        }
    }
    // the workgroup sum of wave_ops.h in its two halves: only the accumulating waves store, and thread 0 alone combines
    wg_sum_publish<RP_WAVES>(acc, smem, threadIdx.x < RP_THREADS);
    if (threadIdx.x != 0) return;
    wg_sum_combine<WG_SUM_PAIRS, RP_WAVES>(acc, smem);
    const float cnt = (float)acc[9];
    float dR[9];  // row-major
    if (sym) {
        float v[3];
        if (cnt > 0.f) { v[0] = (float)acc[0] / fmaxf(cnt, 1.f); v[1] = (float)acc[1] / fmaxf(cnt, 1.f); v[2] = (float)acc[2] / fmaxf(cnt, 1.f); }
        else { v[0] = 0.f; v[1] = 1.f; v[2] = 0.f; }
        float y[3], zr[3], z[3], x[3];
        const float ex[3] = {1.f, 0.f, 0.f};
        normalize3(v, y);
        cross3(ex, y, zr);
        normalize3(zr, z);
        cross3(y, z, x);
        for (int i = 0; i < 3; ++i) { dR[i * 3 + 0] = x[i]; dR[i * 3 + 1] = y[i]; dR[i * 3 + 2] = z[i]; }
    } else {
        float m[9];
        for (int i = 0; i < 9; ++i) m[i] = cnt > 0.f ? (float)acc[i] / fmaxf(cnt, 1.f) : (i % 4 == 0 ? 1.f : 0.f);
        // Gram-Schmidt on the columns (rotations.py:356-372)
        float a1[3] = {m[0], m[3], m[6]}, a2[3] = {m[1], m[4], m[7]}, a3[3] = {m[2], m[5], m[8]};
        float u2[3], u3[3];
        auto dot = [](const float *u, const float *v) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; };
        const float k12 = dot(a1, a2) / fmaxf(dot(a1, a1), 1e-8f);
        for (int i = 0; i < 3; ++i) u2[i] = a2[i] - k12 * a1[i];
        const float k13 = dot(a1, a3) / fmaxf(dot(a1, a1), 1e-8f);
        const float k23 = dot(u2, a3) / fmaxf(dot(u2, u2), 1e-8f);
        for (int i = 0; i < 3; ++i) u3[i] = (a3[i] - k13 * a1[i]) - k23 * u2[i];
        float c1[3], c2[3], c3[3];
        normalize3(a1, c1); normalize3(u2, c2); normalize3(u3, c3);
        for (int i = 0; i < 3; ++i) { dR[i * 3 + 0] = c1[i]; dR[i * 3 + 1] = c2[i]; dR[i * 3 + 2] = c3[i]; }
    }
    const float *Rp = prev_rot + (size_t)q * 9;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            float v = 0.f;
            for (int k = 0; k < 3; ++k) v += Rp[i * 3 + k] * dR[k * 3 + j];
            rot[(size_t)q * 9 + i * 3 + j] = v;
        }
    if (delta != nullptr)
        for (int i = 0; i < 9; ++i) delta[(size_t)q * 9 + i] = dR[i];
}

}  // namespace
