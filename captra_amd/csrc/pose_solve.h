// The 3x3 orthogonal Procrustes solve shared by pose_fit.hip (captra_procrustes_rot3) and the RANSAC fit (pose_ransac.h:
// captra_part_fit_ransac, captra_part_fit_guard): double-precision cyclic Jacobi on M^T M, and the rotation
// U diag(1,1,det(UV^T)) V^T read off its eigenvectors.  The ONE inlier test of the RANSAC fit and the track guard.  And the scale /
// translation algebra under a known rotation (ps_*), shared by part_fit_st_kernel, rs_umeyama and RsGivenRot.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

// |t - (sR s + tr)|^2 under the twelve parameters hp = (sR row-major, tr), every operation a separately rounded fp32 one
static __device__ __forceinline__ float rs_residual2(const float s[3], const float t[3], const float hp[12]) {
    float e[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float pr = ((hp[a * 3] * s[0] + hp[a * 3 + 1] * s[1]) + hp[a * 3 + 2] * s[2]) + hp[9 + a];
        e[a] = t[a] - pr;
    }
    return (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
}
// ... < th2; a NaN residual is no inlier
static __device__ __forceinline__ bool rs_inlier(const float s[3], const float t[3], const float hp[12], float th2) {
    return rs_residual2(s, t, hp) < th2;
}

// The AXIS-ONLY test of the symmetric categories (include/captra_hip.h, captra_part_fit_guard_sym): the camera point lies where the
// NOCS point's height and radius put it on the surface of revolution about the pose's y-axis; no in-plane angle enters.  Seven
// parameters ap = (a = second column of rot, scale, trans); rho = rs_sym_radius(s) depends on the member alone, so a caller that
// meets a member under many poses forms it once.  w = d - h a and not |d|^2 - h^2: the latter cancels near the axis.
static __device__ __forceinline__ float rs_sym_radius(const float s[3]) { return sqrtf(s[0] * s[0] + s[2] * s[2]); }
static __device__ __forceinline__ float rs_residual2_sym(float sy, float rho, const float t[3], const float ap[7]) {
    const float d0 = t[0] - ap[4], d1 = t[1] - ap[5], d2 = t[2] - ap[6];
    const float h = (ap[0] * d0 + ap[1] * d1) + ap[2] * d2;
    const float w0 = d0 - h * ap[0], w1 = d1 - h * ap[1], w2 = d2 - h * ap[2];
    const float rt = sqrtf((w0 * w0 + w1 * w1) + w2 * w2);
    const float eh = h - ap[3] * sy, er = rt - ap[3] * rho;
    return eh * eh + er * er;
}

// The test a kernel instantiated with SYM applies, and how many of a hypothesis's twelve-float slot it reads: the full-rotation
// test on (sR, t), or the axis-only one on (a, scale, t).  rho is read with SYM alone.
template <bool SYM>
struct RsTest {
    static constexpr int NPAR = SYM ? 7 : 12;
    static __device__ __forceinline__ float residual2(const float s[3], float rho, const float t[3], const float *hp) {
        if constexpr (SYM) return rs_residual2_sym(s[1], rho, t, hp);
        else return rs_residual2(s, t, hp);
    }
    static __device__ __forceinline__ bool inlier(const float s[3], float rho, const float t[3], const float *hp, float th2) {
        if constexpr (SYM) return rs_residual2_sym(s[1], rho, t, hp) < th2;      // (a NaN residual is no inlier)
        else return rs_inlier(s, t, hp, th2);
    }
};

// ---- the scale / translation algebra of a fit whose rotation is known (pose_fit.hip's header), in double, on the centred moments
// M[a][c] = sum tc_a sc_c and C6 = sum sc sc^T (xx xy xz yy yz zz) and the centroids sb / tb.
// The in-plane rotation about y of the symmetric categories: the 2-D fit on the (x,z) block of R0^T M is the rotation by
// atan2(M10 - M01, M00 + M11) (h = 0: the identity; a NaN propagates); R = R0 embed_y(that)
static __device__ __forceinline__ void ps_rot_about_y(const double R0[9], const double M[9], double R[9]) {
    double M2[4];
    const int ax[2] = {0, 2};
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) {
            double acc = 0;
            for (int k = 0; k < 3; ++k) acc += R0[k * 3 + ax[i]] * M[k * 3 + ax[j]];
            M2[i * 2 + j] = acc;
        }
    const double a = M2[0] + M2[3], c = M2[2] - M2[1];
    const double h = sqrt(a * a + c * c);
    double cs = 1.0, sn = 0.0;
    if (h > 0.0) {
        cs = a / h;
        sn = c / h;
    } else if (h != h) {
        cs = sn = NAN;
    }
    const double R3[9] = {cs, 0, -sn, 0, 1, 0, sn, 0, cs};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double acc = 0;
            for (int k = 0; k < 3; ++k) acc += R0[i * 3 + k] * R3[k * 3 + j];
            R[i * 3 + j] = acc;
        }
}
// s = <R, M> / (<R^T R, Css> + 1e-6) = sum (R sc).tc / (sum |R sc|^2 + 1e-6): the denominator with the actual R (the reference rotates
// first, then squares, so a non-orthonormal R is honoured)
static __device__ __forceinline__ double ps_scale(const double R[9], const double M[9], const double C6[6]) {
    double num = 0;
    for (int i = 0; i < 9; ++i) num += R[i] * M[i];
    const double Css[9] = {C6[0], C6[1], C6[2], C6[1], C6[3], C6[4], C6[2], C6[4], C6[5]};
    double dn = 0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double g = 0;  // (R^T R)_ij
            for (int k = 0; k < 3; ++k) g += R[k * 3 + i] * R[k * 3 + j];
            dn += g * Css[i * 3 + j];
        }
    return num / (dn + 1e-6);
}
// t = tb - s R sb = mean(tgt - s R src)
static __device__ __forceinline__ void ps_trans(const double R[9], double s, const double sb[3], const double tb[3], double tr[3]) {
    for (int a = 0; a < 3; ++a) tr[a] = tb[a] - s * (R[a * 3] * sb[0] + R[a * 3 + 1] * sb[1] + R[a * 3 + 2] * sb[2]);
}

static __device__ void jacobi_eig3(double A[9], double V[9]) {
    for (int i = 0; i < 9; ++i) V[i] = (i % 4 == 0) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 30; ++sweep) {
        const double off = A[1] * A[1] + A[2] * A[2] + A[5] * A[5];
        if (off < 1e-300) break;
        for (int pq = 0; pq < 3; ++pq) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            const double apq = A[p * 3 + q];
            if (fabs(apq) < 1e-300) continue;
            const double theta = (A[q * 3 + q] - A[p * 3 + p]) / (2.0 * apq);
            const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
            for (int k = 0; k < 3; ++k) {
                const double akp = A[k * 3 + p], akq = A[k * 3 + q];
                A[k * 3 + p] = c * akp - s * akq;
                A[k * 3 + q] = s * akp + c * akq;
            }
            for (int k = 0; k < 3; ++k) {
                const double apk = A[p * 3 + k], aqk = A[q * 3 + k];
                A[p * 3 + k] = c * apk - s * aqk;
                A[q * 3 + k] = s * apk + c * aqk;
            }
            for (int k = 0; k < 3; ++k) {
                const double vkp = V[k * 3 + p], vkq = V[k * 3 + q];
                V[k * 3 + p] = c * vkp - s * vkq;
                V[k * 3 + q] = s * vkp + c * vkq;
            }
        }
    }
}

// R = [u1 u2 u1xu2][v1 v2 v1xv2]^T with v1,v2 the leading eigenvectors of M^T M, u_i = M v_i/|M v_i|:
// equals U diag(1,1,det(UV^T)) V^T for either sign of det(M) (see oracle/captra_oracle.c).
// Rank <= 1 (collinear or coincident points, one point, no point): M v2 (and for M = 0 also M v1) is zero, u2 = M v2/|M v2|
// would be 0/0 -- u is completed with an arbitrary orthonormal vector instead, the identity for M = 0.  sigma_2 counts as zero
// below KABSCH_RANK1_REL * sigma_1: there M v2 holds nothing but the rounding of the double arithmetic (~1e-16 sigma_1), and
// a sigma_2 that small moves the objective tr(R^T M) by 1e-12 sigma_1, four orders below the fp32 rounding of R.
constexpr double KABSCH_RANK1_REL = 1e-12;
static __device__ void kabsch3(const double M[9], double R[9]) {
    double A[9], V[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double acc = 0;
            for (int k = 0; k < 3; ++k) acc += M[k * 3 + i] * M[k * 3 + j];
            A[i * 3 + j] = acc;
        }
    jacobi_eig3(A, V);
    const double ev[3] = {A[0], A[4], A[8]};
    int o0 = 0, o1 = 1, o2 = 2;
    if (ev[o1] > ev[o0]) { int t = o0; o0 = o1; o1 = t; }
    if (ev[o2] > ev[o0]) { int t = o0; o0 = o2; o2 = t; }
    if (ev[o2] > ev[o1]) { int t = o1; o1 = o2; o2 = t; }
    double v1[3], v2[3], v3[3], u1[3], u2[3], u3[3];
    for (int k = 0; k < 3; ++k) {
        v1[k] = V[k * 3 + o0];
        v2[k] = V[k * 3 + o1];
    }
    v3[0] = v1[1] * v2[2] - v1[2] * v2[1];
    v3[1] = v1[2] * v2[0] - v1[0] * v2[2];
    v3[2] = v1[0] * v2[1] - v1[1] * v2[0];
    double n1 = 0, n2 = 0;
    for (int i = 0; i < 3; ++i) {
        u1[i] = M[i * 3] * v1[0] + M[i * 3 + 1] * v1[1] + M[i * 3 + 2] * v1[2];
        u2[i] = M[i * 3] * v2[0] + M[i * 3 + 1] * v2[1] + M[i * 3 + 2] * v2[2];
        n1 += u1[i] * u1[i];
        n2 += u2[i] * u2[i];
    }
    n1 = sqrt(n1);  // sigma_1
    n2 = sqrt(n2);  // sigma_2
    if (n1 == 0.0) {  // M = 0: every rotation is optimal -- the identity
        for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
        return;
    }
    double dp = 0;
    for (int i = 0; i < 3; ++i) u1[i] /= n1;
    if (n2 <= KABSCH_RANK1_REL * n1) {
        // rank 1: M v2 is zero or rounding noise, and every unit vector orthogonal to u1 completes an optimal rotation
        // (tr(R^T M) = sigma_1 for all of them) -- take the coordinate axis farthest from u1; the Gram-Schmidt step below
        // makes it orthonormal (|e_k - u1_k u1|^2 = 1 - u1_k^2 >= 2/3)
        int k = 0;
        if (fabs(u1[1]) < fabs(u1[k])) k = 1;
        if (fabs(u1[2]) < fabs(u1[k])) k = 2;
        for (int i = 0; i < 3; ++i) u2[i] = (i == k) ? 1.0 : 0.0;
    } else {
        for (int i = 0; i < 3; ++i) u2[i] /= n2;
    }
    for (int i = 0; i < 3; ++i) dp += u1[i] * u2[i];
    double nn = 0;
    for (int i = 0; i < 3; ++i) {
        u2[i] -= dp * u1[i];
        nn += u2[i] * u2[i];
    }
    nn = sqrt(nn);
    for (int i = 0; i < 3; ++i) u2[i] /= nn;
    u3[0] = u1[1] * u2[2] - u1[2] * u2[1];
    u3[1] = u1[2] * u2[0] - u1[0] * u2[2];
    u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[i * 3 + j] = u1[i] * v1[j] + u2[i] * v2[j] + u3[i] * v3[j];
}
