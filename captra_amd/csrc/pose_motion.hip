// Motion model: the pose frame i+1 starts from, extrapolated with constant velocity from the results of frames i-1 and i -- per
// (trajectory, part), on device for gfx950, the last launch of the step's sequence.  No reference counterpart: the reference's
// frame i+1 starts from the result of frame i.  Semantics: include/captra_hip.h, captra_pose_extrapolate.
//
// One THREAD per (b, p): 24 floats in, 12 out, a few dozen double operations -- a (b, p) has nothing to share, so no LDS, no
// atomics, no cross-lane traffic; B * P threads in ceil(B P / 64) one-wave workgroups.  Every value is computed in double on the
// fp32 inputs as stored and rounded to fp32 once; the gates compare the doubles, not their fp32 roundings.
#include <hip/hip_runtime.h>
#include <math.h>

#include "captra_hip.h"
#include "common.h"

namespace {

constexpr int PM_THREADS = 64;
constexpr double PM_RAD2DEG = 57.29577951308232087680;      // 180 / pi

__global__ __launch_bounds__(PM_THREADS) void pose_extrapolate_kernel(int total, int sym, const float *__restrict__ rot0,
                                                                      const float *__restrict__ trans0, const float *__restrict__ rot1,
                                                                      const float *__restrict__ trans1, const int *__restrict__ measured0,
                                                                      const int *__restrict__ verdict, double gain, double max_angle_deg,
                                                                      double max_shift, float *__restrict__ rot_next,
                                                                      float *__restrict__ trans_next, int *__restrict__ measured1,
                                                                      int *__restrict__ used_out, float *__restrict__ angle_out,
                                                                      float *__restrict__ shift_out) {
    const int q = blockIdx.x * PM_THREADS + threadIdx.x;
    if (q >= total) return;
    float r0f[9], r1f[9], t0f[3], t1f[3];
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        r0f[i] = rot0[(size_t)q * 9 + i];
        r1f[i] = rot1[(size_t)q * 9 + i];
        finite = finite && isfinite(r0f[i]) && isfinite(r1f[i]);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        t0f[a] = trans0[(size_t)q * 3 + a];
        t1f[a] = trans1[(size_t)q * 3 + a];
        finite = finite && isfinite(t0f[a]) && isfinite(t1f[a]);
    }
    const int verd = verdict != nullptr ? verdict[q] : 0;

    double R1[9] = {}, d[3] = {}, v[3] = {}, c = 0.0, vn = 0.0, theta = 0.0, angle = 0.0, shift = 0.0;
    if (finite) {
        double R0[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            R0[i] = (double)r0f[i];
            R1[i] = (double)r1f[i];
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) d[a] = (double)t1f[a] - (double)t0f[a];
        shift = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
        if (sym) {          // the image of the object's y-axis: the second column
            const double a0[3] = {R0[1], R0[4], R0[7]}, a1[3] = {R1[1], R1[4], R1[7]};
            v[0] = a0[1] * a1[2] - a0[2] * a1[1];
            v[1] = a0[2] * a1[0] - a0[0] * a1[2];
            v[2] = a0[0] * a1[1] - a0[1] * a1[0];
            c = (a0[0] * a1[0] + a0[1] * a1[1]) + a0[2] * a1[2];
        } else {            // D = rot1 rot0^T: D[i][j] = sum_k R1[i][k] R0[j][k]
            double D[9];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    D[i * 3 + j] = (R1[i * 3 + 0] * R0[j * 3 + 0] + R1[i * 3 + 1] * R0[j * 3 + 1]) + R1[i * 3 + 2] * R0[j * 3 + 2];
            v[0] = 0.5 * (D[7] - D[5]);
            v[1] = 0.5 * (D[2] - D[6]);
            v[2] = 0.5 * (D[3] - D[1]);
            c = 0.5 * (((D[0] + D[4]) + D[8]) - 1.0);
        }
        vn = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
        theta = atan2(vn, c);
        angle = theta * PM_RAD2DEG;
    }
    const bool use = measured0[q] != 0 && finite && verd == 0 && angle <= max_angle_deg && shift <= max_shift;

    measured1[q] = (finite && (verd == 0 || verd == 3)) ? 1 : 0;
    used_out[q] = use ? 1 : 0;
    angle_out[q] = (float)angle;
    shift_out[q] = (float)shift;

    if (!use) {             // the pass-through never invents a value: rot1 / trans1 bit for bit, non-finite ones included
#pragma unroll
        for (int i = 0; i < 9; ++i) rot_next[(size_t)q * 9 + i] = r1f[i];
#pragma unroll
        for (int a = 0; a < 3; ++a) trans_next[(size_t)q * 3 + a] = t1f[a];
        return;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) trans_next[(size_t)q * 3 + a] = (float)((double)t1f[a] + gain * d[a]);
    if (vn == 0.0) {        // bit-equal rotations (or a step about no axis): the rotation part is rot1's bits
#pragma unroll
        for (int i = 0; i < 9; ++i) rot_next[(size_t)q * 9 + i] = r1f[i];
        return;
    }
    // Q = I + sin(phi) K + (1 - cos(phi)) K^2, K the cross-product matrix of k = v / |v|
    const double k[3] = {v[0] / vn, v[1] / vn, v[2] / vn};
    const double phi = gain * theta, s = sin(phi), omc = 1.0 - cos(phi);
    const double K[9] = {0.0, -k[2], k[1], k[2], 0.0, -k[0], -k[1], k[0], 0.0};
    double Q[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double k2 = (K[i * 3 + 0] * K[0 * 3 + j] + K[i * 3 + 1] * K[1 * 3 + j]) + K[i * 3 + 2] * K[2 * 3 + j];
            Q[i * 3 + j] = ((i == j ? 1.0 : 0.0) + s * K[i * 3 + j]) + omc * k2;
        }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            rot_next[(size_t)q * 9 + i * 3 + j] = (float)((Q[i * 3 + 0] * R1[0 * 3 + j] + Q[i * 3 + 1] * R1[1 * 3 + j]) + Q[i * 3 + 2] * R1[2 * 3 + j]);
}

}  // namespace

extern "C" int captra_pose_extrapolate(int b, int p, int sym, const float *rot0, const float *trans0, const float *rot1, const float *trans1,
                                       const int *measured0, const int *verdict, float gain, float max_angle_deg, float max_shift,
                                       float *rot_next, float *trans_next, int *measured1, int *used, float *angle, float *shift,
                                       captra_stream_t stream) {
    if (b < 1 || p < 1 || p > 8 || (sym != 0 && sym != 1)) return -1;
    if ((long long)b * p > 0x7fffffffLL / 9) return -1;
    if (!(gain > 0.f && gain <= 1.f) || !(max_angle_deg > 0.f && max_angle_deg <= 90.f) || !(max_shift > 0.f && isfinite(max_shift))) return -1;
    if (rot0 == nullptr || trans0 == nullptr || rot1 == nullptr || trans1 == nullptr || measured0 == nullptr || rot_next == nullptr ||
        trans_next == nullptr || measured1 == nullptr || used == nullptr || angle == nullptr || shift == nullptr)
        return -1;
    const int total = b * p;
    CAPTRA_LAUNCH("pose_extrapolate", pose_extrapolate_kernel, dim3((total + PM_THREADS - 1) / PM_THREADS), dim3(PM_THREADS), 0,
                  (hipStream_t)stream, total, sym, rot0, trans0, rot1, trans1, measured0, verdict, (double)gain, (double)max_angle_deg,
                  (double)max_shift, rot_next, trans_next, measured1, used, angle, shift);
    return captra_last_error();
}
