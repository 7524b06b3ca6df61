// Held box: per (trajectory, part) a histogram of |NOCS coordinate| per axis, accumulated over the track, and the quantile read out of
// it -- on device for gfx950, one launch behind the guard in the step's sequence.  No reference counterpart: the reference takes the
// largest |x|, |y|, |z| of every frame by itself (captra_part_extent).  Semantics: include/captra_hip.h, captra_part_box_hist.
//
// One WORKGROUP of 256 threads per (b, q).  The frame's histogram is built in LDS with integer atomics -- a few thousand members that
// fall into a handful of bins: the launch is bound by same-address LDS atomics and by its own latency, not by the 200 KB it reads --,
// either in ONE histogram all four waves add into or in one per wave (BX_SUB; captra_part_box_set_subhists picks, DESIGN.md §3.3 has
// the measurement).  The accumulation is one pass of 3 bins threads' worth of 64-bit adds, the six quantile read-outs (three axes of
// the held and of the frame's histogram) one wave each: a 64-bit prefix sum over the lanes' runs of bins and a wave minimum.
// Everything is integer arithmetic or an exact fp32 operation: no result depends on the order of the members.
#include <hip/hip_runtime.h>
#include <math.h>

#include "captra_hip.h"
#include "common.h"
#include "pose_ransac.h"
#include "wave_ops.h"

namespace {

constexpr int BX_THREADS = 256;
constexpr int BX_WAVES = BX_THREADS / 64;
constexpr int BX_MAX_BINS = 512;
constexpr int BX_UNROLL = 4;                // points per thread in flight (N = 4096: all of a thread's sixteen loads in four rounds)
constexpr long long BX_INT_MAX = 0x7fffffffLL;

CAPTRA_KNOB int g_box_subhists = 0;         // 0 = the default (BX_DEFAULT_SUB), else 1 or BX_WAVES
constexpr int BX_DEFAULT_SUB = 1;

// the bin of a per-axis value a >= 0 (or not finite): exact, bins is a power of two and a < 1 where the product is taken
__device__ __forceinline__ int bx_bin(float a, int bins) { return (a >= 1.0f || !isfinite(a)) ? bins - 1 : (int)(a * (float)bins); }

// r = sqrt(x x + z z) in fp32, one rounding per operation: the bits numpy's float32 arithmetic gives.  The root through double: the
// double root of an fp32 value rounded to fp32 IS the correctly rounded fp32 root (53 >= 2 * 24 + 2 bits), whereas __fsqrt_rn
// compiles to the bare v_sqrt_f32 here, which is good to one ulp only -- 0.5 would come out of (0.3, 0.4) one bin too low.
__device__ __forceinline__ float bx_radius(float x, float z) {
    const float s = __fadd_rn(__fmul_rn(x, x), __fmul_rn(z, z));
    return (float)sqrt((double)s);
}

// The quantile read-out of one axis' histogram h[0..bins) by ONE wave: lane l owns the bins [l per, (l + 1) per), per = bins / 64.
// -> the extent (0 when the histogram holds fewer than min_points), *total = the histogram's sum; uniform over the wave.
__device__ __forceinline__ float bx_read_out(const int *h, int bins, int permille, int min_points, long long *total) {
    const int lane = lane_id(), per = bins >> 6;
    long long own = 0;
    for (int j = 0; j < per; ++j) own += (long long)h[lane * per + j];
    long long incl = own;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long up = __shfl_up(incl, d);
        if (lane >= d) incl = incl + up;
    }
    const long long T = __shfl(incl, 63);
    *total = T;
    if (T < (long long)min_points) return 0.0f;
    const long long need = (T * (long long)permille + 999LL) / 1000LL;
    long long cum = incl - own;
    unsigned found = 0xffffffffu;
    for (int j = 0; j < per; ++j) {
        cum += (long long)h[lane * per + j];
        if (found == 0xffffffffu && cum >= need) found = (unsigned)(lane * per + j);
    }
    const unsigned jstar = wave_min_u32(found);
    return (float)(jstar + 1u) / (float)bins;
}

template <int SUB>
__global__ __launch_bounds__(BX_THREADS) void part_box_hist_kernel(int p, int n, int bins, int radial, int permille, int min_points,
                                                                   const int *__restrict__ labels, const float *__restrict__ src,
                                                                   const int *__restrict__ verdict, const int *hist_in, int *hist_out,
                                                                   float *__restrict__ extent, float *__restrict__ frame_extent,
                                                                   int *__restrict__ added, int *__restrict__ total) {
    __shared__ int frame[SUB][3 * BX_MAX_BINS];     // the frame's histogram F (after the combine: frame[0])
    __shared__ int held[3 * BX_MAX_BINS];           // hist_out
    const int bq = blockIdx.x, b = bq / p, q = bq - b * p;
    const int tid = threadIdx.x, wave = tid >> 6;
    const int cells = 3 * bins;
    for (int s = 0; s < SUB; ++s)
        for (int c = tid; c < cells; c += BX_THREADS) frame[s][c] = 0;
    __syncthreads();

    int *mine = frame[SUB == 1 ? 0 : wave];
    const int *lab = labels + (size_t)b * n;
    const float *sx = src + (size_t)bq * 3 * n, *sy = sx + n, *sz = sy + n;
    // the label and the three coordinates of a point are loaded together, a non-member's too: four dependent round trips to memory
    // per point otherwise, and the launch is all latency
    // per point otherwise, and the launch is all latency.  BX_UNROLL points per thread are in flight at once; the empty asm keeps
    // the compiler from sinking a load behind the test of the value loaded before it.
    for (int i0 = tid; i0 < n; i0 += BX_THREADS * BX_UNROLL) {
        int l[BX_UNROLL];
        float x[BX_UNROLL], y[BX_UNROLL], z[BX_UNROLL];
#pragma unroll
        for (int u = 0; u < BX_UNROLL; ++u) {
            const int i = i0 + u * BX_THREADS;
            const int ic = i < n ? i : n - 1;           // (in bounds; the copy of the last point is not counted)
            l[u] = i < n ? lab[ic] : -1;
            x[u] = sx[ic], y[u] = sy[ic], z[u] = sz[ic];
        }
#pragma unroll
        for (int u = 0; u < BX_UNROLL; ++u) asm volatile("" : "+v"(l[u]), "+v"(x[u]), "+v"(y[u]), "+v"(z[u]));
#pragma unroll
        for (int u = 0; u < BX_UNROLL; ++u) {
            const bool member = l[u] == q && isfinite(x[u]) && isfinite(y[u]) && isfinite(z[u]);
            if (!member) continue;
            float a0 = fabsf(x[u]), a2 = fabsf(z[u]);
            const float a1 = fabsf(y[u]);
            if (radial) a0 = a2 = bx_radius(x[u], z[u]);
            atomicAdd(&mine[bx_bin(a0, bins)], 1);
            atomicAdd(&mine[bins + bx_bin(a1, bins)], 1);
            atomicAdd(&mine[2 * bins + bx_bin(a2, bins)], 1);
        }
    }
    __syncthreads();

    // F = the sub-histograms' sum; hist_out = min(max(hist_in, 0) + F, 2^31 - 1) where the guard's verdict lets the frame in.
    // (hist_out may be hist_in: a cell is read and written by one thread)
    const int verd = verdict != nullptr ? verdict[bq] : 0;
    const bool accumulate = verd == 0 || verd == 3;
    const size_t base = (size_t)bq * cells;
    for (int c = tid; c < cells; c += BX_THREADS) {
        int f = frame[0][c];
#pragma unroll
        for (int s = 1; s < SUB; ++s) f += frame[s][c];
        long long h = 0;
        if (hist_in != nullptr) {
            const int v = hist_in[base + c];
            h = v > 0 ? (long long)v : 0LL;
        }
        if (accumulate) h += (long long)f;
        const int out = (int)(h < BX_INT_MAX ? h : BX_INT_MAX);
        if (SUB > 1) frame[0][c] = f;
        held[c] = out;
        hist_out[base + c] = out;
    }
    __syncthreads();

    // six read-outs, one wave each: t = 0..2 the held histogram's axes, 3..5 the frame's
    for (int t = wave; t < 6; t += BX_WAVES) {
        const int k = t % 3;
        const bool of_frame = t >= 3;
        long long T;
        const float e = bx_read_out((of_frame ? frame[0] : held) + k * bins, bins, permille, min_points, &T);
        if ((tid & 63) == 0) {
            (of_frame ? frame_extent : extent)[(size_t)bq * 3 + k] = e;
            if (k == 0) (of_frame ? added : total)[bq] = (int)(T < BX_INT_MAX ? T : BX_INT_MAX);
        }
    }
}

}  // namespace

extern "C" void captra_part_box_set_subhists(int sub) { g_box_subhists = (sub == 1 || sub == BX_WAVES) ? sub : 0; }

extern "C" int captra_part_box_hist(int b, int p, int n, int bins, int radial, int quantile_permille, int min_points, const int *labels,
                                    const float *src, const int *verdict, const int *hist_in, int *hist_out, float *extent,
                                    float *frame_extent, int *added, int *total, captra_stream_t stream) {
    if (b < 1 || p < 1 || p > RS_MAX_P || n < 1) return -1;
    if (bins != 64 && bins != 128 && bins != 256 && bins != 512) return -1;
    if (quantile_permille < 500 || quantile_permille > 1000 || min_points < 1) return -1;
    if ((long long)b * p > BX_INT_MAX / (3 * BX_MAX_BINS)) return -1;
    if (labels == nullptr || src == nullptr || hist_out == nullptr || extent == nullptr || frame_extent == nullptr || added == nullptr ||
        total == nullptr)
        return -1;
    const int sub = g_box_subhists != 0 ? g_box_subhists : BX_DEFAULT_SUB;
    const dim3 grid(b * p), block(BX_THREADS);
    if (sub == 1)
        CAPTRA_LAUNCH("part_box_hist", part_box_hist_kernel<1>, grid, block, 0, (hipStream_t)stream, p, n, bins, radial, quantile_permille,
                      min_points, labels, src, verdict, hist_in, hist_out, extent, frame_extent, added, total);
    else
        CAPTRA_LAUNCH("part_box_hist", part_box_hist_kernel<BX_WAVES>, grid, block, 0, (hipStream_t)stream, p, n, bins, radial,
                      quantile_permille, min_points, labels, src, verdict, hist_in, hist_out, extent, frame_extent, added, total);
    return captra_last_error();
}
