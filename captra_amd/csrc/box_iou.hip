// Box IoUs of the evaluation tables on the device (reference pose_utils/bbox_utils.py:11-61, 128-158; host restatement:
// captra_amd/pose_utils/bbox_utils.py iou_3d / nocs_iou_3d / get_pred_nocs_corners).
//
// Occupancy form (mode 0): for every (job, candidate) pair the nres^3 grid over the joint extent of the 16 corners, a point inside a
// box iff 0 < (p - c4).u < u.u for u = c5 - c4, c7 - c4, c0 - c4 (c7 - c4 is a face diagonal with the corner order of
// bbox_from_corners: the reference's protocol).  The grid coordinates are numpy.linspace's float32 values (linspace_coord below).
// A projection (dx ux + dy uy + dz uz) separates over the axes: every workgroup tabulates fl(fl(c - o) u) per box, u and axis in
// LDS (18 nres floats); a lane keeps the y + z part of its (j, k) columns' six projections in registers and walks the workgroup's x
// planes, one add and two compares per projection and point.  The compares land in lane masks, the two counts of a step are two
// scalar popcounts, one integer atomic per wave and count at the end: integer sums, so the counts do not depend on arrival order.
// The planes of a pair are split over gridDim.y workgroups; a second launch turns counts into the best IoU per job.
#include "common.h"

#define BI_THREADS 256
#define BI_MAX_NRES 128
#define BI_MAX_PARTS 64

// numpy.linspace(lo, hi, n)[i] for float32 end points, n >= 2: delta = fl(hi - lo), step = fl(delta / (n - 1)),
// y = fl(i * step) (fl(fl(i / (n - 1)) * delta) when the step underflowed to zero), fl(y + lo), the last one = hi.
__device__ __forceinline__ float linspace_coord(float lo, float hi, int n, int i) {
    if (i == n - 1) return hi;
    const float div = (float)(n - 1);
    const float delta = hi - lo;
    const float step = __fdiv_rn(delta, div);
    const float fi = (float)i;
    const float y = step != 0.0f ? fi * step : __fdiv_rn(fi, div) * delta;
    return y + lo;
}

struct BoxFrame {
    float o[3];      // corner 4
    float u[3][3];   // c5 - c4, c7 - c4, c0 - c4
    float uu[3];     // (ux ux + uy uy) + uz uz
};

__device__ __forceinline__ void load_frame(const float *__restrict__ box, BoxFrame &f) {
    const int far[3] = {5, 7, 0};
#pragma unroll
    for (int a = 0; a < 3; ++a) f.o[a] = box[4 * 3 + a];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
#pragma unroll
        for (int a = 0; a < 3; ++a) f.u[q][a] = box[far[q] * 3 + a] - f.o[a];
        f.uu[q] = (f.u[q][0] * f.u[q][0] + f.u[q][1] * f.u[q][1]) + f.u[q][2] * f.u[q][2];
    }
}

__global__ void box_iou_zero_kernel(long long n, int *__restrict__ counts) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) counts[i] = 0;
}

// grid (pairs, splits): workgroup (pair, s) takes x planes [s * planes, (s + 1) * planes)
__global__ __launch_bounds__(BI_THREADS) void box_iou_count_kernel(int ncand, int nres, int planes, const float *__restrict__ pred_box,
                                                                   const float *__restrict__ gt_box, int *__restrict__ counts) {
    __shared__ float tab[2][3][3][BI_MAX_NRES];      // [box][u][axis][i] = fl(fl(coord(axis, i) - o[axis]) * u[axis])
    const long long pair = blockIdx.x;
    const float *b1 = gt_box + pair * 24;            // order of the host call: fn(gt, pred)
    const float *b2 = pred_box + (pair / ncand) * 24;
    BoxFrame f[2];
    load_frame(b1, f[0]);
    load_frame(b2, f[1]);
    float lo[3], hi[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float l = b1[a], h = b1[a];
        for (int c = 1; c < 8; ++c) { l = fminf(l, b1[c * 3 + a]); h = fmaxf(h, b1[c * 3 + a]); }
        for (int c = 0; c < 8; ++c) { l = fminf(l, b2[c * 3 + a]); h = fmaxf(h, b2[c * 3 + a]); }
        lo[a] = l;
        hi[a] = h;
    }
    for (int t = threadIdx.x; t < 3 * nres; t += BI_THREADS) {
        const int a = t / nres, i = t - a * nres;
        const float l = a == 0 ? lo[0] : a == 1 ? lo[1] : lo[2], h = a == 0 ? hi[0] : a == 1 ? hi[1] : hi[2];
        const float c = linspace_coord(l, h, nres, i);
#pragma unroll
        for (int x = 0; x < 2; ++x) {
            const float o = a == 0 ? f[x].o[0] : a == 1 ? f[x].o[1] : f[x].o[2];
            const float d = c - o;
#pragma unroll
            for (int q = 0; q < 3; ++q) tab[x][q][a][i] = d * (a == 0 ? f[x].u[q][0] : a == 1 ? f[x].u[q][1] : f[x].u[q][2]);
        }
    }
    __syncthreads();
    const int i0 = blockIdx.y * planes;
    const int i1 = i0 + planes < nres ? i0 + planes : nres;
    const int columns = nres * nres;
    int inter = 0, uni = 0;                          // wave-uniform
    // every wave runs the same number of rounds with all lanes (a lane past the last column votes "outside")
    for (int base = 0; base < columns; base += BI_THREADS) {
        const int col = base + (int)threadIdx.x;
        const bool live = col < columns;
        const int j = live ? col / nres : 0, k = live ? col - j * nres : 0;
        float yz[2][3];
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int q = 0; q < 3; ++q) yz[x][q] = tab[x][q][1][j] + tab[x][q][2][k];
        const unsigned long long alive = __ballot(live);
        for (int i = i0; i < i1; ++i) {
            unsigned long long in[2];                // lane masks: the compares write them, the logic on them is scalar
#pragma unroll
            for (int x = 0; x < 2; ++x) {
                in[x] = alive;
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const float proj = tab[x][q][0][i] + yz[x][q];
                    in[x] &= __ballot(proj > 0.0f) & __ballot(proj < f[x].uu[q]);
                }
            }
            inter += __popcll(in[0] & in[1]);
            uni += __popcll(in[0] | in[1]);
        }
    }
    if (lane_id() == 0) {
        if (inter) atomicAdd(counts + pair * 2, inter);
        if (uni) atomicAdd(counts + pair * 2 + 1, uni);
    }
}

// IoU of the axis-aligned extents of two corner sets (nocs_iou_3d): fp32, products in axis order
__device__ __forceinline__ float extent_iou(const float *__restrict__ b1, const float *__restrict__ b2) {
    float e1[3], e2[3], ov[3];
    bool apart = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float l1 = b1[a], h1 = b1[a], l2 = b2[a], h2 = b2[a];
        for (int c = 1; c < 8; ++c) {
            l1 = fminf(l1, b1[c * 3 + a]); h1 = fmaxf(h1, b1[c * 3 + a]);
            l2 = fminf(l2, b2[c * 3 + a]); h2 = fmaxf(h2, b2[c * 3 + a]);
        }
        e1[a] = h1 - l1;
        e2[a] = h2 - l2;
        ov[a] = fminf(h1, h2) - fmaxf(l1, l2);
        apart = apart || ov[a] < 0.0f;
    }
    const float inter = apart ? 0.0f : (ov[0] * ov[1]) * ov[2];
    const float uni = ((e1[0] * e1[1]) * e1[2] + (e2[0] * e2[1]) * e2[2]) - inter;
    return __fdiv_rn(inter, uni);
}

// one thread per job: the best IoU over the candidates, the first one on ties (Python's max)
__global__ void box_iou_best_kernel(int njobs, int ncand, int mode, const float *__restrict__ pred_box, const float *__restrict__ gt_box,
                                    const int *__restrict__ counts, float *__restrict__ iou) {
    const int job = blockIdx.x * blockDim.x + threadIdx.x;
    if (job >= njobs) return;
    float best = 0.0f;
    for (int c = 0; c < ncand; ++c) {
        const long long pair = (long long)job * ncand + c;
        float v;
        if (mode == 0) {
            const int inter = counts[pair * 2], uni = counts[pair * 2 + 1];
            v = uni == 0 ? 1.0f : __fdiv_rn((float)inter, (float)uni);      // no sample inside either box: the reference's "both empty" = 1
        } else {
            v = extent_iou(gt_box + pair * 24, pred_box + (long long)job * 24);
        }
        if (c == 0 || v > best) best = v;
    }
    iou[job] = best;
}

extern "C" int captra_box_iou(int njobs, int ncand, int mode, int nres, const float *pred_box, const float *gt_box, float *iou, int *counts,
                              captra_stream_t stream) {
    if (njobs < 0 || ncand < 1 || (mode != 0 && mode != 1)) return -1;
    if (njobs == 0) return 0;
    if (pred_box == nullptr || gt_box == nullptr || iou == nullptr) return -1;
    const hipStream_t st = (hipStream_t)stream;
    const long long pairs = (long long)njobs * ncand;
    if (pairs > 0x7fffffffLL) return -2;
    if (mode == 0) {
        if (nres < 2 || counts == nullptr) return -1;
        if (nres > BI_MAX_NRES) return -2;
        // a pair's planes over several workgroups while the pairs alone do not fill the chip (about four workgroups per CU)
        long long want = (1024 + pairs - 1) / pairs;
        want = want < 1 ? 1 : (want > nres ? nres : want);
        const int planes = (int)((nres + want - 1) / want);
        const int splits = (nres + planes - 1) / planes;
        CAPTRA_LAUNCH("box_iou_zero", box_iou_zero_kernel, dim3((unsigned)((pairs * 2 + 255) / 256)), dim3(256), 0, st, pairs * 2, counts);
        CAPTRA_LAUNCH("box_iou_count", box_iou_count_kernel, dim3((unsigned)pairs, splits), dim3(BI_THREADS), 0, st, ncand, nres, planes,
                      pred_box, gt_box, counts);
    }
    CAPTRA_LAUNCH("box_iou_best", box_iou_best_kernel, dim3((njobs + 255) / 256), dim3(256), 0, st, njobs, ncand, mode, pred_box, gt_box,
                  counts, iou);
    return captra_last_error();
}

// One workgroup per cloud: per part the largest |x|, |y|, |z| over the points that carry its label.  |v| >= 0, so the order of the
// floats is the order of their bit patterns and an unsigned integer max in LDS gives the exact maximum in any arrival order.
__global__ __launch_bounds__(BI_THREADS) void part_extent_kernel(int p, int n, const int *__restrict__ labels, const float *__restrict__ nocs,
                                                                 float *__restrict__ out) {
    __shared__ unsigned size[BI_MAX_PARTS * 3];
    __shared__ unsigned seen[BI_MAX_PARTS];
    for (int t = threadIdx.x; t < p * 3; t += BI_THREADS) size[t] = 0u;
    for (int t = threadIdx.x; t < p; t += BI_THREADS) seen[t] = 0u;
    __syncthreads();
    const long long cloud = blockIdx.x;
    const int *lab = labels + cloud * n;
    const float *x = nocs + cloud * n * 3;
    for (int t = threadIdx.x; t < n; t += BI_THREADS) {
        const int l = lab[t];
        if (l < 0 || l >= p) continue;
        seen[l] = 1u;                                 // every writer stores the same value
#pragma unroll
        for (int a = 0; a < 3; ++a) atomicMax(&size[l * 3 + a], __float_as_uint(fabsf(x[(long long)t * 3 + a])));
    }
    __syncthreads();
    for (int t = threadIdx.x; t < p * 3; t += BI_THREADS) {
        const int l = t / 3, a = t - l * 3;
        const float s = __uint_as_float(size[t]);
        float *o = out + (cloud * p + l) * 6;
        o[a] = seen[l] ? -s : 0.0f;
        o[3 + a] = seen[l] ? s : 0.0f;
    }
}

extern "C" int captra_part_extent(int b, int p, int n, const int *labels, const float *nocs, float *out, captra_stream_t stream) {
    if (b < 0 || p < 1 || n < 0) return -1;
    if (p > BI_MAX_PARTS) return -2;
    if (b == 0) return 0;
    if (out == nullptr || (n > 0 && (labels == nullptr || nocs == nullptr))) return -1;
    CAPTRA_LAUNCH("part_extent", part_extent_kernel, dim3(b), dim3(BI_THREADS), 0, (hipStream_t)stream, p, n, labels, nocs, out);
    return captra_last_error();
}
