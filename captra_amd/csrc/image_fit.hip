// The correspondences of a first-pose fit from frame 0's images, for gfx950 (include/captra_hip.h: captra_image_members, where the rule
// is stated in full): the pixels of an eroded instance mask that carry a depth, in row-major order, subsampled to at most `cap` by a
// fixed stride, each back-projected (captra_crop_ball's float64 arithmetic) and paired with the NOCS coordinate its pixel of the
// coordinate image encodes -- the first half of the reference's get_image_pose (datasets/nocs_data/preproc_nocs/get_gt_poses.py:20-34,
// nocs_utils.py:5-33 `backproject`, 44-54 `remove_border`), in the layouts captra_part_fit_ransac reads.
//
// Which slot a member lands in depends on the members in front of it AND on the image's total (the stride), so an image is counted
// before it is written.  ONE launch, `split` workgroups per image, no scratch memory:
//   pass 1  every workgroup of an image counts the WHOLE image -- the members in front of its own share, the members and the holes of
//           the image.  The count reads the mask alone, 16 bytes per lane and four such vectors in flight, and looks further (window,
//           depth) only where a vector holds a set byte -- then for its sixteen pixels at once, without a branch, so that the loads go
//           out together: an instance covers a few per cent of a frame, so the pass costs a workgroup one read of 0.3 MB (480 x 640)
//           that the other workgroups of the image find in the cache.  Sums of integers: any order gives the same numbers.
//           The pass is REDUNDANT by the split, and it is what the launch costs (111 us on 32 frames against 12
//           for a copy); per-workgroup counts in a scratch buffer would remove it, and the call has no workspace argument.
//   pass 2  the workgroup walks its own share of the flat pixel range 1024 pixels at a time and compacts the members in order (wave
//           ballot + LDS wave offsets, as csrc/crop.hip); member j goes to slot j / step when j % step == 0.
// One workgroup per image (split = 1) leaves most of the device idle on a batch of 32; the launcher spreads an image over as many
// workgroups as fill the device twice (captra_image_members_set_split overrides it: the result does not depend on it).
#include "common.h"

#include <limits.h>

namespace {

constexpr int IM_T = 1024;

struct ImImage {
    const int *depth;
    const unsigned char *mask;
    int h, w, border;
};

// pixel (r,c) = flat pixel t: 0 = not inside the eroded mask, 1 = a member, 2 = a hole (inside, depth <= 0); d = its depth.  Without a
// branch: the window's loads -- coordinates clamped into the image, which repeats pixels of the clipped window (it holds (r,c) itself
// for border >= 1) and so changes no verdict -- and the depth's go out together, one round trip instead of one per test.  border = 0:
// the empty window, the pixel's own byte (`set`) decides.
__device__ __forceinline__ int im_classify(const ImImage &im, int t, int r, int c, bool set, int &d) {
    bool inside = set;
    for (int dr = 1 - im.border; dr <= im.border; ++dr) {
        const int rr = r + dr < 0 ? 0 : (r + dr < im.h ? r + dr : im.h - 1);
        for (int dc = 1 - im.border; dc <= im.border; ++dc) {
            const int cc = c + dc < 0 ? 0 : (c + dc < im.w ? c + dc : im.w - 1);
            inside = inside & (im.mask[(size_t)rr * im.w + cc] != 0);
        }
    }
    d = im.depth[t];
    return inside ? (d > 0 ? 1 : 2) : 0;
}

// CAM (captra_image_members_cam; include/captra_hip.h, "The CAMERA MODEL"): Kinv and the depth unit of image i are those of row cam_of[i]
// (clamped into the table) of cams (ncam,19) = K, K^-1, depth_unit -- one row per workgroup, read once in front of pass 2.  The three
// parameters come last and the plain instantiation does not touch them: captra_image_members' instruction stream is what it was.
template <bool CAM>
__global__ __launch_bounds__(IM_T) void image_members_kernel(int h, int w, int cap, int border, int negate_z, int split, int share,
                                                             const int *__restrict__ depth_all, const unsigned char *__restrict__ mask_all,
                                                             const unsigned char *__restrict__ coord_all, const double *__restrict__ kinv,
                                                             float *__restrict__ src_all, float *__restrict__ tgt_all,
                                                             int *__restrict__ labels_all, int *__restrict__ pix_all,
                                                             int *__restrict__ counts, int ncam, const double *__restrict__ cams,
                                                             const int *__restrict__ cam_of) {
    __shared__ int acc[3];
    __shared__ int wave_tot[2][IM_T / 64];
    const int img = blockIdx.x / split, g = blockIdx.x - img * split;
    const int hw = h * w;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned char *__restrict__ mask = mask_all + (size_t)img * hw;
    const ImImage im = {depth_all + (size_t)img * hw, mask, h, w, border};
    const long long lo = (long long)g * share, hi = lo + share;
    const int t_lo = lo < hw ? (int)lo : hw, t_hi = hi < hw ? (int)hi : hw;    // this workgroup's share of the flat pixel range

    // ---- pass 1: the whole image's counts
    if (tid < 3) acc[tid] = 0;
    __syncthreads();
    int n_before = 0, n_members = 0, n_holes = 0;
    auto count = [&](int t, int r, int c, bool set) {
        int d;
        const int kind = im_classify(im, t, r, c, set, d);
        n_members += kind == 1;
        n_before += kind == 1 && t < t_lo;
        n_holes += kind == 2;
    };
    const int head_full = (int)((16 - ((uintptr_t)mask & 15)) & 15);
    const int head = head_full < hw ? head_full : hw;                // bytes in front of the first 16-byte boundary
    const int nvec = (hw - head) / 16;
    const uint4 *__restrict__ vec = reinterpret_cast<const uint4 *>(mask + head);
    constexpr int IM_V = 4;                                          // vectors in flight per lane: their loads are issued together
    for (int v0 = tid; v0 < nvec; v0 += IM_V * IM_T) {
        uint4 q[IM_V];
#pragma unroll
        for (int i = 0; i < IM_V; ++i) {
            const int v = v0 + i * IM_T;
            q[i] = vec[v < nvec ? v : v0];
            if (v >= nvec) q[i] = make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int i = 0; i < IM_V; ++i) {
            if ((q[i].x | q[i].y | q[i].z | q[i].w) == 0u) continue;
            const unsigned words[4] = {q[i].x, q[i].y, q[i].z, q[i].w};
            const int t = head + 16 * (v0 + i * IM_T);
            int r = t / w, c = t - r * w;
#pragma unroll
            for (int k = 0; k < 16; ++k) {                           // (no branch per byte: the sixteen pixels' loads go out together)
                count(t + k, r, c, ((words[k >> 2] >> (8 * (k & 3))) & 0xFFu) != 0u);
                if (++c == w) { c = 0; ++r; }
            }
        }
    }
    if (tid < head && mask[tid] != 0) count(tid, tid / w, tid % w, true);
    const int tail = head + 16 * nvec + tid;                         // (at most 15 bytes behind the last vector)
    if (tid < hw - (head + 16 * nvec) && mask[tail] != 0) count(tail, tail / w, tail % w, true);
    if (n_before != 0) atomicAdd(&acc[0], n_before);
    if (n_members != 0) atomicAdd(&acc[1], n_members);
    if (n_holes != 0) atomicAdd(&acc[2], n_holes);
    __syncthreads();
    const int before = acc[0], total = acc[1], holes = acc[2];
    const int step = total <= cap ? 1 : (int)(((long long)total + cap - 1) / cap);
    const int used = (int)(((long long)total + step - 1) / step);
    if (g == 0 && tid == 0) {
        counts[img * 3 + 0] = total;
        counts[img * 3 + 1] = used;
        counts[img * 3 + 2] = holes;
    }

    float *__restrict__ src = src_all + (size_t)img * 3 * cap;
    float *__restrict__ tgt = tgt_all + (size_t)img * 3 * cap;
    int *__restrict__ labels = labels_all + (size_t)img * cap;
    int *__restrict__ pix = pix_all + (size_t)img * cap;

    // ---- the slots no member takes, shared among the image's workgroups
    for (long long s = (long long)used + (long long)g * IM_T + tid; s < cap; s += (long long)split * IM_T) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { src[(size_t)k * cap + s] = 0.f; tgt[(size_t)k * cap + s] = 0.f; }
        labels[s] = -1;
        pix[s] = -1;
    }
    if (total == 0) return;

    // ---- pass 2: this workgroup's share, in order
    double k9[9];
    double unit = 0.001;
    if constexpr (CAM) {
        int ci = cam_of[img];
        ci = ci < 0 ? 0 : (ci < ncam ? ci : ncam - 1);
        const double *__restrict__ cam = cams + (size_t)ci * 19;
#pragma unroll
        for (int i = 0; i < 9; ++i) k9[i] = cam[9 + i];
        unit = cam[18];
    } else {
#pragma unroll
        for (int i = 0; i < 9; ++i) k9[i] = kinv[i];
    }
    const unsigned char *__restrict__ coord = coord_all + (size_t)img * hw * 3;
    int base = before, it = 0;
    for (long long t0 = t_lo; t0 < t_hi; t0 += IM_T, ++it) {        // (64-bit: hw may be INT_MAX)
        const bool mine = t0 + tid < t_hi;
        const int t = mine ? (int)(t0 + tid) : 0;
        bool member = false;
        int r = 0, c = 0, d = 0;
        if (mine && mask[t] != 0) {
            r = t / w;
            c = t - r * w;
            member = im_classify(im, t, r, c, true, d) == 1;
        }
        const unsigned long long m = __ballot(member);
        if (lane == 0) wave_tot[it & 1][wave] = __popcll(m);
        __syncthreads();
        int in_front = 0, all = 0;
#pragma unroll
        for (int i = 0; i < IM_T / 64; ++i) {
            const int e = wave_tot[it & 1][i];
            in_front += i < wave ? e : 0;
            all += e;
        }
        if (member) {
            const int j = base + in_front + __popcll(m & ((1ull << lane) - 1ull));
            const int s = j / step;
            if (j - s * step == 0) {
                const double u = (double)c, v = (double)(h - r);
                const double rx = (k9[0] * u + k9[1] * v) + k9[2];
                const double ry = (k9[3] * u + k9[4] * v) + k9[5];
                const double rz = (k9[6] * u + k9[7] * v) + k9[8];
                const double z = (double)(float)d;                   // captra_crop_ball's: depth[idxs].astype(np.float32)
                tgt[s] = (float)((rx * z / rz) * unit);
                tgt[(size_t)cap + s] = (float)((ry * z / rz) * unit);
                tgt[(size_t)2 * cap + s] = (float)(-(rz * z / rz) * unit);
                const unsigned char *__restrict__ q = coord + (size_t)t * 3;
                const double n0 = (double)q[0] / 255.0 - 0.5, n1 = (double)q[1] / 255.0 - 0.5, n2 = (double)q[2] / 255.0 - 0.5;
                src[s] = (float)n0;
                src[(size_t)cap + s] = (float)n1;
                src[(size_t)2 * cap + s] = (float)(negate_z != 0 ? -n2 : n2);
                labels[s] = 0;
                pix[s] = t;
            }
        }
        base += all;
    }
}

CAPTRA_KNOB int g_im_split = 0;          // measurement knob: workgroups per image (0 = as many as fill the device twice)

}  // namespace

extern "C" void captra_image_members_set_split(int n) { g_im_split = n; }

// The launch of both entry points: kinv (CAM = false) or the camera table (CAM = true).
template <bool CAM>
static int image_members_launch(int b, int h, int w, int cap, int border, int negate_z, const int *depth, const unsigned char *mask,
                                const unsigned char *coord, const double *kinv, int ncam, const double *cams, const int *cam_of, float *src,
                                float *tgt, int *labels, int *pix, int *counts, captra_stream_t stream) {
    if (b < 0 || h < 0 || w < 0 || cap < 1 || border < 0 || border > 3) return -1;
    if ((long long)h * (long long)w > (long long)INT_MAX) return -1;
    if (CAM && ncam < 1) return -1;
    if (b == 0 || h == 0 || w == 0) return 0;
    if (depth == nullptr || mask == nullptr || coord == nullptr || src == nullptr || tgt == nullptr || labels == nullptr || pix == nullptr ||
        counts == nullptr)
        return -1;
    if (CAM ? (cams == nullptr || cam_of == nullptr) : kinv == nullptr) return -1;
    const int hw = h * w;
    // workgroups per image: the device filled twice, a share of at least 4096 pixels (the knob: any number up to a pixel per workgroup)
    long long split = g_im_split > 0 ? g_im_split : (2LL * captra_device_cus() + b - 1) / b;
    const long long most = g_im_split > 0 ? hw : (hw + 4095) / 4096;
    split = split < most ? split : most;
    split = split < INT_MAX / b ? split : INT_MAX / b;               // (the grid is one-dimensional: images x split)
    split = split > 1 ? split : 1;
    const int share = (int)((hw + split - 1) / split);
    CAPTRA_LAUNCH("image_members", image_members_kernel<CAM>, dim3((unsigned)(b * split)), dim3(IM_T), 0, (hipStream_t)stream, h, w, cap, border,
                  negate_z, (int)split, share, depth, mask, coord, kinv, src, tgt, labels, pix, counts, ncam, cams, cam_of);
    return captra_last_error();
}

extern "C" int captra_image_members(int b, int h, int w, int cap, int border, int negate_z, const int *depth, const unsigned char *mask,
                                    const unsigned char *coord, const double *kinv, float *src, float *tgt, int *labels, int *pix,
                                    int *counts, captra_stream_t stream) {
    return image_members_launch<false>(b, h, w, cap, border, negate_z, depth, mask, coord, kinv, 0, nullptr, nullptr, src, tgt, labels, pix,
                                       counts, stream);
}

extern "C" int captra_image_members_cam(int b, int h, int w, int cap, int border, int negate_z, const int *depth, const unsigned char *mask,
                                        const unsigned char *coord, int ncam, const double *cams, const int *cam_of, float *src, float *tgt,
                                        int *labels, int *pix, int *counts, captra_stream_t stream) {
    return image_members_launch<true>(b, h, w, cap, border, negate_z, depth, mask, coord, nullptr, ncam, cams, cam_of, src, tgt, labels,
                                      pix, counts, stream);
}
