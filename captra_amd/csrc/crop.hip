// Ball crop of a depth frame around a predicted centre, for gfx950 — the candidate extraction of the on-the-fly re-crop
// of NOCS tracking (reference datasets/nocs_data/nocs_data_process.py:92-109, 151-163 `crop_ball_from_depth_image` /
// `crop_ball_from_pts`; nocs_utils.py:5-33 `backproject`): inside the image-space box of the ball, back-project every
// pixel with a valid depth, keep those within `radius` of the centre, IN ROW-MAJOR PIXEL ORDER (the order decides which
// point furthest-point sampling starts from).  The reference does this in numpy on the host per tracked instance; the
// torch restatement in captra_amd/nocs_otf.py costs ~0.35 ms and two host syncs per instance.  Here one workgroup per
// instance walks its box 1024 pixels at a time and compacts the members in order (wave ballot + LDS wave offsets).
//
// Arithmetic is float64 like numpy's, written out operation by operation (no FMA contraction: the build runs with
// -ffp-contract=off):  ray = Kinv (col, H - row, 1);  p = ray * z / ray_z;  p = (p_x, p_y, -p_z) * 0.001;
// member  <=>  sqrt(((p - c)_x^2 + (p - c)_y^2) + (p - c)_z^2) <= radius.
//
// The camera model (include/captra_hip.h: captra_crop_ball_cam and its kin): the *_cam entry points take a table of cameras, (ncam,19)
// doubles = K, K^-1, depth_unit per row, and one row index per trajectory; Kinv and 0.001 above become that row's Kinv and unit, the box
// projection takes that row's K (its 1000.0 stays a constant: the projection is scale-free).  The kernels are templated on CAM; the
// plain instantiations read `kinv` / `kmat` and the literal 0.001 as before.
#include "common.h"

#include <math.h>

namespace {

constexpr int CB_T = 1024;
constexpr int CAM_ROW = 19;              // doubles per camera: K (9), K^-1 (9), depth_unit (1)

// The camera row of trajectory i: cam_of[i] clamped into the table (memory safety only: the host wrapper builds cam_of).
__device__ __forceinline__ const double *cam_row(const double *__restrict__ cams, const int *__restrict__ cam_of, int ncam, int i) {
    int c = cam_of[i];
    c = c < 0 ? 0 : (c < ncam ? c : ncam - 1);
    return cams + (size_t)c * CAM_ROW;
}

// DET (captra_crop_ball_det): the instance mask of trajectory b is detection sel[b] of det_masks (B,ndet,h,w) -- the mask the detector
// route selected (crop_box_det_kernel below) -- and mask_all's when sel[b] < 0 (no detection of the category: the reference keeps the
// pre-fetched mask, nocs_data_process.py:217-218).  The three extra parameters come LAST and the plain instantiation does not touch
// them: captra_crop_ball's instruction stream is what it was.
// CAM (captra_crop_ball_cam, captra_crop_ball_det_cam): Kinv and the depth unit of trajectory b are those of row cam_of[b] of cams -- one
// row per workgroup, at a workgroup-uniform address: ten scalar loads in front of the pixel loop, nothing per pixel.  Again the three
// parameters come last and the plain instantiations do not touch them (their unit is the literal 0.001).
template <bool DET, bool CAM>
__global__ __launch_bounds__(CB_T) void crop_ball_kernel(int h, int w, int cap, const int *__restrict__ depth_all,
                                                         const unsigned char *__restrict__ mask_all,
                                                         const int *__restrict__ box_all, const double *__restrict__ center_all,
                                                         const double *__restrict__ radius_all, const double *__restrict__ kinv,
                                                         double *__restrict__ pts_all, unsigned char *__restrict__ obj_all,
                                                         int *__restrict__ pix_all, int *__restrict__ counts,
                                                         const unsigned char *__restrict__ det_masks, const int *__restrict__ sel_all,
                                                         int ndet, int ncam, const double *__restrict__ cams,
                                                         const int *__restrict__ cam_of) {
    __shared__ int wave_tot[2][16];
    const int b = blockIdx.x;
    const int *depth = depth_all + (size_t)b * h * w;
    const unsigned char *mask = mask_all + (size_t)b * h * w;
    if constexpr (DET) {
        const int s = sel_all[b];
        if (s >= 0 && s < ndet) mask = det_masks + ((size_t)b * ndet + s) * h * w;      // (an index outside the stack: the pre-fetched mask)
    }
    const int r0 = box_all[b * 4 + 0], c0 = box_all[b * 4 + 1], r1 = box_all[b * 4 + 2], c1 = box_all[b * 4 + 3];
    const double cx = center_all[b * 3 + 0], cy = center_all[b * 3 + 1], cz = center_all[b * 3 + 2];
    const double rad = radius_all[b];
    double k[9];
    double unit = 0.001;
    if constexpr (CAM) {
        const double *__restrict__ cam = cam_row(cams, cam_of, ncam, b);
#pragma unroll
        for (int i = 0; i < 9; ++i) k[i] = cam[9 + i];
        unit = cam[18];
    } else {
#pragma unroll
        for (int i = 0; i < 9; ++i) k[i] = kinv[i];
    }
    double *pts = pts_all + (size_t)b * cap * 3;
    unsigned char *obj = obj_all + (size_t)b * cap;
    int *pix = pix_all + (size_t)b * cap;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bw = c1 - c0 + 1, bh = r1 - r0 + 1;
    const long long total = (bw > 0 && bh > 0) ? (long long)bw * bh : 0;
    int base = 0, valid = 0, it = 0;
    for (long long t0 = 0; t0 < total; t0 += CB_T, ++it) {
        const long long t = t0 + tid;
        bool member = false, has_depth = false;
        double px = 0., py = 0., pz = 0.;
        int row = 0, col = 0;
        if (t < total) {
            row = r0 + (int)(t / bw);
            col = c0 + (int)(t % bw);
            const int d = depth[(size_t)row * w + col];
            if (d > 0) {
                has_depth = true;
                const double u = (double)col, v = (double)(h - row);
                const double rx = (k[0] * u + k[1] * v) + k[2];
                const double ry = (k[3] * u + k[4] * v) + k[5];
                const double rz = (k[6] * u + k[7] * v) + k[8];
                const double z = (double)(float)d;                 // depth[idxs].astype(np.float32)
                px = (rx * z / rz) * unit;
                py = (ry * z / rz) * unit;
                pz = -(rz * z / rz) * unit;
                const double dx = px - cx, dy = py - cy, dz = pz - cz;
                member = sqrt((dx * dx + dy * dy) + dz * dz) <= rad;
            }
        }
        const unsigned long long m = __ballot(member), v = __ballot(has_depth);
        if (lane == 0) wave_tot[it & 1][wave] = __popcll(m) | (__popcll(v) << 8);
        __syncthreads();
        int before = 0, all = 0, allv = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int e = wave_tot[it & 1][i];
            before += i < wave ? (e & 0xFF) : 0;
            all += e & 0xFF;
            allv += e >> 8;
        }
        if (member) {
            const int pos = base + before + __popcll(m & ((1ull << lane) - 1ull));
            if (pos < cap) {
                pts[(size_t)pos * 3 + 0] = px; pts[(size_t)pos * 3 + 1] = py; pts[(size_t)pos * 3 + 2] = pz;
                obj[pos] = mask[(size_t)row * w + col];
                pix[pos] = row * w + col;
            }
        }
        base += all;
        valid += allv;
    }
    if (tid == 0) { counts[b * 2 + 0] = base; counts[b * 2 + 1] = valid; }
}

// The crop's image-space box from the device-resident pose (reference nocs_data_process.py:136-148 `proj_corners`; model.py:425-452:
// the ball is centred on the pose predicted for the previous frame, radius = radius_factor x its scale): float64, operation by
// operation as numpy evaluates captra_amd/nocs_otf.py::proj_corners_batch -- r = max(radius_factor * scale, 0.05); the 8 corners of
// c +- r times 1000; (-x / z, -y / z, 1); u = (K00 x + K01 y) + K02, v = (K10 x + K11 y) + K12 truncated to int32; rows = h - v, cols = u;
// min / max over the corners, clamped to the image.  One thread per instance: the box, centre and radius crop_ball_kernel reads.
__device__ __forceinline__ long long ll_max(long long a, long long b) { return a > b ? a : b; }
__device__ __forceinline__ long long ll_min(long long a, long long b) { return a < b ? a : b; }

// The projection itself, for the raw radius r_in: -> box[4] = {row_min, col_min, row_max, col_max}; returns the clamped radius.
__device__ __forceinline__ double crop_box_project(int h, int w, const double c[3], double r_in, const double *__restrict__ kmat, int box[4]) {
    const double r = r_in > 0.05 ? r_in : 0.05;  // numpy.maximum(r, 0.05) (NaN propagates there; a NaN pose has no crop either way)
    int rmin = 0x7fffffff, rmax = -0x7fffffff - 1, cmin = 0x7fffffff, cmax = -0x7fffffff - 1;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const double bx = ((e & 1) ? c[0] + r : c[0] - r) * 1000.0;
        const double by = ((e & 2) ? c[1] + r : c[1] - r) * 1000.0;
        const double bz = ((e & 4) ? c[2] + r : c[2] - r) * 1000.0;
        const double hx = (-bx) / bz, hy = (-by) / bz, hz = -((-bz) / bz);
        const double u = (kmat[0] * hx + kmat[1] * hy) + kmat[2] * hz;
        const double v = (kmat[3] * hx + kmat[4] * hy) + kmat[5] * hz;
        const int row = h - (int)v, col = (int)u;
        rmin = row < rmin ? row : rmin; rmax = row > rmax ? row : rmax;
        cmin = col < cmin ? col : cmin; cmax = col > cmax ? col : cmax;
    }
    box[0] = rmin > 0 ? rmin : 0;
    box[1] = cmin > 0 ? cmin : 0;
    box[2] = rmax < h - 1 ? rmax : h - 1;
    box[3] = cmax < w - 1 ? cmax : w - 1;
    return r;
}

// CAM (captra_crop_box_cam): the projection of instance i with the K of row cam_of[i] of cams (the first 9 doubles of the row).
template <bool CAM>
__global__ void crop_box_kernel(int b, int h, int w, double radius_factor, const float *__restrict__ trans, const float *__restrict__ scale,
                                const double *__restrict__ kmat, int *__restrict__ box, double *__restrict__ center,
                                double *__restrict__ radius, int ncam, const double *__restrict__ cams, const int *__restrict__ cam_of) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b) return;
    if constexpr (CAM) kmat = cam_row(cams, cam_of, ncam, i);
    const double c[3] = {(double)trans[i * 3 + 0], (double)trans[i * 3 + 1], (double)trans[i * 3 + 2]};
    int bx[4];
    const double r = crop_box_project(h, w, c, radius_factor * (double)scale[i], kmat, bx);
    box[i * 4 + 0] = bx[0]; box[i * 4 + 1] = bx[1]; box[i * 4 + 2] = bx[2]; box[i * 4 + 3] = bx[3];
    center[i * 3 + 0] = c[0]; center[i * 3 + 1] = c[1]; center[i * 3 + 2] = c[2];
    radius[i] = r;
}

// The detector route of the re-crop (reference nocs_data_process.py:166-179, 206-229: `--track_cfg/nocs2d_label True`): the instance mask
// of a frame is the 2D detection of the tracked category whose box overlaps the crop's box best, and the crop's radius grows by 1.2
// per round while no detection of the category overlaps it by more than 0.05 (until the radius passes 0.5).  Operation by operation as
// numpy evaluates it: the box of (centre, raw radius) by crop_box_project (the 0.05 clamp inside the projection only); intersection
// and the three areas as 64-bit integers max(x2 - x1, 0) * max(y2 - y1, 0) (exclusive extents, as the reference has them); the IoU
// ONE float64 division, times `same`; the selection the FIRST arg max of the last round -- after a give-up with every IoU zero that is
// detection 0 whatever its class, as in the reference.
// ONE WAVE per trajectory: lane l takes detections l, l + 64, ... of the det_count[b] real ones (any K: nothing is staged, no cap) and
// keeps its best (IoU, index) -- `>` keeps the first, its indices ascend --, then six xor-shuffle steps reduce (larger IoU, on a tie
// the smaller index) so that every lane holds the wave's verdict and the loop's exit test is wave-uniform without LDS or a barrier.
// The projection is recomputed by every lane (8 corners, ~100 float64 operations per round; the rounds are sequential anyway).
// Outside the reference's contract: a detection whose union with the box is 0 counts as IoU 0 (numpy: 0/0 = NaN); a growth step that
// does not enlarge the radius -- NaN, inf, <= 0, or a subnormal that 1.2 x rounds back to itself -- ends the loop at once (the
// reference would not terminate there).
// CAM (captra_crop_box_det_cam): as crop_box_kernel<true>; the row is the wave's.
template <bool CAM>
__global__ __launch_bounds__(64) void crop_box_det_kernel(int h, int w, int ndet, int category, double radius_factor,
                                                          const float *__restrict__ trans, const float *__restrict__ scale,
                                                          const double *__restrict__ kmat, const int *__restrict__ det_boxes,
                                                          const int *__restrict__ det_class, const int *__restrict__ det_count,
                                                          int *__restrict__ box, double *__restrict__ center, double *__restrict__ radius,
                                                          double *__restrict__ radius_raw, int *__restrict__ sel, int ncam,
                                                          const double *__restrict__ cams, const int *__restrict__ cam_of) {
    const int i = blockIdx.x, lane = threadIdx.x;
    if constexpr (CAM) kmat = cam_row(cams, cam_of, ncam, i);
    const double c[3] = {(double)trans[i * 3 + 0], (double)trans[i * 3 + 1], (double)trans[i * 3 + 2]};
    double r = radius_factor * (double)scale[i];
    int cnt = det_count[i];
    cnt = cnt < 0 ? 0 : (cnt > ndet ? ndet : cnt);
    const int *db = det_boxes + (size_t)i * ndet * 4;
    const int *dc = det_class + (size_t)i * ndet;
    bool any_same = false;
    for (int k = lane; k < cnt; k += 64) any_same |= dc[k] == category;
    int bx[4], best_k = -1;
    double rc;
    if (__ballot(any_same) == 0ull) {
        rc = crop_box_project(h, w, c, r, kmat, bx);          // `no same class pred!`: captra_crop_box's outputs, sel = -1
    } else {
        for (;;) {
            rc = crop_box_project(h, w, c, r, kmat, bx);
            const long long barea = ll_max((long long)bx[3] - bx[1], 0) * ll_max((long long)bx[2] - bx[0], 0);
            double best = -1.0;
            best_k = 0x7fffffff;
            for (int k = lane; k < cnt; k += 64) {
                const long long y1 = db[k * 4 + 0], x1 = db[k * 4 + 1], y2 = db[k * 4 + 2], x2 = db[k * 4 + 3];
                const long long iy1 = ll_max(bx[0], y1), iy2 = ll_min(bx[2], y2);
                const long long ix1 = ll_max(bx[1], x1), ix2 = ll_min(bx[3], x2);
                const long long inter = ll_max(ix2 - ix1, 0) * ll_max(iy2 - iy1, 0);
                const long long uni = (barea + ll_max(x2 - x1, 0) * ll_max(y2 - y1, 0)) - inter;
                const double iou = (dc[k] == category && uni != 0) ? (double)inter / (double)uni : 0.0;
                if (iou > best) { best = iou; best_k = k; }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const double ob = __shfl_xor(best, off, 64);
                const int ok = __shfl_xor(best_k, off, 64);
                if (ob > best || (ob == best && ok < best_k)) { best = ob; best_k = ok; }
            }
            if (best > 0.05 || r > 0.5) break;
            const double grown = r * 1.2;
            if (!(grown > r)) break;
            r = grown;
        }
    }
    if (lane == 0) {
        box[i * 4 + 0] = bx[0]; box[i * 4 + 1] = bx[1]; box[i * 4 + 2] = bx[2]; box[i * 4 + 3] = bx[3];
        center[i * 3 + 0] = c[0]; center[i * 3 + 1] = c[1]; center[i * 3 + 2] = c[2];
        radius[i] = rc;
        radius_raw[i] = r;
        sel[i] = best_k;
    }
}

// ---- the re-crop's candidate lists and its read-out without the host --------------------------------------
// What the host did between the crop and the sampler, from the member counts it fetched (captra_amd/nocs_otf.py, reference
// data_utils.py:138-162 farthest_point_sample's caller / nocs_data_process.py:92-109): the candidate list of an instance is its
// member table repeated until it holds at least num_points entries (list doubling: candidate j = member j mod count, length =
// count * 2^k), thinned by a random permutation when longer than 5 num_points (the host's generator: a RARE path here).
// otf_candidates_kernel builds the lists (fp32 coordinates, the sampler's input) and their lengths on the device and raises the
// rare-path word; otf_finish_kernel turns the sampler's picks into the frame's tensors (reference nocs_data_process.py:43-50,
// 227-236: points, labels 0 = object / 1 = background, ground-truth NOCS of the object's points) in the layouts the networks read.
__device__ __forceinline__ int otf_list_length(int c, int num_points) {
    int len = c;
    while (len < num_points) len *= 2;
    return len;
}

// THIN (captra_otf_candidates_thin / captra_otf_finish_thin): a row whose thinned[b] is set takes its list from table (B, 5 num_points),
// the ascending member numbers captra_otf_thin (csrc/otf_thin.hip) selected -- candidate j = member table[b][j], length 5 num_points,
// rare only when that outgrows the stride (the list is then the table's first `stride` entries), info[2] counts such rows.  As with
// crop_ball_kernel<DET>, the two extra parameters come LAST and the plain instantiation does not touch them.
template <bool THIN>
__global__ __launch_bounds__(256) void otf_candidates_kernel(int cap, int stride, int num_points, const double *__restrict__ pts,
                                                             const int *__restrict__ counts, float *__restrict__ cand,
                                                             int *__restrict__ lens, int *__restrict__ info,
                                                             const int *__restrict__ table, const int *__restrict__ thinned) {
    const int b = blockIdx.y;
    const int c = counts[b * 2];
    const int lim = cap < stride ? cap : stride;                    // members a list may name: what the table holds, at most a stride
    const int cc = c < 1 ? 1 : (c > lim ? lim : c);                 // rare rows clamped: every access stays inside its instance's table
    if constexpr (THIN) {
        if (thinned[b] != 0) {
            const double *pb = pts + (size_t)b * cap * 3;
            float *cb = cand + (size_t)b * stride * 3;
            const int t_keep = 5 * num_points;
            const int keep = t_keep < stride ? t_keep : stride;
            if (blockIdx.x == 0 && threadIdx.x == 0) {
                lens[b] = keep;
                if (t_keep > stride) atomicOr(info, 1);
                atomicMax(info + 1, t_keep);
                atomicAdd(info + 2, 1);
            }
            const int *tb = table + (size_t)b * t_keep;
            for (int j = blockIdx.x * 256 + threadIdx.x; j < stride; j += gridDim.x * 256) {
                float x = 0.f, y = 0.f, z = 0.f;
                if (j < keep) {
                    const double *q = pb + (size_t)tb[j] * 3;
                    x = (float)q[0]; y = (float)q[1]; z = (float)q[2];
                }
                cb[(size_t)j * 3 + 0] = x; cb[(size_t)j * 3 + 1] = y; cb[(size_t)j * 3 + 2] = z;
            }
            return;
        }
    }
    const int len = otf_list_length(cc, num_points);
    const int keep = len < stride ? len : stride;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        lens[b] = keep;
        if (c < 10 || c > lim || len > stride) atomicOr(info, 1);
        atomicMax(info + 1, c > cap ? cap : otf_list_length(c < 1 ? 1 : c, num_points));
    }
    const double *pb = pts + (size_t)b * cap * 3;
    float *cb = cand + (size_t)b * stride * 3;
    for (int j = blockIdx.x * 256 + threadIdx.x; j < stride; j += gridDim.x * 256) {
        float x = 0.f, y = 0.f, z = 0.f;
        if (j < keep) {
            const double *q = pb + (size_t)(j % cc) * 3;
            x = (float)q[0]; y = (float)q[1]; z = (float)q[2];
        }
        cb[(size_t)j * 3 + 0] = x; cb[(size_t)j * 3 + 1] = y; cb[(size_t)j * 3 + 2] = z;
    }
}

template <bool THIN>
__global__ __launch_bounds__(256) void otf_finish_kernel(int cap, int stride, int n, const double *__restrict__ pts,
                                                         const unsigned char *__restrict__ obj, const int *__restrict__ counts,
                                                         const int *__restrict__ picks, const float *__restrict__ mean,
                                                         const double *__restrict__ rot, const double *__restrict__ trans,
                                                         const double *__restrict__ scale, float *__restrict__ points_cn,
                                                         long long *__restrict__ labels, float *__restrict__ nocs_cn,
                                                         const int *__restrict__ table, const int *__restrict__ thinned) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = counts[b * 2];
    const int lim = cap < stride ? cap : stride;
    const int cc = c < 1 ? 1 : (c > lim ? lim : c);                   // otf_candidates_kernel's clamp
    int m = picks[(size_t)b * n + i] % cc;                            // candidate -> member
    if constexpr (THIN) {
        if (thinned[b] != 0) {                                        // a thinned row: through its table of 5 n members (a pick stays inside it)
            const int p = picks[(size_t)b * n + i];
            m = table[(size_t)b * 5 * n + (p < 0 ? 0 : (p < 5 * n ? p : 5 * n - 1))];
        }
    }
    const double *q = pts + ((size_t)b * cap + m) * 3;
    const bool o = obj[(size_t)b * cap + m] != 0;
    const double *R = rot + (size_t)b * 9, *t = trans + (size_t)b * 3;
    const double s = scale[b];
    const double x0 = (q[0] - t[0]) / s, x1 = (q[1] - t[1]) / s, x2 = (q[2] - t[2]) / s;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        // (a NaN leaves with its sign clear, as from captra_canonicalize: include/captra_hip.h, "NaN / Inf contract")
        const float pc = (float)q[a] - mean[b * 3 + a];
        points_cn[((size_t)b * 3 + a) * n + i] = pc != pc ? __int_as_float(__float_as_int(pc) & 0x7FFFFFFF) : pc;
        nocs_cn[((size_t)b * 3 + a) * n + i] = o ? (float)((x0 * R[a] + x1 * R[3 + a]) + x2 * R[6 + a]) : 0.f;
    }
    labels[(size_t)b * n + i] = o ? 0 : 1;
}

}  // namespace

extern "C" int captra_crop_box(int b, int h, int w, double radius_factor, const float *trans, const float *scale, const double *kmat,
                               int *box, double *center, double *radius, captra_stream_t stream) {
    if (b < 0 || h < 1 || w < 1) return -1;
    if (b == 0) return 0;
    CAPTRA_LAUNCH("crop_ball", crop_box_kernel<false>, dim3((b + 63) / 64), dim3(64), 0, (hipStream_t)stream, b, h, w, radius_factor, trans,
                  scale, kmat, box, center, radius, 0, (const double *)nullptr, (const int *)nullptr);
    return captra_last_error();
}

extern "C" int captra_crop_ball(int b, int h, int w, int cap, const int *depth, const unsigned char *mask, const int *box,
                                const double *center, const double *radius, const double *kinv, double *pts,
                                unsigned char *obj, int *pix, int *counts, captra_stream_t stream) {
    if (b < 0 || h < 1 || w < 1 || cap < 1) return -1;
    if (b == 0) return 0;
    CAPTRA_LAUNCH("crop_ball", (crop_ball_kernel<false, false>), dim3(b), dim3(CB_T), 0, (hipStream_t)stream, h, w, cap, depth, mask, box,
                  center, radius, kinv, pts, obj, pix, counts, (const unsigned char *)nullptr, (const int *)nullptr, 0, 0,
                  (const double *)nullptr, (const int *)nullptr);
    return captra_last_error();
}

// The detector route (see crop_box_det_kernel): captra_crop_box's outputs after the reference's radius growth, the radius as the
// reference hands it on (radius_raw: unclamped) and the selected detection per trajectory (sel, -1 = none of the category).
extern "C" int captra_crop_box_det(int b, int h, int w, int ndet, int category, double radius_factor, const float *trans, const float *scale,
                                   const double *kmat, const int *det_boxes, const int *det_class, const int *det_count, int *box,
                                   double *center, double *radius, double *radius_raw, int *sel, captra_stream_t stream) {
    if (b < 0 || h < 1 || w < 1 || ndet < 0) return -1;
    if (b == 0) return 0;
    CAPTRA_LAUNCH("crop_ball", crop_box_det_kernel<false>, dim3(b), dim3(64), 0, (hipStream_t)stream, h, w, ndet, category, radius_factor, trans,
                  scale, kmat, det_boxes, det_class, det_count, box, center, radius, radius_raw, sel, 0, (const double *)nullptr,
                  (const int *)nullptr);
    return captra_last_error();
}

// captra_crop_ball with the instance mask of trajectory i taken from det_masks (B,ndet,h,w) at detection sel[i], and from mask where sel[i] < 0.
extern "C" int captra_crop_ball_det(int b, int h, int w, int cap, int ndet, const int *depth, const unsigned char *mask,
                                    const unsigned char *det_masks, const int *sel, const int *box, const double *center,
                                    const double *radius, const double *kinv, double *pts, unsigned char *obj, int *pix, int *counts,
                                    captra_stream_t stream) {
    if (b < 0 || h < 1 || w < 1 || cap < 1 || ndet < 0) return -1;
    if (b == 0) return 0;
    CAPTRA_LAUNCH("crop_ball", (crop_ball_kernel<true, false>), dim3(b), dim3(CB_T), 0, (hipStream_t)stream, h, w, cap, depth, mask, box,
                  center, radius, kinv, pts, obj, pix, counts, det_masks, sel, ndet, 0, (const double *)nullptr, (const int *)nullptr);
    return captra_last_error();
}

// ---- the camera model: the four calls above with a camera per trajectory (include/captra_hip.h, "The CAMERA MODEL") -----------------
extern "C" int captra_crop_box_cam(int b, int h, int w, double radius_factor, const float *trans, const float *scale, int ncam,
                                   const double *cams, const int *cam_of, int *box, double *center, double *radius, captra_stream_t stream) {
    if (b < 0 || h < 1 || w < 1 || ncam < 1) return -1;
    if (b == 0) return 0;
    if (cams == nullptr || cam_of == nullptr) return -1;
    CAPTRA_LAUNCH("crop_ball", crop_box_kernel<true>, dim3((b + 63) / 64), dim3(64), 0, (hipStream_t)stream, b, h, w, radius_factor, trans,
                  scale, (const double *)nullptr, box, center, radius, ncam, cams, cam_of);
    return captra_last_error();
}

extern "C" int captra_crop_box_det_cam(int b, int h, int w, int ndet, int category, double radius_factor, const float *trans,
                                       const float *scale, int ncam, const double *cams, const int *cam_of, const int *det_boxes,
                                       const int *det_class, const int *det_count, int *box, double *center, double *radius,
                                       double *radius_raw, int *sel, captra_stream_t stream) {
    if (b < 0 || h < 1 || w < 1 || ndet < 0 || ncam < 1) return -1;
    if (b == 0) return 0;
    if (cams == nullptr || cam_of == nullptr) return -1;
    CAPTRA_LAUNCH("crop_ball", crop_box_det_kernel<true>, dim3(b), dim3(64), 0, (hipStream_t)stream, h, w, ndet, category, radius_factor,
                  trans, scale, (const double *)nullptr, det_boxes, det_class, det_count, box, center, radius, radius_raw, sel, ncam, cams,
                  cam_of);
    return captra_last_error();
}

extern "C" int captra_crop_ball_cam(int b, int h, int w, int cap, const int *depth, const unsigned char *mask, const int *box,
                                    const double *center, const double *radius, int ncam, const double *cams, const int *cam_of,
                                    double *pts, unsigned char *obj, int *pix, int *counts, captra_stream_t stream) {
    if (b < 0 || h < 1 || w < 1 || cap < 1 || ncam < 1) return -1;
    if (b == 0) return 0;
    if (cams == nullptr || cam_of == nullptr) return -1;
    CAPTRA_LAUNCH("crop_ball", (crop_ball_kernel<false, true>), dim3(b), dim3(CB_T), 0, (hipStream_t)stream, h, w, cap, depth, mask, box,
                  center, radius, (const double *)nullptr, pts, obj, pix, counts, (const unsigned char *)nullptr, (const int *)nullptr, 0,
                  ncam, cams, cam_of);
    return captra_last_error();
}

extern "C" int captra_crop_ball_det_cam(int b, int h, int w, int cap, int ndet, const int *depth, const unsigned char *mask,
                                        const unsigned char *det_masks, const int *sel, const int *box, const double *center,
                                        const double *radius, int ncam, const double *cams, const int *cam_of, double *pts,
                                        unsigned char *obj, int *pix, int *counts, captra_stream_t stream) {
    if (b < 0 || h < 1 || w < 1 || cap < 1 || ndet < 0 || ncam < 1) return -1;
    if (b == 0) return 0;
    if (cams == nullptr || cam_of == nullptr) return -1;
    CAPTRA_LAUNCH("crop_ball", (crop_ball_kernel<true, true>), dim3(b), dim3(CB_T), 0, (hipStream_t)stream, h, w, cap, depth, mask, box,
                  center, radius, (const double *)nullptr, pts, obj, pix, counts, det_masks, sel, ndet, ncam, cams, cam_of);
    return captra_last_error();
}

// The candidate lists of a re-crop and the ragged sampler's per-cloud counts, from the crop's device-resident member counts (see the
// kernels above).  cand (B,stride,3) fp32, lens (B,), info: 4 ints, zeroed here on the stream, [0] = a rare-path instance was met
// (< 10 members, more members than `stride` or than the table's `cap` rows, or a list longer than `stride`), [1] = the longest list.
// num_points <= stride; cap may be smaller than stride (a list then repeats the first cap members: it never leaves its table).
extern "C" int captra_otf_candidates(int b, int cap, int stride, int num_points, const double *pts, const int *counts, float *cand,
                                     int *lens, int *info, captra_stream_t stream) {
    if (b < 0 || cap < 1 || stride < 1 || num_points < 1 || num_points > stride) return -1;
    if (b == 0) return 0;
    if (captra_zero_async(info, 16, (hipStream_t)stream) != 0) return -1;
    CAPTRA_LAUNCH("crop_ball", otf_candidates_kernel<false>, dim3((unsigned)((stride + 1023) / 1024), b), dim3(256), 0, (hipStream_t)stream, cap, stride,
                  num_points, pts, counts, cand, lens, info, (const int *)nullptr, (const int *)nullptr);
    return captra_last_error();
}

// captra_otf_candidates with the rows flagged in thinned (B,) taking their lists from table (B, 5 num_points) (captra_otf_thin's outputs);
// info[2] = the number of such rows.  With thinned all zero: captra_otf_candidates' outputs.
extern "C" int captra_otf_candidates_thin(int b, int cap, int stride, int num_points, const double *pts, const int *counts, float *cand,
                                          int *lens, int *info, const int *table, const int *thinned, captra_stream_t stream) {
    if (b < 0 || cap < 1 || stride < 1 || num_points < 1 || num_points > stride || num_points > 0x7fffffff / 5) return -1;
    if (b == 0) return 0;
    if (captra_zero_async(info, 16, (hipStream_t)stream) != 0) return -1;
    CAPTRA_LAUNCH("crop_ball", otf_candidates_kernel<true>, dim3((unsigned)((stride + 1023) / 1024), b), dim3(256), 0, (hipStream_t)stream, cap, stride,
                  num_points, pts, counts, cand, lens, info, table, thinned);
    return captra_last_error();
}

// picks (B,n) = the sampler's indices into the candidate lists -> points_cn (B,3,n) fp32 = member coordinates - mean (B,3),
// labels (B,n) int64 (0 object / 1 background), nocs_cn (B,3,n) fp32 = ((p - trans) / scale) R of the object's points in float64, 0 elsewhere.
extern "C" int captra_otf_finish(int b, int cap, int stride, int n, const double *pts, const unsigned char *obj, const int *counts,
                                 const int *picks, const float *mean, const double *rot, const double *trans, const double *scale,
                                 float *points_cn, long long *labels, float *nocs_cn, captra_stream_t stream) {
    if (b < 0 || cap < 1 || stride < 1 || n < 1) return -1;
    if (b == 0) return 0;
    CAPTRA_LAUNCH("crop_ball", otf_finish_kernel<false>, dim3((unsigned)((n + 255) / 256), b), dim3(256), 0, (hipStream_t)stream, cap, stride, n, pts, obj,
                  counts, picks, mean, rot, trans, scale, points_cn, labels, nocs_cn, (const int *)nullptr, (const int *)nullptr);
    return captra_last_error();
}

// captra_otf_finish with a pick p of a row flagged in thinned (B,) read as member table[b][p] of table (B, 5 n).
extern "C" int captra_otf_finish_thin(int b, int cap, int stride, int n, const double *pts, const unsigned char *obj, const int *counts,
                                      const int *picks, const float *mean, const double *rot, const double *trans, const double *scale,
                                      float *points_cn, long long *labels, float *nocs_cn, const int *table, const int *thinned,
                                      captra_stream_t stream) {
    if (b < 0 || cap < 1 || stride < 1 || n < 1 || n > 0x7fffffff / 5) return -1;
    if (b == 0) return 0;
    CAPTRA_LAUNCH("crop_ball", otf_finish_kernel<true>, dim3((unsigned)((n + 255) / 256), b), dim3(256), 0, (hipStream_t)stream, cap, stride, n, pts, obj,
                  counts, picks, mean, rot, trans, scale, points_cn, labels, nocs_cn, table, thinned);
    return captra_last_error();
}
