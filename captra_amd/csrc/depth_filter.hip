// Flying-pixel rejection on an organised depth image, for gfx950 (include/captra_hip.h: captra_depth_support_filter, where the rule
// is stated in full).  A structured-light or time-of-flight sensor reports, along a silhouette, depths that lie between the object and
// what is behind it; such a pixel has few image neighbours at its own depth.  A pixel with d > 0 is kept when at least min_support
// of the other in-image pixels of the (2 window + 1)^2 square around it carry a depth d' > 0 with |d' - d| <= abs_mm + floor(d
// rel_permille / 1000); else it becomes 0.  Depth is integer millimetres: pure integer arithmetic, bit for bit a numpy judge's.
//
// One workgroup of 4 waves per tile of 16 rows x 64 columns of one image.  The tile and its halo of `window` pixels are staged once
// into LDS -- (16 + 2 W) x (64 + 2 W) ints, at most 22 x 70 -- a wave per row, with 0 ("no depth") in every cell outside the image,
// so the compare loop has no bounds test and never looks into the next row's wrap-around or the next image of the batch.  A wave then
// owns 4 rows of the tile and a thread a strip of 4 pixels, one below the other: the 4 windows overlap, so the strip reads
// (4 + 2 W) x (2 W + 1) cells (70 for W = 3) where four single pixels read 4 (2 W + 1)^2 (196), each cell compared against the pixels
// whose window holds it.  A wave's lanes read consecutive words of one LDS row: no bank conflict.  The 64-bit rule is folded into two
// 32-bit bounds per pixel, exactly:
//     d' > 0 and |d' - d| <= tol   <=>   lo <= d' <= hi,  lo = max(d - tol, 1), hi = min(d + tol, INT_MAX)   (tol in 64-bit)
//                                  <=>   (unsigned)(d' - lo) <= (unsigned)(hi - lo)                           (1 <= lo <= d <= hi)
// so a halo or hole cell (0) never supports; W is a template parameter, everything is unrolled and the pixel itself is skipped at
// compile time.  (Four-wave workgroups, not one of 16 waves with a pixel per thread: that form spent 85 us on 32 images of 480 x 640
// at W = 1 -- a CU held two workgroups, each waiting at its barrier for its loads, then for its neighbours' -- against 12 us for a copy.)
// The count of removed pixels: a ballot and a population count per strip row (a one-bit flag per lane needs no reduction tree), one
// integer atomicAdd per wave that removed any -- integer, so the count does not depend on the order the waves arrive in.
#include "common.h"

#include <limits.h>

namespace {

constexpr int DF_ROWS = 16, DF_COLS = 64, DF_WAVES = 4, DF_T = DF_WAVES * 64, DF_STRIP = DF_ROWS / DF_WAVES;

template <int W>
__global__ __launch_bounds__(DF_T) void depth_support_filter_kernel(int h, int w, int tiles_x, int tiles_y, int abs_mm, int rel_permille,
                                                                    int min_support, const int *__restrict__ depth_in,
                                                                    int *__restrict__ depth_out, int *__restrict__ removed) {
    constexpr int TH = DF_ROWS + 2 * W, TW = DF_COLS + 2 * W;
    __shared__ int tile[TH * TW];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));             // (uniform: row addresses are scalar work)
    int t = blockIdx.x;                                          // tile number: ((image, tile row), tile column)
    const int tx = t % tiles_x;
    t /= tiles_x;
    const int ty = t % tiles_y, img = t / tiles_y;
    const int r0 = ty * DF_ROWS, c0 = tx * DF_COLS;
    const size_t image = (size_t)img * h * w;
    const int *__restrict__ in = depth_in + image;

    // ---- stage: tile row ry = image row r0 - W + ry, tile column k = image column c0 - W + k.  Wave `wave` takes the rows wave + 4 j:
    // their first 64 columns a row per load, their last 2 W columns -- NR rows x 2 W cells, at most 36 -- in one load of the wave.
    // Every load is UNCONDITIONAL, from the nearest pixel inside the image (h, w >= 1), and the value is replaced by 0 afterwards: a
    // load under a branch is waited for before the next one is issued, and the workgroup then pays the memory latency NR + 1 times.
    constexpr int NR = (TH + DF_WAVES - 1) / DF_WAVES;
    auto pixel = [&](int ry, int k, bool &valid) -> int {
        const int r = r0 - W + ry, c = c0 - W + k;
        valid = ry < TH && r >= 0 && r < h && c >= 0 && c < w;
        const int rc = r < 0 ? 0 : (r < h ? r : h - 1), cc = c < 0 ? 0 : (c < w ? c : w - 1);
        return in[(size_t)rc * w + cc];
    };
    int body[NR];
    bool body_ok[NR], tail_ok;
#pragma unroll
    for (int j = 0; j < NR; ++j) body[j] = pixel(wave + DF_WAVES * j, lane, body_ok[j]);
    const int tj = lane / (2 * W), tk = DF_COLS + lane % (2 * W);                              // the tail cell of this lane
    const int tail = pixel(wave + DF_WAVES * tj, tk, tail_ok);
#pragma unroll
    for (int j = 0; j < NR; ++j)
        if (wave + DF_WAVES * j < TH) tile[(wave + DF_WAVES * j) * TW + lane] = body_ok[j] ? body[j] : 0;
    if (tj < NR && wave + DF_WAVES * tj < TH) tile[(wave + DF_WAVES * tj) * TW + tk] = tail_ok ? tail : 0;
    __syncthreads();

    // ---- the strip: image rows r0 + 4 wave + p, p = 0 .. 3, column c0 + lane = tile rows 4 wave + p + W, tile column lane + W
    const int ls = wave * DF_STRIP;
    const int c = c0 + lane;
    int d[DF_STRIP];
    unsigned lo[DF_STRIP], span[DF_STRIP];
    int support[DF_STRIP];
#pragma unroll
    for (int p = 0; p < DF_STRIP; ++p) {
        d[p] = tile[(ls + p + W) * TW + lane + W];
        const unsigned dd = d[p] > 0 ? (unsigned)d[p] : 1u;      // (d <= 0: bounds of no use, the pixel is copied)
        // floor(d rel / 1000) without a 64-bit division: d = 1000 a + b -> a rel + floor(b rel / 1000), a rel <= 2 147 483 000 and
        // b rel < 10^6, so every term and the sum fit 32 bits unsigned
        const unsigned a = dd / 1000u, b = dd - 1000u * a;
        const unsigned long long tol = (unsigned long long)abs_mm + (a * (unsigned)rel_permille + (b * (unsigned)rel_permille) / 1000u);
        const unsigned l = tol >= dd ? 1u : dd - (unsigned)tol;                                // max(d - tol, 1)
        const unsigned hh = tol > (unsigned)INT_MAX - dd ? (unsigned)INT_MAX : dd + (unsigned)tol;   // min(d + tol, INT_MAX)
        lo[p] = l;
        span[p] = hh - l;
        support[p] = 0;
    }
#pragma unroll
    for (int ry = 0; ry < DF_STRIP + 2 * W; ++ry)
#pragma unroll
        for (int dx = 0; dx <= 2 * W; ++dx) {
            const unsigned o = (unsigned)tile[(ls + ry) * TW + lane + dx];
#pragma unroll
            for (int p = 0; p < DF_STRIP; ++p) {
                const int dy = ry - p;                           // the cell's row in pixel p's window
                if (dy < 0 || dy > 2 * W || (dy == W && dx == W)) continue;                    // outside it / the pixel itself
                support[p] += (o - lo[p] <= span[p]) ? 1 : 0;
            }
        }
    int n = 0;
#pragma unroll
    for (int p = 0; p < DF_STRIP; ++p) {
        const int r = r0 + ls + p;
        const bool inside = r < h && c < w;
        const bool drop = inside && d[p] > 0 && support[p] < min_support;
        if (inside) depth_out[image + (size_t)r * w + c] = drop ? 0 : d[p];
        n += __popcll(__ballot(drop));                           // wave-uniform
    }
    if (lane == 0 && n > 0) atomicAdd(&removed[img], n);
}

}  // namespace

extern "C" int captra_depth_support_filter(int b, int h, int w, int window, int abs_mm, int rel_permille, int min_support,
                                           const int *depth_in, int *depth_out, int *removed, captra_stream_t stream) {
    if (b < 0 || h < 0 || w < 0 || window < 1 || window > 3 || abs_mm < 0 || rel_permille < 0 || rel_permille > 1000) return -1;
    if (min_support < 1 || min_support > (2 * window + 1) * (2 * window + 1) - 1) return -1;
    if (h > INT_MAX - 128 || w > INT_MAX - 128) return -1;                                   // (tile and halo coordinates are ints)
    if (b == 0 || h == 0 || w == 0) return 0;
    if (depth_in == nullptr || depth_out == nullptr || removed == nullptr) return -1;
    const unsigned long long n = (unsigned long long)b * (unsigned long long)h * (unsigned long long)w;
    if (n > (unsigned long long)PTRDIFF_MAX / sizeof(int)) return -1;
    const uintptr_t pi = (uintptr_t)depth_in, po = (uintptr_t)depth_out;
    if (pi < po + n * sizeof(int) && po < pi + n * sizeof(int)) return -1;                   // the images overlap: decisions are depth_in's
    const int tiles_x = (w - 1) / DF_COLS + 1, tiles_y = (h - 1) / DF_ROWS + 1;
    const unsigned long long tiles = (unsigned long long)b * tiles_x * tiles_y;
    if (tiles > (unsigned long long)INT_MAX) return -1;
    const hipStream_t s = (hipStream_t)stream;
    if (window == 1)
        CAPTRA_LAUNCH("depth_filter", depth_support_filter_kernel<1>, dim3((unsigned)tiles), dim3(DF_T), 0, s, h, w, tiles_x, tiles_y, abs_mm,
                      rel_permille, min_support, depth_in, depth_out, removed);
    else if (window == 2)
        CAPTRA_LAUNCH("depth_filter", depth_support_filter_kernel<2>, dim3((unsigned)tiles), dim3(DF_T), 0, s, h, w, tiles_x, tiles_y, abs_mm,
                      rel_permille, min_support, depth_in, depth_out, removed);
    else
        CAPTRA_LAUNCH("depth_filter", depth_support_filter_kernel<3>, dim3((unsigned)tiles), dim3(DF_T), 0, s, h, w, tiles_x, tiles_y, abs_mm,
                      rel_permille, min_support, depth_in, depth_out, removed);
    return captra_last_error();
}
