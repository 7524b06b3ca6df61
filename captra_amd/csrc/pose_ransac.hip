// RANSAC similarity fit (rotation + scale + translation) between NOCS coordinates and camera points, per (trajectory, part),
// on device for gfx950.
//
// Replaces pose_fit of the reference's datasets/nocs_data/preproc_nocs/align_pose.py:49-93 (host numpy: 64 three-point Umeyama
// hypotheses, the inlier count of each at a distance threshold, the first best one, a refit on its inliers) -- the estimator
// that needs no previous pose.  Semantics: include/captra_hip.h, captra_part_fit_ransac.
//
// One workgroup of RS_THREADS per (b, p):
//   1. compact the members (label == p) in ascending point index into a u16 list in LDS; for N <= RS_LDS_N their six
//      coordinates follow them into LDS (the target with its mean added once), above that they are re-read through the list;
//   2. thread h solves hypothesis h in double: centre the three pairs, kabsch3 on tgt_c^T src_c, scale, translation; the
//      parameters (s R, t) go to LDS as fp32;
//   3. score: a work item is (256 members, 16 hypotheses); a wave holds four members per lane in registers and walks its
//      hypotheses, whose parameters are wave-uniform LDS reads; a member is an inlier when the squared fp32 residual is below
//      th^2, counted by ballot + population count, added to score[h] as an INTEGER (any order gives the same sum);
//   4. best = first h with the largest score; two double block reductions over its inliers (count and centroids, then the
//      centred cross-covariance and source covariance) and one thread finishes the same Umeyama solve.
// The inlier test is one fp32 expression of (member, hypothesis) alone, evaluated by the same inline function in 3. and 4.:
// the inlier set is a pure function of the inputs, whatever the wave that meets the member.
#include "common.h"
#include "pose_solve.h"

#include <math.h>

namespace {

constexpr int RS_THREADS = 1024;
constexpr int RS_WAVES = RS_THREADS / 64;
constexpr int RS_MAX_P = 8, RS_MAX_H = 256, RS_MAX_N = 16384;
constexpr int RS_LDS_N = 4096;         // member coordinates live in LDS up to this N
constexpr int RS_PPL = 4;              // members per lane of a work item
constexpr int RS_HG = 16;              // hypotheses per work item
constexpr int RS_CHUNK = 64 * RS_PPL;

static inline int rs_idx_bytes(int n) { return ((n * 2 + 15) / 16) * 16; }
static inline int rs_lds_bytes(int n) { return rs_idx_bytes(n) + (n <= RS_LDS_N ? 6 * n * 4 : 0); }
constexpr int RS_LDS_MAX = RS_LDS_N * 2 + 6 * RS_LDS_N * 4;      // 104 KiB at N = 4096; N = 16384 needs 32 KiB (the list alone)
static_assert(RS_LDS_MAX >= RS_MAX_N * 2, "the member list of the largest N fits");

template <int NV>
__device__ __forceinline__ void rs_block_sum(double (&v)[NV], double *smem /* [NV][RS_WAVES] */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        double x = v[i];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
        v[i] = x;
    }
    __syncthreads();
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < NV; ++i) smem[i * RS_WAVES + wave] = v[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        double x = 0.0;
#pragma unroll
        for (int w = 0; w < RS_WAVES; ++w) x += smem[i * RS_WAVES + w];
        v[i] = x;
    }
}

// splitmix64's finaliser: the draw generator of captra_part_fit_ransac (include/captra_hip.h)
__device__ __forceinline__ unsigned long long rs_mix(unsigned long long z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ unsigned rs_draw(unsigned long long key, int bi, int pi, int h, int draw) {
    const unsigned long long ctr = ((unsigned long long)(unsigned)bi << 32) | ((unsigned long long)pi << 24) | ((unsigned long long)h << 8) |
                                   (unsigned long long)draw;
    return (unsigned)(rs_mix(key ^ ctr) >> 32);
}

// where the members of this (b, p) are
struct RsMembers {
    const float *S, *T;              // global, channel-major, stride n
    int n;
    float tm[3];
    bool has_tm, in_lds;
    const unsigned short *idx;       // LDS: point index of member m
    const float *co;                 // LDS: [6][n] src xyz, tgt xyz of member m (in_lds)
    __device__ __forceinline__ void load(int m, float s[3], float t[3]) const {
        if (in_lds) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                s[a] = co[a * n + m];
                t[a] = co[(3 + a) * n + m];
            }
        } else {
            const int i = idx[m];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                s[a] = S[(size_t)a * n + i];
                const float tv = T[(size_t)a * n + i];
                t[a] = has_tm ? tv + tm[a] : tv;
            }
        }
    }
};

// |t - (sR s + tr)|^2 < th2, every operation a separately rounded fp32 one; a NaN residual is no inlier
__device__ __forceinline__ bool rs_inlier(const float s[3], const float t[3], const float hp[12], float th2) {
    float e[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float pr = ((hp[a * 3] * s[0] + hp[a * 3 + 1] * s[1]) + hp[a * 3 + 2] * s[2]) + hp[9 + a];
        e[a] = t[a] - pr;
    }
    return (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2] < th2;
}

// Umeyama from the centred moments: M[a][c] = sum tc_a sc_c, Css = sum sc sc^T (xx xy xz yy yz zz), centroids sb / tb
//   R = kabsch3(M); s = <R, M> / (<R^T R, Css> + 1e-6) = sum (R sc).tc / (sum |R sc|^2 + 1e-6); t = tb - s R sb = mean(tgt - s R src)
__device__ void rs_umeyama(const double M[9], const double C6[6], const double sb[3], const double tb[3], double R[9], double *sc_out,
                           double tr[3]) {
    kabsch3(M, R);
    double num = 0;
    for (int i = 0; i < 9; ++i) num += R[i] * M[i];
    const double Css[9] = {C6[0], C6[1], C6[2], C6[1], C6[3], C6[4], C6[2], C6[4], C6[5]};
    double dn = 0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double g = 0;
            for (int k = 0; k < 3; ++k) g += R[k * 3 + i] * R[k * 3 + j];
            dn += g * Css[i * 3 + j];
        }
    const double sca = num / (dn + 1e-6);
    for (int a = 0; a < 3; ++a) tr[a] = tb[a] - sca * (R[a * 3] * sb[0] + R[a * 3 + 1] * sb[1] + R[a * 3 + 2] * sb[2]);
    *sc_out = sca;
}

__global__ __launch_bounds__(RS_THREADS) void part_fit_ransac_kernel(int p, int n, int num_hyps, float th, int tgt_per_part,
                                                                     const int *__restrict__ labels, const float *__restrict__ src,
                                                                     const float *__restrict__ tgt, const float *__restrict__ tgt_mean,
                                                                     const int *__restrict__ sample_rank, unsigned long long seed,
                                                                     float *__restrict__ rot, float *__restrict__ scale,
                                                                     float *__restrict__ trans, int *__restrict__ valid,
                                                                     int *__restrict__ best_out, int *__restrict__ num_inliers,
                                                                     int *__restrict__ samples_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rs_dyn[];
    __shared__ float s_hp[RS_MAX_H * 12];
    __shared__ int s_score[RS_MAX_H];
    __shared__ double s_red[15 * RS_WAVES];
    __shared__ int s_wcnt[RS_WAVES];
    __shared__ int s_best;

    const int q = blockIdx.x;
    const int bi = q / p, pi = q % p;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int *lab = labels + (size_t)bi * n;
    unsigned short *idx = reinterpret_cast<unsigned short *>(rs_dyn);
    float *co = reinterpret_cast<float *>(rs_dyn + ((n * 2 + 15) / 16) * 16);

    RsMembers mem;
    mem.S = src + (size_t)q * 3 * n;
    mem.T = tgt + (size_t)(tgt_per_part ? q : bi) * 3 * n;
    mem.n = n;
    mem.has_tm = tgt_mean != nullptr;
#pragma unroll
    for (int a = 0; a < 3; ++a) mem.tm[a] = tgt_mean ? tgt_mean[bi * 3 + a] : 0.f;
    mem.in_lds = n <= RS_LDS_N;
    mem.idx = idx;
    mem.co = co;

    // ---- 1. members, in ascending point index
    int count = 0;
    for (int base = 0; base < n; base += RS_THREADS) {
        const int i = base + tid;
        const bool in = i < n && lab[i] == pi;
        const unsigned long long bal = __ballot(in);
        if (lane == 0) s_wcnt[wave] = __popcll(bal);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < RS_WAVES; ++w) {
            const int c = s_wcnt[w];
            before += w < wave ? c : 0;
            total += c;
        }
        if (in) idx[count + before + __popcll(bal & ((1ull << lane) - 1ull))] = (unsigned short)i;
        count += total;
        __syncthreads();
    }
    if (mem.in_lds) {
        for (int m = tid; m < count; m += RS_THREADS) {
            const int i = idx[m];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                co[a * n + m] = mem.S[(size_t)a * n + i];
                const float tv = mem.T[(size_t)a * n + i];
                co[(3 + a) * n + m] = mem.has_tm ? tv + mem.tm[a] : tv;
            }
        }
    }
    if (tid < RS_MAX_H) s_score[tid] = 0;
    __syncthreads();

    int best = 0, ninl = 0;
    bool ok = false;
    float Rf[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, scf = 1.f, trf[3] = {0.f, 0.f, 0.f};

    if (count >= 3) {       // (uniform over the workgroup: the barriers below are met by all or none)
        // ---- 2. one hypothesis per thread
        if (tid < num_hyps) {
            const int h = tid;
            unsigned r[3];
            if (sample_rank != nullptr) {
                for (int j = 0; j < 3; ++j) r[j] = (unsigned)sample_rank[((size_t)q * num_hyps + h) * 3 + j] % (unsigned)count;
            } else {
                const unsigned long long key = rs_mix(seed + 0x9E3779B97F4A7C15ull);
                r[0] = rs_draw(key, bi, pi, h, 0) % (unsigned)count;
                r[1] = rs_draw(key, bi, pi, h, 1) % (unsigned)(count - 1);
                r[2] = rs_draw(key, bi, pi, h, 2) % (unsigned)(count - 2);
                if (r[1] >= r[0]) ++r[1];
                const unsigned lo = r[0] < r[1] ? r[0] : r[1], hi = r[0] < r[1] ? r[1] : r[0];
                if (r[2] >= lo) ++r[2];
                if (r[2] >= hi) ++r[2];
            }
            double S3[3][3], T3[3][3], sb[3] = {0, 0, 0}, tb[3] = {0, 0, 0};
            for (int j = 0; j < 3; ++j) {
                float s[3], t[3];
                mem.load((int)r[j], s, t);
                for (int a = 0; a < 3; ++a) {
                    S3[j][a] = s[a];
                    T3[j][a] = t[a];
                    sb[a] += s[a];
                    tb[a] += t[a];
                }
                if (samples_out != nullptr) samples_out[((size_t)q * num_hyps + h) * 3 + j] = idx[r[j]];
            }
            for (int a = 0; a < 3; ++a) {
                sb[a] /= 3.0;
                tb[a] /= 3.0;
            }
            double M[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, C6[6] = {0, 0, 0, 0, 0, 0};
            for (int j = 0; j < 3; ++j) {
                double sc[3], tc[3];
                for (int a = 0; a < 3; ++a) {
                    sc[a] = S3[j][a] - sb[a];
                    tc[a] = T3[j][a] - tb[a];
                }
                for (int a = 0; a < 3; ++a)
                    for (int c = 0; c < 3; ++c) M[a * 3 + c] += tc[a] * sc[c];
                C6[0] += sc[0] * sc[0]; C6[1] += sc[0] * sc[1]; C6[2] += sc[0] * sc[2];
                C6[3] += sc[1] * sc[1]; C6[4] += sc[1] * sc[2]; C6[5] += sc[2] * sc[2];
            }
            double R[9], sca, tr[3];
            rs_umeyama(M, C6, sb, tb, R, &sca, tr);
            for (int i = 0; i < 9; ++i) s_hp[h * 12 + i] = (float)(sca * R[i]);
            for (int a = 0; a < 3; ++a) s_hp[h * 12 + 9 + a] = (float)tr[a];
        }
        __syncthreads();

        // ---- 3. scores
        const float th2 = th * th;
        const int chunks = (count + RS_CHUNK - 1) / RS_CHUNK, groups = (num_hyps + RS_HG - 1) / RS_HG;
        for (int item = wave; item < chunks * groups; item += RS_WAVES) {
            const int c = item / groups, g = item % groups;
            float s[RS_PPL][3], t[RS_PPL][3];
            bool have[RS_PPL];
#pragma unroll
            for (int k = 0; k < RS_PPL; ++k) {
                const int m = c * RS_CHUNK + k * 64 + lane;
                have[k] = m < count;
                mem.load(have[k] ? m : 0, s[k], t[k]);
            }
            int mine = 0;
            const int h1 = (g + 1) * RS_HG < num_hyps ? (g + 1) * RS_HG : num_hyps;
            for (int h = g * RS_HG; h < h1; ++h) {
                float hp[12];
#pragma unroll
                for (int i = 0; i < 12; ++i) hp[i] = s_hp[h * 12 + i];
                int pc = 0;
#pragma unroll
                for (int k = 0; k < RS_PPL; ++k) pc += __popcll(__ballot(have[k] && rs_inlier(s[k], t[k], hp, th2)));
                mine = (lane == h - g * RS_HG) ? pc : mine;
            }
            if (g * RS_HG + lane < h1) atomicAdd(&s_score[g * RS_HG + lane], mine);
        }
        __syncthreads();

        // ---- 4. the first best hypothesis (largest score, then smallest h), and the refit on its inliers
        if (wave == 0) {
            int key = -1;
            for (int h = lane; h < num_hyps; h += 64) {
                const int k = (s_score[h] << 9) | (511 - h);
                key = k > key ? k : key;
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const int o = __shfl_xor(key, off, 64);
                key = o > key ? o : key;
            }
            if (lane == 0) s_best = 511 - (key & 511);
        }
        __syncthreads();
        best = s_best;
        ninl = s_score[best];
        float hp[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) hp[i] = s_hp[best * 12 + i];

        if (ninl >= 3) {    // (uniform)
            double r1[7] = {0, 0, 0, 0, 0, 0, 0};
            for (int m = tid; m < count; m += RS_THREADS) {
                float s[3], t[3];
                mem.load(m, s, t);
                if (rs_inlier(s, t, hp, th2)) {
                    r1[0] += 1.0;
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        r1[1 + a] += (double)s[a];
                        r1[4 + a] += (double)t[a];
                    }
                }
            }
            rs_block_sum<7>(r1, s_red);
            const double cnt = r1[0];
            const double sb[3] = {r1[1] / cnt, r1[2] / cnt, r1[3] / cnt}, tb[3] = {r1[4] / cnt, r1[5] / cnt, r1[6] / cnt};
            double r2[15];
#pragma unroll
            for (int i = 0; i < 15; ++i) r2[i] = 0.0;
            for (int m = tid; m < count; m += RS_THREADS) {
                float s[3], t[3];
                mem.load(m, s, t);
                if (rs_inlier(s, t, hp, th2)) {
                    double sc[3], tc[3];
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        sc[a] = (double)s[a] - sb[a];
                        tc[a] = (double)t[a] - tb[a];
                    }
#pragma unroll
                    for (int a = 0; a < 3; ++a)
#pragma unroll
                        for (int c = 0; c < 3; ++c) r2[a * 3 + c] += tc[a] * sc[c];
                    r2[9] += sc[0] * sc[0]; r2[10] += sc[0] * sc[1]; r2[11] += sc[0] * sc[2];
                    r2[12] += sc[1] * sc[1]; r2[13] += sc[1] * sc[2]; r2[14] += sc[2] * sc[2];
                }
            }
            rs_block_sum<15>(r2, s_red);
            if (tid == 0) {
                double R[9], sca, tr[3];
                rs_umeyama(r2, r2 + 9, sb, tb, R, &sca, tr);
                float fR[9], fs = (float)sca, ft[3] = {(float)tr[0], (float)tr[1], (float)tr[2]};
                float chk = fs + ((ft[0] + ft[1]) + ft[2]);
                for (int i = 0; i < 9; ++i) {
                    fR[i] = (float)R[i];
                    chk += fR[i];
                }
                ok = isfinite(chk);
                if (ok) {
                    for (int i = 0; i < 9; ++i) Rf[i] = fR[i];
                    scf = fs;
                    for (int a = 0; a < 3; ++a) trf[a] = ft[a];
                }
            }
        }
    } else if (samples_out != nullptr) {
        for (int i = tid; i < num_hyps * 3; i += RS_THREADS) samples_out[(size_t)q * num_hyps * 3 + i] = -1;
    }

    if (tid == 0) {
        for (int i = 0; i < 9; ++i) rot[(size_t)q * 9 + i] = Rf[i];
        scale[q] = scf;
        for (int a = 0; a < 3; ++a) trans[(size_t)q * 3 + a] = trf[a];
        valid[q] = ok ? 1 : 0;
        if (best_out != nullptr) best_out[q] = best;
        if (num_inliers != nullptr) num_inliers[q] = ninl;
    }
}

}  // namespace

extern "C" int captra_part_fit_ransac(int b, int p, int n, int num_hyps, float inlier_th, const int *labels, const float *src,
                                      const float *tgt, int tgt_per_part, const float *tgt_mean, const int *sample_rank,
                                      unsigned long long seed, float *rot, float *scale, float *trans, int *valid, int *best,
                                      int *num_inliers, int *samples_out, captra_stream_t stream) {
    if (b < 0 || p < 1 || p > RS_MAX_P || n < 1 || n > RS_MAX_N || num_hyps < 1 || num_hyps > RS_MAX_H) return -1;
    if (b == 0) return 0;
    constexpr auto kern = part_fit_ransac_kernel;
    if (int e = captra_allow_lds<kern>(RS_LDS_MAX)) return e;
    CAPTRA_LAUNCH("part_fit_ransac", kern, dim3(b * p), dim3(RS_THREADS), rs_lds_bytes(n), (hipStream_t)stream, p, n, num_hyps,
                  inlier_th, tgt_per_part, labels, src, tgt, tgt_mean, sample_rank, seed, rot, scale, trans, valid, best, num_inliers,
                  samples_out);
    return captra_last_error();
}
