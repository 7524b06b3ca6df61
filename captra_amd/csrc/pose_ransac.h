// The RANSAC similarity fit of one (trajectory, part) by one workgroup of RS_THREADS, shared by pose_ransac.hip
// (captra_part_fit_ransac: the fit alone) and pose_guard.hip (captra_part_fit_guard: the fit behind a check of the tracked pose).
// Both kernels go through the same three device functions in the same order, so the same inputs and draws give the same bits:
//   rs_list_members : the members (label == p) in ascending point index into a u16 list in LDS;
//   rs_stage_members: for N <= RS_LDS_N their six coordinates follow them into LDS (the target with its mean added once), above
//                     that they are re-read through the list;
//   rs_fit          : hypotheses, scores, first best, refit on its inliers (the stages are described in pose_ransac.hip).
#pragma once
#include "common.h"
#include "pose_solve.h"
#include "wave_ops.h"

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

// the static LDS of a workgroup that fits
struct RsLds {
    float hp[RS_MAX_H * 12];
    int score[RS_MAX_H];
    double red[15 * RS_WAVES];
    int wcnt[RS_WAVES];
    int best;
};

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
    unsigned short *idx;             // LDS: point index of member m
    float *co;                       // LDS: [6][n] src xyz, tgt xyz of member m (in_lds)
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

// The members of one (b, p) from a kernel's arguments: S / T its source and target rows, tgt_mean (B,3) or NULL, dyn the kernel's
// dynamic LDS (the index list, then the coordinates); nothing is staged yet (rs_stage_members)
__device__ __forceinline__ RsMembers rs_members(const float *S, const float *T, int n, const float *tgt_mean, int bi, unsigned char *dyn) {
    unsigned short *idx = reinterpret_cast<unsigned short *>(dyn);
    float *co = reinterpret_cast<float *>(dyn + ((n * 2 + 15) / 16) * 16);
    RsMembers mem;
    mem.S = S;
    mem.T = T;
    mem.n = n;
    mem.has_tm = tgt_mean != nullptr;
#pragma unroll
    for (int a = 0; a < 3; ++a) mem.tm[a] = tgt_mean ? tgt_mean[bi * 3 + a] : 0.f;
    mem.in_lds = false;
    mem.idx = idx;
    mem.co = co;
    return mem;
}

// The members of part pi among lab[0..n), in ascending point index, into idx; -> their number (uniform over the workgroup).
__device__ __forceinline__ int rs_list_members(const int *__restrict__ lab, int pi, int n, unsigned short *idx, int *s_wcnt) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
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
    return count;
}

// The members' coordinates into LDS (N <= RS_LDS_N; mem.in_lds says which regime holds afterwards).  Ends with a barrier.
__device__ __forceinline__ void rs_stage_members(RsMembers &mem, int count) {
    const int n = mem.n;
    float *co = mem.co;
    mem.in_lds = n <= RS_LDS_N;
    if (mem.in_lds) {
        for (int m = threadIdx.x; m < count; m += RS_THREADS) {
            const int i = mem.idx[m];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                co[a * n + m] = mem.S[(size_t)a * n + i];
                const float tv = mem.T[(size_t)a * n + i];
                co[(3 + a) * n + m] = mem.has_tm ? tv + mem.tm[a] : tv;
            }
        }
    }
    __syncthreads();
}

// The first best hypothesis: the largest score, then the smallest h (num_hyps <= 512, scores < 2^22).  One whole wave calls it; every
// lane gets the answer.
__device__ __forceinline__ int rs_first_best(const int *score, int num_hyps) {
    int key = -1;
    for (int h = (int)(threadIdx.x & 63); h < num_hyps; h += 64) {
        const int k = (score[h] << 9) | (511 - h);
        key = k > key ? k : key;
    }
    WAVE_BUTTERFLY(key, 32, imax);
    return 511 - (key & 511);
}

// Umeyama from the centred moments: M[a][c] = sum tc_a sc_c, Css = sum sc sc^T (xx xy xz yy yz zz), centroids sb / tb
//   R = kabsch3(M); s = <R, M> / (<R^T R, Css> + 1e-6) = sum (R sc).tc / (sum |R sc|^2 + 1e-6); t = tb - s R sb = mean(tgt - s R src)
__device__ void rs_umeyama(const double M[9], const double C6[6], const double sb[3], const double tb[3], double R[9], double *sc_out,
                           double tr[3]) {
    kabsch3(M, R);
    *sc_out = ps_scale(R, M, C6);
    ps_trans(R, *sc_out, sb, tb, tr);
}

// The SOLVER of rs_fit: what turns the centred moments of a set of pairs (three members, or the winner's inliers) into a pose.
// RsUmeyama is the similarity fit above (rotation, scale, translation all free).
struct RsUmeyama {
    __device__ __forceinline__ void operator()(const double M[9], const double C6[6], const double sb[3], const double tb[3], double R[9],
                                               double *sc_out, double tr[3]) const {
        rs_umeyama(M, C6, sb, tb, R, sc_out, tr);
    }
};

// RsGivenRot: the rotation R0 is GIVEN (the workgroup's), scale and translation are fitted -- the algebra of part_fit_st_kernel
// (pose_fit.hip) on the same moments, by the same functions (pose_solve.h): SYM takes the in-plane rotation about y first.
template <bool SYM>
struct RsGivenRot {
    double R0[9];
    __device__ void operator()(const double M[9], const double C6[6], const double sb[3], const double tb[3], double R[9], double *sc_out,
                               double tr[3]) const {
        if constexpr (SYM) ps_rot_about_y(R0, M, R);
        else for (int i = 0; i < 9; ++i) R[i] = R0[i];
        *sc_out = ps_scale(R, M, C6);
        ps_trans(R, *sc_out, sb, tb, tr);
    }
};

// RsGivenRotScale: the rotation R0 AND the scale s are given, the translation is fitted -- captra_part_fit_st with given_scale on a
// set of pairs: RsGivenRot with s in place of ps_scale (SYM still takes the in-plane rotation from the moments first: that step does
// not depend on s).  The solver of captra_part_fit_st_size's held fit (pose_size.hip).
template <bool SYM>
struct RsGivenRotScale {
    double R0[9], s;
    __device__ void operator()(const double M[9], const double C6[6], const double sb[3], const double tb[3], double R[9], double *sc_out,
                               double tr[3]) const {
        if constexpr (SYM) ps_rot_about_y(R0, M, R);
        else for (int i = 0; i < 9; ++i) R[i] = R0[i];
        *sc_out = s;
        ps_trans(R, s, sb, tb, tr);
    }
};

// What rs_fit found: best / ninl are uniform over the workgroup, ok and the pose are thread 0's (identity / 1 / 0 when not ok).
struct RsResult {
    int best = 0, ninl = 0;
    bool ok = false;
    float R[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, sc = 1.f, tr[3] = {0.f, 0.f, 0.f};
};

// Stages 2-4 of the fit on the `count` listed members of part (bi, pi); q = the part's index in this launch (sample_rank /
// samples_out rows), key_b = the trajectory's index in the draw key.  Every thread of the workgroup calls it (barriers inside);
// with count < 3 nothing is drawn or scored.  SYM: a hypothesis is scored, and the winner's inliers are selected, by the axis-only
// test (pose_solve.h) on (fp32 second column of R_h, fp32 s_h, fp32 t_h) -- seven floats in the same twelve-float slot; draws,
// hypotheses, work items, first best, the refit and the validity rule are the same code.  Solver: what fits a pose to a set of pairs,
// a compile-time policy used for the hypotheses and for the refit alike (RsUmeyama: the similarity fit; RsGivenRot: scale and
// translation under the workgroup's rotation, captra_part_fit_st_ransac).
template <bool SYM, class Solver = RsUmeyama>
__device__ __forceinline__ void rs_fit(const RsMembers &mem, int count, int q, int key_b, int pi, int num_hyps, float th,
                                       const int *__restrict__ sample_rank, unsigned long long seed, int *__restrict__ samples_out,
                                       RsLds &L, RsResult &res, const Solver &solve = Solver()) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned short *idx = mem.idx;
    if (tid < RS_MAX_H) L.score[tid] = 0;
    __syncthreads();

    if (count >= 3) {       // (uniform over the workgroup: the barriers below are met by all or none)
        // ---- 2. one hypothesis per thread
        if (tid < num_hyps) {
            const int h = tid;
            unsigned r[3];
            if (sample_rank != nullptr) {
                for (int j = 0; j < 3; ++j) r[j] = (unsigned)sample_rank[((size_t)q * num_hyps + h) * 3 + j] % (unsigned)count;
            } else {
                const unsigned long long key = rs_mix(seed + 0x9E3779B97F4A7C15ull);
                r[0] = rs_draw(key, key_b, pi, h, 0) % (unsigned)count;
                r[1] = rs_draw(key, key_b, pi, h, 1) % (unsigned)(count - 1);
                r[2] = rs_draw(key, key_b, pi, h, 2) % (unsigned)(count - 2);
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
            solve(M, C6, sb, tb, R, &sca, tr);
            if constexpr (SYM) {
                for (int a = 0; a < 3; ++a) L.hp[h * 12 + a] = (float)R[a * 3 + 1];
                L.hp[h * 12 + 3] = (float)sca;
                for (int a = 0; a < 3; ++a) L.hp[h * 12 + 4 + a] = (float)tr[a];
            } else {
                for (int i = 0; i < 9; ++i) L.hp[h * 12 + i] = (float)(sca * R[i]);
                for (int a = 0; a < 3; ++a) L.hp[h * 12 + 9 + a] = (float)tr[a];
            }
        }
        __syncthreads();

        // ---- 3. scores
        using Test = RsTest<SYM>;
        const float th2 = th * th;
        const int chunks = (count + RS_CHUNK - 1) / RS_CHUNK, groups = (num_hyps + RS_HG - 1) / RS_HG;
        for (int item = wave; item < chunks * groups; item += RS_WAVES) {
            const int c = item / groups, g = item % groups;
            float s[RS_PPL][3], t[RS_PPL][3], rho[RS_PPL];
            bool have[RS_PPL];
#pragma unroll
            for (int k = 0; k < RS_PPL; ++k) {
                const int m = c * RS_CHUNK + k * 64 + lane;
                have[k] = m < count;
                mem.load(have[k] ? m : 0, s[k], t[k]);
                rho[k] = SYM ? rs_sym_radius(s[k]) : 0.f;       // (once per member, not per hypothesis)
            }
            int mine = 0;
            const int h1 = (g + 1) * RS_HG < num_hyps ? (g + 1) * RS_HG : num_hyps;
            for (int h = g * RS_HG; h < h1; ++h) {
                float hp[Test::NPAR];
#pragma unroll
                for (int i = 0; i < Test::NPAR; ++i) hp[i] = L.hp[h * 12 + i];
                int pc = 0;
#pragma unroll
                for (int k = 0; k < RS_PPL; ++k) pc += __popcll(__ballot(have[k] && Test::inlier(s[k], rho[k], t[k], hp, th2)));
                mine = (lane == h - g * RS_HG) ? pc : mine;
            }
            if (g * RS_HG + lane < h1) atomicAdd(&L.score[g * RS_HG + lane], mine);
        }
        __syncthreads();

        // ---- 4. the first best hypothesis (largest score, then smallest h), and the refit on its inliers
        if (wave == 0) {
            const int best = rs_first_best(L.score, num_hyps);
            if (lane == 0) L.best = best;
        }
        __syncthreads();
        res.best = L.best;
        res.ninl = L.score[res.best];
        float hp[Test::NPAR];
#pragma unroll
        for (int i = 0; i < Test::NPAR; ++i) hp[i] = L.hp[res.best * 12 + i];

        if (res.ninl >= 3) {    // (uniform)
            double r1[7] = {0, 0, 0, 0, 0, 0, 0};
            for (int m = tid; m < count; m += RS_THREADS) {
                float s[3], t[3];
                mem.load(m, s, t);
                if (Test::inlier(s, SYM ? rs_sym_radius(s) : 0.f, t, hp, th2)) {
                    r1[0] += 1.0;
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        r1[1 + a] += (double)s[a];
                        r1[4 + a] += (double)t[a];
                    }
                }
            }
            wg_sum<WG_SUM_SERIAL, RS_WAVES>(r1, L.red);
            const double cnt = r1[0];
            const double sb[3] = {r1[1] / cnt, r1[2] / cnt, r1[3] / cnt}, tb[3] = {r1[4] / cnt, r1[5] / cnt, r1[6] / cnt};
            double r2[15];
#pragma unroll
            for (int i = 0; i < 15; ++i) r2[i] = 0.0;
            for (int m = tid; m < count; m += RS_THREADS) {
                float s[3], t[3];
                mem.load(m, s, t);
                if (Test::inlier(s, SYM ? rs_sym_radius(s) : 0.f, t, hp, th2)) {
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
            wg_sum<WG_SUM_SERIAL, RS_WAVES>(r2, L.red);
            if (tid == 0) {
                double R[9], sca, tr[3];
                solve(r2, r2 + 9, sb, tb, R, &sca, tr);
                float fR[9], fs = (float)sca, ft[3] = {(float)tr[0], (float)tr[1], (float)tr[2]};
                float chk = fs + ((ft[0] + ft[1]) + ft[2]);
                for (int i = 0; i < 9; ++i) {
                    fR[i] = (float)R[i];
                    chk += fR[i];
                }
                res.ok = isfinite(chk);
                if (res.ok) {
                    for (int i = 0; i < 9; ++i) res.R[i] = fR[i];
                    res.sc = fs;
                    for (int a = 0; a < 3; ++a) res.tr[a] = ft[a];
                }
            }
        }
    } else if (samples_out != nullptr) {
        for (int i = tid; i < num_hyps * 3; i += RS_THREADS) samples_out[(size_t)q * num_hyps * 3 + i] = -1;
    }
}

}  // namespace
