// Shared device/host helpers for libcaptra_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "captra_hip.h"   // captra_launch_opts, captra_stream_t

#define CAPTRA_WAVE 64


// ---- profiling hooks (prof.cpp) -------------------------------------------------------------
// CAPTRA_LAUNCH brackets a kernel launch with HIP events on the launch stream when profiling
// is enabled (captra_prof_enable).  Outside profiling it costs one relaxed load.
struct CaptraProfScope {
    int slot;
    hipStream_t stream;
    CaptraProfScope(const char *name, hipStream_t s);
    ~CaptraProfScope();
};

#define CAPTRA_LAUNCH(name, kernel, grid, block, shmem, stream, ...)                     \
    do {                                                                                 \
        CaptraProfScope _scope(name, stream);                                            \
        hipLaunchKernelGGL(kernel, grid, block, shmem, stream, __VA_ARGS__);             \
    } while (0)

// In-kernel phase timers of the SA kernels (captra_sa_fused_set_prof, tools/bench_sa_fused.py --phases) exist only in a build with
// -DCAPTRA_SA_PROF=1 (CAPTRA_HIPCC_EXTRA): the runtime test `p.prof != nullptr` alone -- a branch at every phase boundary, which
// the scheduler cannot move anything across -- costs the fp32 SA1 scales 2.7 %, the SA2 scales 1-2 % and cost the bf16 SA2 kernel
// a third (same-box A/B of two builds, CAPTRA_LIB).
#ifndef CAPTRA_SA_PROF
#define CAPTRA_SA_PROF 0
#endif
#define CAPTRA_PROF_ON(ptr) (CAPTRA_SA_PROF != 0 && (ptr) != nullptr)

// Ablation instantiations and timing modes whose RESULTS ARE WRONG BY CONSTRUCTION (measurement only: tools/bench_l1_stream.py,
// tools/bf16_variants.sh) exist only in a build with -DCAPTRA_ABLATIONS=1 (CAPTRA_HIPCC_EXTRA); the shipped library ignores their knobs.
#ifndef CAPTRA_ABLATIONS
#define CAPTRA_ABLATIONS 0
#endif

// Per-call options (include/captra_hip.h captra_launch_opts; NULL = defaults): the library keeps no product-affecting state.
// CUs a persistent launch leaves free
static inline int captra_reserved_cus(const captra_launch_opts *o) { return (o != nullptr && o->reserved_cus > 0) ? o->reserved_cus : 0; }
// the call's centre window clipped to [0, m); true when one is given
static inline bool captra_centre_window(const captra_launch_opts *o, int m, int *m0, int *mc) {
    if (o == nullptr || o->centre_mc <= 0) { *m0 = 0; *mc = m; return false; }
    const int w0 = o->centre_m0 < 0 ? 0 : o->centre_m0;
    *m0 = w0 < m ? w0 : m;
    *mc = o->centre_mc < m - *m0 ? o->centre_mc : m - *m0;
    return true;
}

static inline int captra_last_error() { return (int)hipGetLastError(); }

// ---- per-device launch plumbing: dynamic-LDS limit, CU count, occupancy ------------------------------------------------------------
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is per DEVICE: a process that launches on a second GPU must set it
// there too.  Launchers do not use this struct themselves; in front of the launch they write
//     if (int e = captra_allow_lds<three_interpolate_kernel>(TI_LDS_BYTES)) return e;
// first_use() only LOOKS (true until done() ran for the current device): the device is marked after the attribute call
// returned, so a second host thread racing the first either sees the mark (attribute already applied) or applies it
// itself (idempotent) -- it can never launch with more dynamic LDS than the attribute allows yet.
#include <atomic>
struct CaptraDeviceOnce {
    std::atomic<unsigned long long> seen[2] = {{0ull}, {0ull}};   // device ordinals 0..127
    static int device() {
        int dev = 0;
        return (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 128) ? dev : -1;
    }
    bool first_use() const {
        const int dev = device();
        if (dev < 0) return true;                                  // unknown device: always (re)set
        return (seen[dev >> 6].load(std::memory_order_acquire) & (1ull << (dev & 63))) == 0ull;
    }
    void done() {
        const int dev = device();
        if (dev >= 0) seen[dev >> 6].fetch_or(1ull << (dev & 63), std::memory_order_release);
    }
};

// Let kernel `Kern` be launched with up to `bytes` of dynamic LDS on the current device: 0, or the HIP error.  The one-shot belongs
// to the KERNEL (one per instantiation of this template), not to the call site: a launcher that picks one of several variants at run
// time calls this for the variant it is about to launch, and none of them can go without.  A failure is not remembered (the next
// launch tries again).
template <auto Kern>
int captra_allow_lds(int bytes) {
    static CaptraDeviceOnce once;
    if (!once.first_use()) return 0;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) { (void)hipGetLastError(); return (int)e; }
    once.done();
    return 0;
}

// CUs of the current device (256 when the query fails), from one table per process (prof.cpp): once the device's entry is there,
// hipGetDevice is the only runtime call -- launches happen during graph capture.
int captra_device_cus();
// ... minus the CUs a persistent launch leaves free (captra_launch_opts::reserved_cus), at least 1
static inline int captra_free_cus(const captra_launch_opts *o) {
    const int cus = captra_device_cus() - captra_reserved_cus(o);
    return cus > 0 ? cus : 1;
}

// Workgroups of `Kern` (`threads` wide, `lds_bytes` of dynamic LDS) resident on a CU, at least 1: asked once per kernel and device,
// AFTER captra_allow_lds<Kern> (the answer depends on the attribute).
template <auto Kern>
int captra_blocks_per_cu(int threads, int lds_bytes) {
    static std::atomic<int> per_cu_of[128];
    const int dev = CaptraDeviceOnce::device();
    int per_cu = dev >= 0 ? per_cu_of[dev].load(std::memory_order_relaxed) : 0;
    if (per_cu == 0) {
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, Kern, threads, lds_bytes) != hipSuccess || per_cu < 1) per_cu = 1;
        if (dev >= 0) per_cu_of[dev].store(per_cu, std::memory_order_relaxed);
    }
    return per_cu;
}

// debug / experiment knobs (captra_*_set_*): thread-local so that one host thread's A/B switch never changes what
// another thread (another GPU's stream in the same process) launches; the reference boundary has no global state.
#define CAPTRA_KNOB thread_local

// Zero `nbytes` (a multiple of 16, 16-byte aligned) on `stream` with a KERNEL (prof.cpp).  Not hipMemsetAsync: inside a captured
// hipGraph a memset node is not a kernel node, and in a graph that is ONE linear chain (the step with the networks one after the
// other) the fill was observed to overlap the kernel behind it at 64+ KiB -- the level-1 stream kernel's granules zeroed after its
// samplers had published them (consumers gave up waiting, garbage picks); a kernel node is ordered like every other launch.
int captra_zero_async(void *p, size_t nbytes, hipStream_t stream);

// ---- device helpers ---------------------------------------------------------------------------
__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63); }

// squared distance exactly as the reference kernels and the oracle write it:
// ((dx*dx + dy*dy) + dz*dz), every operation rounded separately (build uses -ffp-contract=off).
__device__ __forceinline__ float dist2_unfused(float ax, float ay, float az, float bx, float by,
                                               float bz) {
    float dx = ax - bx, dy = ay - by, dz = az - bz;
    float xx = dx * dx, yy = dy * dy, zz = dz * dz;
    return (xx + yy) + zz;
}

// activation codes of the shared-MLP entry points (include/captra_hip.h: CAPTRA_ACT_*)
enum { ACT_NONE = 0, ACT_RELU = 1, ACT_SIGMOID_M05 = 2 };

// ReLU as the reference's F.relu: a NaN of either sign and any payload stays that NaN (the fp32 MFMA itself generates the sign-SET
// 0xFFC00000 from Inf - Inf, so a max on the bit pattern as a signed integer, one v_max_i32, turns exactly the NaNs a layer makes
// into 0).  A compare and a select on the untouched bits: written as fmaxf(v, 0) the compiler emits a canonicalising
// v_max_f32 x, x, x in front of a v_max_f32 x, 0 that returns the 0 for a quiet NaN (IEEE mode).  -0 and negatives give +0.
// (The name is from the integer form it replaces; it no longer works on the bit pattern.  Every caller takes the new form and its
// second instruction: the exact-fp32 dense kernels, the generic SA kernel, GroupNorm, and through apply_act the f32x6 and bf16 kernels'
// epilogues (dense_x6, sa_x6, chain_x6, bf16_*), whose finite results are unchanged and whose NaN propagation is not tested.)
__device__ __forceinline__ float relu_bits(float v) {
    return v <= 0.f ? 0.f : v;
}
// ReLU in front of a max pool, as a bit pattern: 0 for -0 and negatives, the value's own bits for a positive number, and a NaN
// with its sign cleared.  The results are non-negative signed integers ordered as torch.max orders them (a NaN above +Inf), so
// the pool behind it is an integer max (imax / imax_dpp, wave_ops.h) and hands a NaN on.
__device__ __forceinline__ int relu_pool_bits(float v) {
    return v <= 0.f ? 0 : (__float_as_int(v) & 0x7FFFFFFF);
}
// max of two floats that hands a NaN of either operand on (torch.max); fmaxf returns the other operand
__device__ __forceinline__ float max_nan(float a, float b) {
    const float m = a <= b ? b : a;          // a NaN a: a
    return b != b ? b : m;
}
__device__ __forceinline__ float apply_act(float v, int act) {
    if (act == ACT_RELU) return relu_bits(v);
    if (act == ACT_SIGMOID_M05) return 1.0f / (1.0f + expf(-v)) - 0.5f;
    return v;
}
