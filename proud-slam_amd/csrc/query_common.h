// Device-side helpers of the ray-query units (query_trace.hip,
// query_sample.hip, query_dist.hip) that more than one of them uses: the
// wave-level reductions and LDS hand-off, the single-workgroup scan and the
// diagnostic stamp macros.  Everything here is inlined or a template over
// its caller's lambda: no unit shares a compiled body with another.
#pragma once

#include <hip/hip_runtime.h>

#include "psvo_common.h"

namespace psvo {
namespace {

__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v = max(v, __shfl_xor(v, s, kWave));
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, kWave);
    return v;
}

// ---------------------------------------------------------------------------
// The slab test and the level bound of every octree walk (query_trace.hip's
// traversals, covis.hip's visibility walk): one copy, so all of them compare
// the same values.  Contraction is off inside the bodies whatever the
// including unit sets (hit indices reproduce the CPU oracle bit for bit).
constexpr int kLevels = 16;  // octree depth <= 15 (grid_dim <= 32768)

__device__ __forceinline__ bool ray_aabb(const float o[3], const float inv[3], float cx, float cy, float cz,
                                         float half, float &t_lo, float &t_hi) {
#pragma clang fp contract(off)
    float lo_all = 0.0f, hi_all = 100000.0f;
    const float c[3] = {cx, cy, cz};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float lo = (c[a] - half - o[a]) * inv[a];
        float hi = (c[a] + half - o[a]) * inv[a];
        if (hi < lo) {
            const float tmp = lo;
            lo = hi;
            hi = tmp;
        }
        if (hi < lo_all) return false;
        if (lo > hi_all) return false;
        lo_all = (lo > lo_all) ? lo : lo_all;
        hi_all = (hi < hi_all) ? hi : hi_all;
        if (lo_all > hi_all) return false;
    }
    t_lo = lo_all;
    t_hi = hi_all;
    return true;
}

// ray_aabb without the early exits: the same comparisons on the same values
// in the same order (NaNs included), the verdict accumulated instead of
// returned.  The traversal's node record is then consumed in one basic block,
// so the compiler cannot sink the y / z loads behind the x test (a second
// dependent memory round trip per round); t_lo / t_hi are set only on a hit.
__device__ __forceinline__ bool ray_aabb_nb(const float o[3], const float inv[3], float cx, float cy, float cz,
                                            float half, float &t_lo, float &t_hi) {
#pragma clang fp contract(off)
    float lo_all = 0.0f, hi_all = 100000.0f;
    bool miss = false;
    const float c[3] = {cx, cy, cz};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float lo = (c[a] - half - o[a]) * inv[a];
        float hi = (c[a] + half - o[a]) * inv[a];
        const bool sw = hi < lo;
        const float l2 = sw ? hi : lo, h2 = sw ? lo : hi;
        miss = miss | (h2 < lo_all) | (l2 > hi_all);
        lo_all = (l2 > lo_all) ? l2 : lo_all;
        hi_all = (h2 < hi_all) ? h2 : hi_all;
        miss = miss | (lo_all > hi_all);
    }
    if (!miss) {
        t_lo = lo_all;
        t_hi = hi_all;
    }
    return !miss;
}

// Diagnostic build only (-DPSVO_IS_STAMPS, `make is_stamps`: lib/diag/): per
// ray, k_intersect_sorted's cycles by segment (s_memtime; scalar reads of the
// clock only), read through psvo_debug_is_stamps (scripts/intersect_stamps.py).
// Segments: [0] whole ray, [1] pop + node load + AABB test, [2] scan +
// re-queue + child push, [3] leaf merge, [4] final sort + output, [5] rounds,
// [6] rounds that found leaves, [7] AABB tests.  The product build has none.
// k_sample_fused per workgroup (s_memrealtime, 100 MHz — one clock for all
// CUs): [0] entry, [1] its rays sampled (wave 0), [2] the row stores drained
// + barrier, [3] the look-back's prefix known (wave 0), [4] compaction done
// (psvo_debug_smp_stamps, scripts/sampler_stamps.py).  Each stamp array is
// defined in the unit that writes it: psvo_g_is_stamps in query_trace.hip,
// psvo_g_smp_stamps in query_sample.hip.
#ifdef PSVO_IS_STAMPS
#define IS_T(v)                                                                   \
    do {                                                                          \
        __builtin_amdgcn_sched_barrier(0);                                        \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v)::"memory"); \
        __builtin_amdgcn_sched_barrier(0);                                        \
    } while (0)
#define IS_DECL unsigned long long is_t0 = 0, is_ta = 0, is_tb = 0, is_acc[5] = {0, 0, 0, 0, 0}, is_lr = 0
#define IS_MARK(var) IS_T(var)
#define IS_ADD(k, from, to) is_acc[k] += (to) - (from)
#define SMP_T(k)                                                                          \
    do {                                                                                  \
        __builtin_amdgcn_sched_barrier(0);                                                \
        const unsigned long long t_ = __builtin_amdgcn_s_memrealtime();                   \
        if ((threadIdx.x & 63) == 0 && w == 0) psvo_g_smp_stamps[blockIdx.x & 4095][k] = t_; \
        __builtin_amdgcn_sched_barrier(0);                                                \
    } while (0)
#define SMP_T0(k)                                                                         \
    do {                                                                                  \
        __builtin_amdgcn_sched_barrier(0);                                                \
        const unsigned long long t_ = __builtin_amdgcn_s_memrealtime();                   \
        if (threadIdx.x == 0) psvo_g_smp_stamps[blockIdx.x & 4095][k] = t_;               \
        __builtin_amdgcn_sched_barrier(0);                                                \
    } while (0)
#else
#define IS_DECL
#define IS_MARK(var)
#define IS_ADD(k, from, to)
#define SMP_T(k)
#define SMP_T0(k)
#endif

// ---------------------------------------------------------------------------
// Single-workgroup exclusive scan (n ≲ 10^6): each thread owns a contiguous
// run; run totals scanned in LDS.
// Runs of up to kRegRun elements (n ≤ 8·1024 with 1024 threads) are read
// once, in one round of independent loads, and kept in registers (the
// general loop re-reads them after the barriers); `lmax`, if set, receives
// the thread's largest value.
constexpr int kRegRun = 8;

template <typename F>
__device__ void block_scan_runs(int64_t n, F value, int *__restrict__ out, int *total, int *lmax = nullptr) {
    // thread t scans the run [t·per, (t+1)·per); the run totals are scanned
    // with wave shuffles and one LDS pass over the ≤ 16 wave totals
    // (2 barriers instead of a 2·log2(1024)-barrier Hillis–Steele pass)
    __shared__ int s_wave[16];
    const int tid = threadIdx.x;
    const int nt = blockDim.x;
    const int lane = tid & (kWave - 1), w = tid / kWave, nw = nt / kWave;
    const int64_t per = (n + nt - 1) / nt;
    const int64_t beg = tid * per;
    const int64_t end = beg + per < n ? beg + per : n;
    const bool in_regs = per <= kRegRun;  // block-uniform
    int vals[kRegRun];
    int local = 0, mx = 0;
    if (in_regs) {
#pragma unroll
        for (int k = 0; k < kRegRun; ++k) vals[k] = beg + k < end ? value(beg + k) : 0;
#pragma unroll
        for (int k = 0; k < kRegRun; ++k) {
            local += vals[k];
            mx = max(mx, vals[k]);
        }
    } else {
        for (int64_t i = beg; i < end; ++i) {
            const int v = value(i);
            local += v;
            mx = max(mx, v);
        }
    }
    if (lmax) *lmax = mx;
    int incl = local;
#pragma unroll
    for (int sh = 1; sh < kWave; sh <<= 1) {
        const int t = __shfl_up(incl, sh, kWave);
        if (lane >= sh) incl += t;
    }
    if (lane == kWave - 1) s_wave[w] = incl;
    __syncthreads();
    if (w == 0) {
        int v = lane < nw ? s_wave[lane] : 0;
#pragma unroll
        for (int sh = 1; sh < 16; sh <<= 1) {
            const int t = __shfl_up(v, sh, kWave);
            if (lane >= sh) v += t;
        }
        if (lane < nw) s_wave[lane] = v;  // inclusive wave prefix
    }
    __syncthreads();
    int run = (w > 0 ? s_wave[w - 1] : 0) + incl - local;
    if (in_regs) {
#pragma unroll
        for (int k = 0; k < kRegRun; ++k)
            if (beg + k < end) {
                out[beg + k] = run;
                run += vals[k];
            }
    } else {
        for (int64_t i = beg; i < end; ++i) {
            out[i] = run;
            run += value(i);
        }
    }
    if (tid == nt - 1) *total = s_wave[nw - 1];
}

}  // namespace
}  // namespace psvo
