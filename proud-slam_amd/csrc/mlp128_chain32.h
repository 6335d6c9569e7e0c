// The width-128 decoder's forward chain (mlp_fwd.hip: k_mlp_fwd2, k_mlp_sdf2;
// k_mlp_prep builds its operand images): v_mfma_f32_32x32x2_f32 on 32-sample
// tiles, every activation in accumulator form (mlp128.h's head comment), the
// weights read from LDS in a layout permuted to match.
#pragma once
#include "mlp128.h"

namespace psvo {
namespace {

constexpr int kImgFwd = 128 * 144;                    // largest forward image (W4)

// Position of M[i][k] (product row i, reduction index k fed from
// accumulator blocks) in the A-operand image [ib][kb][rg][lane][4].
__device__ __forceinline__ int perm_acc(int i, int k, int nkb) {
    const int ib = i >> 5, ii = i & 31;
    const int kb = k >> 5, kk = k & 31;
    const int r = (kk & 3) | ((kk >> 3) << 2);
    const int h = (kk >> 2) & 1;
    const int lane = ii + 32 * h;
    return ((((ib * nkb + kb) * 4 + (r >> 2)) * 64 + lane) << 2) + (r & 3);
}
// Same for a 16-wide reduction fed from the x registers: k-step t takes
// k = 2t + h, 8 steps grouped by 4: [ib][tg][lane][4].
__device__ __forceinline__ int perm_x(int i, int k) {
    const int ib = i >> 5, ii = i & 31;
    const int t = k >> 1, h = k & 1;
    const int lane = ii + 32 * h;
    return (((ib * 2 + (t >> 2)) * 64 + lane) << 2) + (t & 3);
}

// acc[ob] += image(`wl`: NOUT x NIN blocks) · in[kb].  Software-pipelined:
// the NOUT operand groups of step (kb, rg) + 1 are read from LDS before the
// 4·NOUT MFMAs of step (kb, rg) issue (ob innermost, independent
// accumulators), and scheduling barriers per step keep the compiler from
// pulling those reads back next to their first use — so the LDS latency
// hides behind a step of MFMAs instead of stalling every 4 of them.  `st`
// (St::kN stores per step) drains a pending store queue between the reads
// and the MFMAs of each step — spread over the GEMM instead of a burst that
// fills the TA command FIFO and stalls the wave.
struct NoStore {
    static constexpr int kN = 0;
    __device__ __forceinline__ void operator()(int, int) const {}
};

template <int NIN, int NOUT, typename St = NoStore>
__device__ __forceinline__ void gemm_acc(const float *wl, const f32x16 (&in)[NIN], f32x16 (&acc)[NOUT], int lane,
                                         const St &st = St()) {
    constexpr int kSteps = NIN * 4;
    auto opnd = [&](int step, int ob) {
        const int kb = step >> 2, rg = step & 3;
        return *reinterpret_cast<const float4 *>(wl + ((((ob * NIN + kb) * 4 + rg) * 64 + lane) << 2));
    };
    float4 cur[NOUT];
#pragma unroll
    for (int ob = 0; ob < NOUT; ++ob) cur[ob] = opnd(0, ob);
#pragma unroll
    for (int step = 0; step < kSteps; ++step) {
        const int kb = step >> 2, rg = step & 3;
        float4 nxt[NOUT];
        if (step + 1 < kSteps) {
#pragma unroll
            for (int ob = 0; ob < NOUT; ++ob) nxt[ob] = opnd(step + 1, ob);
        }
        st(kb, rg);
#pragma unroll
        for (int ob = 0; ob < NOUT; ++ob) acc[ob] = mfma(cur[ob].x, in[kb][4 * rg + 0], acc[ob]);
#pragma unroll
        for (int ob = 0; ob < NOUT; ++ob) acc[ob] = mfma(cur[ob].y, in[kb][4 * rg + 1], acc[ob]);
#pragma unroll
        for (int ob = 0; ob < NOUT; ++ob) acc[ob] = mfma(cur[ob].z, in[kb][4 * rg + 2], acc[ob]);
#pragma unroll
        for (int ob = 0; ob < NOUT; ++ob) acc[ob] = mfma(cur[ob].w, in[kb][4 * rg + 3], acc[ob]);
        if (step + 1 < kSteps) __builtin_amdgcn_sched_group_barrier(0x100, NOUT, 0);  // the next step's reads
        if (St::kN > 0) __builtin_amdgcn_sched_group_barrier(0x040, St::kN, 0);      // queued stores
        __builtin_amdgcn_sched_group_barrier(0x008, 4 * NOUT, 0);                     // this step's MFMAs
        __builtin_amdgcn_sched_barrier(0);
        if (step + 1 < kSteps) {
#pragma unroll
            for (int ob = 0; ob < NOUT; ++ob) cur[ob] = nxt[ob];
        }
    }
}

// acc[ob] += image(perm_x) · x  (x[t] = x feature 2t + h).  `st` (a store
// queue of 16 slots, e.g. CfQueue: one 16-KB CF tile) drains 2 slots per k
// sub-step, between that sub-step's 4 MFMAs.
template <typename St = NoStore>
__device__ __forceinline__ void gemm_x(const float *wl, const float (&x)[8], f32x16 (&acc)[kNB], int lane,
                                       const St &st = St()) {
#pragma unroll
    for (int tg = 0; tg < 2; ++tg) {
        float4 a[kNB];
#pragma unroll
        for (int ob = 0; ob < kNB; ++ob) a[ob] = *reinterpret_cast<const float4 *>(wl + (((ob * 2 + tg) * 64 + lane) << 2));
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (St::kN > 0) {
                const int q = 2 * (4 * tg + c);
                st(q >> 2, q & 3);
                st((q + 1) >> 2, (q + 1) & 3);
            }
#pragma unroll
            for (int ob = 0; ob < kNB; ++ob) acc[ob] = mfma(a[ob][c], x[4 * tg + c], acc[ob]);
            if (St::kN > 0) {
                __builtin_amdgcn_sched_group_barrier(0x040, 2 * St::kN, 0);  // the queued stores
                __builtin_amdgcn_sched_group_barrier(0x008, kNB, 0);         // then this sub-step's MFMAs
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
}

__device__ __forceinline__ void init_bias(f32x16 (&acc)[kNB], const float *b, int h) {
#pragma unroll
    for (int ob = 0; ob < kNB; ++ob)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[ob][r] = b[32 * ob + phi(r, h)];
}

// max(v, 0) in one instruction.  fmaxf() on an accumulator element costs two:
// the compiler does not know an MFMA result to be canonical and quiets it
// first (v_max v, v, v).  v_med3_f32(v, 0, +inf) needs no such step and gives
// fmaxf's bits for every input the chain can produce: MAX(v, 0) by the same
// comparator when nothing is a NaN (−0 → +0, denormals kept), MIN3 = 0 for a
// quiet NaN.  `inf` is opaque_inf(): with the literal the compiler folds the
// median back into canonicalise + max.
__device__ __forceinline__ float opaque_inf() {
    float inf = __builtin_inff();
    asm("" : "+s"(inf));
    return inf;
}
__device__ __forceinline__ float relu1(float v, float inf) { return __builtin_amdgcn_fmed3f(v, 0.0f, inf); }

// One element's ReLU mask bit, shifted into `acc` from below: a signed integer
// compare of y = max(v, 0) against 0 (true exactly for the positive non-zero
// patterns, denormals included; ±0 false) into VCC, then acc = 2·acc + carry.
// Both in one statement, so no compare result stays live in an SGPR pair (the
// compare form written in C++ spilled ~300 SGPRs), and the statement pins the
// element in program order: the scheduler would otherwise hoist all 64 element
// computations and keep them live at once.  y is the compiler's own v_max
// result, a VALU write: no MFMA read hazard inside the statement.  The k-th
// element shifted in ends at bit 31 − k after 32 of them: mask_word() turns
// the word round.
__device__ __forceinline__ void mask_shift_in(uint32_t &acc, float &y) {
    asm volatile("v_cmp_lt_i32 vcc, 0, %1\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(acc), "+v"(y) : : "vcc");
}
__device__ __forceinline__ uint32_t mask_word(uint32_t acc) { return __builtin_bitreverse32(acc); }

// ReLU in place; returns the (value > 0) mask, bit 16b + r: per element the
// max and mask_shift_in's two instructions.
__device__ __forceinline__ uint64_t relu(f32x16 (&v)[kNB]) {
    uint32_t half[2] = {0u, 0u};
    const float inf = opaque_inf();
#pragma unroll
    for (int b = 0; b < kNB; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float y = relu1(v[b][r], inf);
            mask_shift_in(half[b >> 1], y);  // element 16 (b & 1) + r of its word, in this order
            v[b][r] = y;
        }
    return (uint64_t)mask_word(half[0]) | ((uint64_t)mask_word(half[1]) << 32);
}

// ReLU in place, values only (k_mlp_sdf2, the inference forwards: nobody reads
// a mask): relu()'s values, bit for bit, one max per element.  Pinned in
// program order like relu()'s elements.
__device__ __forceinline__ void relu_values(f32x16 (&v)[kNB]) {
    const float inf = opaque_inf();
#pragma unroll
    for (int b = 0; b < kNB; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float y = relu1(v[b][r], inf);
            asm volatile("" : "+v"(y));
            v[b][r] = y;
        }
}

// Σ_k w[k] · v[k][sample] over this lane's 64 features (other half via partner lane)
// (roundings spelled out — an fmaf chain and one add — so every kernel that
// uses it, e.g. the sdf-only and the training forward, gives the same bits
// whatever the compiler would contract around it)
__device__ __forceinline__ float row_dot(const float *w, const f32x16 (&v)[kNB], int h) {
    float s = 0.f;
#pragma unroll
    for (int b = 0; b < kNB; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) s = fmaf(w[32 * b + phi(r, h)], v[b][r], s);
    return __fadd_rn(s, __shfl_xor(s, 32, 64));
}

// Store an activation held in accumulator form as rows of a row-major
// [M][ld] matrix (sample s = lane's column): 16-B stores.
__device__ __forceinline__ void store_rows(float *dst, int64_t s, bool valid, int ld, const f32x16 (&v)[kNB], int h) {
    if (!valid) return;
    float *row = dst + s * ld;
#pragma unroll
    for (int b = 0; b < kNB; ++b)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg)
            *reinterpret_cast<float4 *>(row + 32 * b + 8 * rg + 4 * h) =
                make_float4(v[b][4 * rg], v[b][4 * rg + 1], v[b][4 * rg + 2], v[b][4 * rg + 3]);
}

// store_rows' inverse: row `row` of a row-major [·][128] matrix into
// accumulator form (zeros when !valid)
__device__ __forceinline__ void load_rows(const float *__restrict__ src, int64_t row, bool valid, f32x16 (&v)[kNB],
                                          int h) {
    const float *p = src + (valid ? row : 0) * kW;
#pragma unroll
    for (int b = 0; b < kNB; ++b)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
            float4 q = *reinterpret_cast<const float4 *>(p + 32 * b + 8 * rg + 4 * h);
            if (!valid) q = make_float4(0.f, 0.f, 0.f, 0.f);
            v[b][4 * rg] = q.x;
            v[b][4 * rg + 1] = q.y;
            v[b][4 * rg + 2] = q.z;
            v[b][4 * rg + 3] = q.w;
        }
}

// ---- k_mlp_fwd2's W4 layer, one 32-row output block at a time ----------
// Block OB's MFMAs carry the CF stores of f (its block OB, the layer input)
// and of c1 block OB-1 (finished, ReLU'd) — one store each per k-step — so
// the c1 tile no longer leaves in one 64-store burst that, issued by every
// wave of the chip at once, stalled the epilogue on HBM write drain; block
// OB's ReLU and mask bits run under block OB+1's MFMAs.  Per accumulator the
// MFMA order is unchanged: the same bits.
template <int OB>
struct L4Queue {
    static constexpr int kN = OB > 0 ? 2 : 1;
    const CfStore &c;
    const f32x16 (&f)[kNB];
    const f32x16 (&c1)[kNB];
    __amdgpu_buffer_rsrc_t rf, rc;
    __device__ L4Queue(const CfStore &cs, const float *fm, const float *cm, int64_t bytes, bool on,
                       const f32x16 (&ff)[kNB], const f32x16 (&cc)[kNB])
        : c(cs), f(ff), c1(cc),
          rf(__builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(fm), 0,
                                               __builtin_amdgcn_readfirstlane((on && cs.ok) ? (int)bytes : 0),
                                               0x00020000)),
          rc(__builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(cm), 0,
                                               __builtin_amdgcn_readfirstlane((on && cs.ok) ? (int)bytes : 0),
                                               0x00020000)) {}
    __device__ __forceinline__ void operator()(int kb, int rg) const {
        const int r = 4 * kb + rg;
        const int vo = c.voff[((r >> 1) & 1) + 2 * ((r >> 2) & 1)];
        const int so = 1024 * (r >> 2) + 128 * (r & 3);
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(f[OB][r]), rf, vo, 4096 * OB + so, 0);
        if (OB > 0)
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(c1[OB - 1][r]), rc, vo, 4096 * (OB - 1) + so, 0);
    }
};

// relu() restricted to block OB (same per-element sequence): `half` collects
// the blocks' bits as relu()'s words do, blocks in order 0..3, and is turned
// round by mask_word() after the last one.  MASK false: relu_values()'s.
template <int OB, bool MASK>
__device__ __forceinline__ void relu_block(f32x16 &v, uint32_t (&half)[2]) {
    const float inf = opaque_inf();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float y = relu1(v[r], inf);
        if constexpr (MASK)
            mask_shift_in(half[OB >> 1], y);
        else
            asm volatile("" : "+v"(y));
        v[r] = y;
    }
}

// bacc[OB] += W4 block OB · [f; x] (bias already in bacc), then its ReLU and
// mask bits (the rgb head's dots wait for all four blocks: until then f is
// live as the layer input and the registers are spoken for)
template <int OB, bool MASK>
__device__ __forceinline__ void l4_block(const float *wl, const f32x16 (&a)[kNB], const float (&x)[8],
                                         f32x16 (&bacc)[kNB], int lane, const L4Queue<OB> &q,
                                         uint32_t (&half)[2]) {
    f32x16 (&acc)[1] = *reinterpret_cast<f32x16(*)[1]>(&bacc[OB]);
    gemm_acc<kNB, 1>(wl + OB * kNB * 4 * 64 * 4, a, acc, lane, q);
    const float *wx = wl + kNB * kNB * 16 * 64;
#pragma unroll
    for (int tg = 0; tg < 2; ++tg) {
        const float4 w4 = *reinterpret_cast<const float4 *>(wx + (((OB * 2 + tg) * 64 + lane) << 2));
        acc[0] = mfma(w4.x, x[4 * tg + 0], acc[0]);
        acc[0] = mfma(w4.y, x[4 * tg + 1], acc[0]);
        acc[0] = mfma(w4.z, x[4 * tg + 2], acc[0]);
        acc[0] = mfma(w4.w, x[4 * tg + 3], acc[0]);
    }
    relu_block<OB, MASK>(bacc[OB], half);
}

// LDS of the persistent forward kernels: the vectors and W1 resident, then
// two buffers the later layers' images stream through
constexpr int kF2Tile = kF2Waves * 32;  // samples per workgroup iteration
constexpr int kF2W1 = kVecPad, kF2Buf0 = kF2W1 + 2048, kF2Buf1 = kF2Buf0 + kImgFwd;
constexpr int kLdsFwd2 = (kF2Buf1 + kImgFwd) * 4;  // 160,768 B
static_assert(kLdsFwd2 <= 160 * 1024, "fwd2 LDS budget");
constexpr int kLdsSdf2 = (kF2Buf0 + 16384) * 4;    // k_mlp_sdf2: W1 and W2 resident (77 KB)

}  // namespace
}  // namespace psvo
