// NRGBD decoder (src/variations/nrgbd.py:80-146, depth 2, width 128, input
// 16, embedder 'none', skips [] — every shipped Replica config) as fused
// fp32-MFMA kernels for gfx950: what every width-128 kernel shares.
//
//   h1 = relu(W1 x + b1)           W1 [128,16]
//   h2 = relu(W2 h1 + b2)          W2 [128,128]
//   o  = W3 h2 + b3 = [sdf | f]    W3 [129,128]
//   c1 = relu(W4 [f; x] + b4)      W4 [128,144]
//   rgb = sigmoid(W5 c1 + b5)      W5 [3,128]
//
// Two operand layouts, one file of helpers each:
//
// mlp128_chain32.h — the forward ("transposed" chain, mlp_fwd.hip): a wave
// owns 32 samples and keeps every activation as feature-rows x sample-columns
// in v_mfma_f32_32x32x2_f32 accumulator form — lane l holds sample l&31,
// register r of block b holds feature 32b + phi(r, l>>5), phi(r,h) = (r&3) +
// 8(r>>2) + 4h.  The next layer consumes that register directly as its B
// operand (k-pair {phi(r,0), phi(r,1)}), so the chain needs no LDS round trip
// and no shuffles; the A operand (weights) is read from LDS in a layout
// permuted to match (one ds_read_b128 feeds 4 MFMAs).  Each layer's weights
// are staged into LDS (≤ 73.7 KB) by straight copies of k_mlp_prep's images.
//
// mlp128_chain16.h — the backward chains (mlp_bwd.hip, mlp128_trunk_fb.h):
// v_mfma_f32_16x16x4_f32 on 16-sample units, lane (n, q) holding features
// 16·ob + 4q + j of sample n (j = register): half the registers of the
// 32-sample form, which leaves room for the weight-gradient accumulators
// (those stay 32x32x2 MFMAs: phi / mfma below).
//
// fp32 in, fp32 accumulate (exact fmaf chains, no TF32-like rounding): the
// numerics class of the reference.  The host side of each kernel family sits
// under its kernels; decoder.cpp picks the width.
#pragma once
#include <hip/hip_runtime.h>

#include "psvo_common.h"

#ifdef PSVO_STAMPS
__device__ unsigned long long psvo_g_stamps[3][256][8][8][16];  // diagnostic build only
#endif

namespace psvo {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kW = 128;     // decoder width
constexpr int kIn = 16;     // embedding dim
constexpr int kNB = kW / 32;

// LDS carve (floats): small vectors first, then the staged weight image.
constexpr int kOffB1 = 0, kOffB2 = kOffB1 + 128, kOffB3 = kOffB2 + 128, kOffB4 = kOffB3 + 132,
              kOffB5 = kOffB4 + 128;                  // biases b1 b2 b3[129] b4 b5[3]
constexpr int kOffW3r0 = kOffB5 + 4, kOffW5 = kOffW3r0 + 128;  // W3 row 0 (sdf), W5 [3][128]
constexpr int kOffW = kOffW5 + 3 * 128;               // = 1032 floats (16-B aligned)

// every kernel below k_mlp_prep runs 8-wave workgroups, one per CU
constexpr int kF2Waves = 8, kF2Threads = kF2Waves * 64;

__device__ __forceinline__ int phi(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

template <int N>
__device__ __forceinline__ void zero(f32x16 (&acc)[N]) {
#pragma unroll
    for (int b = 0; b < N; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[b][r] = 0.0f;
}

// Activations and δ's the weight gradients consume are stored TILE-FEATURE
// major ("CF"): per 32-sample tile a [128 feature][32 slot] block (16 KB) in
// which tile-local sample c sits at position p = (c&1)·16 + c/2 (the two
// samples of one f32 MFMA k-step pair, 2t and 2t+1, at t and 16 + t) and the
// 8 16-B groups of a row are XOR-swizzled by feature (slot = g ^ (f/2)%8: any
// 16 consecutive rows then cover all 64 banks once per 16-B column).  That
// is exactly the weight-gradient MFMAs' operand image (conflict-free
// 4-k-step ds_read_b128).  The producing wave writes its 32-sample tile
// register by register with buffer stores: each covers two 64-B runs of two
// feature rows.
constexpr int kCh = 64;                 // allocation granule: CF buffers hold whole 64-sample pairs of tiles
constexpr int kTileS = 32;              // samples per CF tile
constexpr int kCfTile = 128 * kTileS;   // floats per CF tile
constexpr int64_t kMaxSamples = (int64_t)131071 * kTileS;  // one CF matrix < 2 GiB (buffer offsets)

// Element (b, r) of a wave's accumulator tile lands at byte
//   tile·16384 + f·128 + 4·((((p>>2) ^ X) << 2) | (p&3)),  f = 32b + phi(r, h)
// with X = (f/2)%8 = 4((r>>2)&1) + 2h + ((r>>1)&1): per lane 4 XOR variants
// voff[((r>>1)&1) + 2((r>>2)&1)] (tile and 512h folded in) and a
// wave-uniform rest 4096b + 1024(r>>2) + 128(r&3) (soffset).
struct CfStore {
    int voff[4];
    bool ok;
    __device__ CfStore(int64_t tile, int lane, int64_t n_tiles) {
        ok = tile < n_tiles;
        const int c = lane & 31;
        const int p = (c & 1) * 16 + (c >> 1);
        const int hh = lane >> 5;
        const int base = (int)(tile * kCfTile * 4) + 512 * hh;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int xr = 4 * (v >> 1) + 2 * hh + (v & 1);
            voff[v] = base + 4 * ((((p >> 2) ^ xr) << 2) | (p & 3));
        }
    }
    __device__ __forceinline__ void store(const float *matrix, int64_t bytes, const f32x16 (&v)[kNB]) const {
        if (!ok) return;
        const __amdgpu_buffer_rsrc_t rs =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(matrix), 0, (int)bytes, 0x00020000);
#pragma unroll
        for (int b = 0; b < kNB; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[b][r]), rs, voff[((r >> 1) & 1) + 2 * ((r >> 2) & 1)],
                                                      4096 * b + 1024 * (r >> 2) + 128 * (r & 3), 0);
    }
};

// Pending-store queue for gemm_acc: the tile `v` (the GEMM's input) into a CF
// matrix, 4 registers per GEMM step.  A disabled queue (or a tile past the
// allocation) gets an empty buffer range, so the hardware drops its stores
// without a branch in the MFMA stream.
struct CfQueue {
    static constexpr int kN = 4;
    const CfStore &c;
    const f32x16 (&v)[kNB];
    __amdgpu_buffer_rsrc_t rs;
    __device__ CfQueue(const CfStore &cs, const float *matrix, int64_t bytes, bool on, const f32x16 (&vv)[kNB])
        : c(cs), v(vv),
          rs(__builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(matrix), 0,
                                               __builtin_amdgcn_readfirstlane((on && cs.ok) ? (int)bytes : 0),
                                               0x00020000)) {}
    __device__ __forceinline__ void operator()(int kb, int rg) const {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = 4 * rg + j;
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[kb][r]), rs, c.voff[((r >> 1) & 1) + 2 * ((r >> 2) & 1)],
                                                  4096 * kb + 1024 * (r >> 2) + 128 * (r & 3), 0);
        }
    }
};

// ---------------------------------------------------------------------------
// Weight images: every layer's LDS operand image, laid out exactly as the
// kernels read it, built once per weight update by k_mlp_prep (a gather,
// coalesced writes) so that staging is a straight 16-B copy.
//   fwd: W1 (perm_x), W2, W3 rows 1..128 (perm_acc), W4 ([f | x])
//   bwd (k_mlp_bwd3's chain): W4ᵀ, W3[1:]ᵀ, W2ᵀ, W1ᵀ as 16 × 16 blocks
constexpr int kImgF1 = 0, kImgF2 = kImgF1 + 2048, kImgF3 = kImgF2 + 16384, kImgF4 = kImgF3 + 16384,
              kImgVec = kImgF4 + 18432,   // the small vectors in their LDS layout (kOffB1..kOffW), padded
              kVecPad = 1280,             // to whole 1-KB glds pieces
              // k_mlp_bwd3's chain (v_mfma_f32_16x16x4_f32, 16-sample units): Wᵀ as 16 × 16
              // blocks (ob, kb), lane (m, q) holding Wᵀ[16ob + m][16kb + 4q .. 4q + 3]
              kImgC4 = kImgVec + kVecPad,   // W4ᵀ: 9 × 8 blocks (144 rows: f and x)
              kImgC3 = kImgC4 + 9 * 8 * 256,  // W3[1:]ᵀ
              kImgC2 = kImgC3 + 8 * 8 * 256,  // W2ᵀ
              kImgC1 = kImgC2 + 8 * 8 * 256,  // W1ᵀ: 1 × 8 blocks
              // the trunk kernel's forward in the same chain layout (W, not Wᵀ):
              // lane (m, q) holding W[16ob + m][16kb + 4q .. 4q + 3]
              kImgT1 = kImgC1 + 8 * 256,    // W1: 8 × 1 blocks
              kImgT2 = kImgT1 + 8 * 256,    // W2: 8 × 8 blocks
              kImgTotal = kImgT2 + 8 * 8 * 256;  // 126,208 floats
static_assert(kOffW <= kVecPad, "vector image");

// Barrier for LDS hazards only: waits for this wave's LDS operations, not for
// its global stores (__syncthreads' fence would also drain every outstanding
// activation store and glds before each layer).
__device__ __forceinline__ void raw_barrier() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): this wave's LDS ops done (vmcnt left as is)
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ void load_x(const float *__restrict__ feat, int64_t s, bool valid, int h, float (&x)[8]) {
    const float *fr = feat + (valid ? s : 0) * kIn;
#pragma unroll
    for (int t = 0; t < 8; ++t) x[t] = valid ? fr[2 * t + h] : 0.0f;
}

// global → LDS copies (global_load_lds_*): LDS destination = wave-uniform
// base (M0) + lane × size.  Issued through inline asm so that the compiler's
// wait insertion does not treat them as LDS writes aliasing every ds_read
// (it would drain the prefetch with vmcnt(0) before each operand read); the
// kernel counts them itself (wait_vm).
__device__ __forceinline__ uint32_t lds_addr(const float *l) {
    return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) float *)l;
}
__device__ __forceinline__ void glds16(const float *g, float *l) {
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(g), "s"(__builtin_amdgcn_readfirstlane(lds_addr(l)))
                 : "memory");
}

// an image of n_floats (whole 1-KB pieces) into LDS, by the workgroup's 8 waves
__device__ __forceinline__ void stage8(float *dst, const float *img, int n_floats, int wave, int lane) {
    for (int c = wave; c < n_floats / 256; c += kF2Waves) glds16(img + (c * 64 + lane) * 4, dst + c * 256);
}

// streaming (nt) store of one float at base[i]: the slabs are read once, by
// the reduce kernel (a kernel boundary also pays ≈ dirty bytes ÷ 6 TB/s for
// what stays dirty in L2; measured: nt slab stores 0.99 -> 0.985 ms per BA
// iteration, write-through (sc1) ones no gain)
__device__ __forceinline__ void store_nt(float *base, int i, float v) { __builtin_nontemporal_store(v, base + i); }

// s_waitcnt vmcnt(n) for this wave's global_load_lds copies (the kernels count them)
__device__ __forceinline__ void wait_vm(int n) {
    // s_waitcnt vmcnt(n) only (expcnt / lgkmcnt at their maxima); n <= 63
    asm volatile("" ::: "memory");
    switch (n) {
        case 0: __builtin_amdgcn_s_waitcnt(0x0F70); break;
        case 1: __builtin_amdgcn_s_waitcnt(0x0F71); break;
        case 8: __builtin_amdgcn_s_waitcnt(0x0F78); break;
        case 9: __builtin_amdgcn_s_waitcnt(0x0F79); break;
        case 16: __builtin_amdgcn_s_waitcnt(0x4F70); break;
        case 17: __builtin_amdgcn_s_waitcnt(0x4F71); break;
        case 18: __builtin_amdgcn_s_waitcnt(0x4F72); break;
        default: __builtin_amdgcn_s_waitcnt(0x0F70); break;  // conservative: everything
    }
    asm volatile("" ::: "memory");
}

// The weight gradients' slabs: k_mlp_bwd3 and k_mlp_trunk_fb write one slab of
// every layer per workgroup, k_mlp_dw_reduce sums them.  Matrix l = 0..4: W1
// .. W5, each followed by its bias.  (Both structs are kernel arguments: their
// layout fixes the kernarg offsets.)
struct DwGrid {
    int wg_begin[5];  // not read (a per-layer workgroup split no kernel uses any more)
    int n_split[5];   // slabs per weight matrix (W5 has W1's)
    int slab_off[5];  // float offset of matrix l's first slab
    int slab_len[5];  // rows*cols + rows
};

struct DwDst {
    float *w[5], *b[5];
    int rows[5], cols[5];
    int elem_begin[6];
};

// Diagnostic build only (-DPSVO_STAMPS, `make stamps`: lib/diag/): per-wave
// s_memtime stamps at the layer boundaries of k_mlp_fwd2 (kStampK 0),
// k_mlp_bwd3 (1) and k_mlp_trunk_fb (2), read through psvo_debug_stamps.  In
// the product library every PSVO_STAMP is empty.
#ifdef PSVO_STAMPS
constexpr int kStampIters = 8, kStampWgs = 256;  // psvo_g_stamps[3][256][8][8][16]
#define PSVO_STAMP_DECL int stit_ = 0
#define PSVO_STAMP(i)                                                                               \
    do {                                                                                            \
        __builtin_amdgcn_sched_barrier(0);                                                          \
        const unsigned long long t_ = __builtin_amdgcn_s_memtime();                                 \
        __builtin_amdgcn_sched_barrier(0);                                                          \
        if ((threadIdx.x & 63) == 0 && stit_ < kStampIters && blockIdx.x < kStampWgs)               \
            psvo_g_stamps[kStampK][blockIdx.x][threadIdx.x >> 6][stit_][i] = t_;                         \
    } while (0)
#define PSVO_STAMP_FLUSH(k) ++stit_
#else
#define PSVO_STAMP_DECL
#define PSVO_STAMP(i)
#define PSVO_STAMP_FLUSH(k)
#endif

}  // namespace
}  // namespace psvo
