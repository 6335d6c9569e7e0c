// The width-128 decoder's backward chains, shared by k_mlp_bwd3 (mlp_bwd.hip)
// and k_mlp_trunk_fb (mlp128_trunk_fb.h): a chain wave runs
// v_mfma_f32_16x16x4_f32 on a 16-sample unit, its weights streaming from L2
// as MFMA A operands (mlp128.h's kImgC* / kImgT* images); a gradient wave
// accumulates Σ_s δ[o][s] a[i][s] with 32x32x2 MFMAs, the δ's handed over
// through LDS as unit images.
#pragma once
#include "mlp128.h"

namespace psvo {
namespace {

// LDS image of a unit's δ (and of its x): 128 (16) rows × 16 slots, sample
// n at slot 8(n&1) + n/2 (k-step t of the 32x32x2 gradient MFMA takes
// samples 2t, 2t+1 — the CF tile's order), the four 16-B chunks of row r
// XOR-permuted by (r >> 2) & 3: the chain's ds_write_b32 (4 rows × 16
// slots) are at most 2-way, the gradient waves' ds_read_b128 (32 rows ×
// one chunk) conflict-free.
constexpr int kU = 16;                                  // samples per chain unit
constexpr int kUImg = 128 * kU;                         // a unit's δ image (8 KB)
// k_mlp_bwd3's LDS carve (floats), after the vectors
constexpr int kB3Slot = kVecPad;                        // δ images [set 2][unit 4]
constexpr int kB3Small = kB3Slot + 2 * 4 * kUImg;       // per-sample rows [set 2][unit 4][4][16]: δ5 / δsdf
constexpr int kB3X = kB3Small + 2 * 4 * 4 * kU;         // x images [round parity 2][unit 4][16 × 16]
constexpr int kB3I = kB3X + 2 * 4 * 16 * kU;            // interpolation backward scatter staging [chain wave 4][512]
constexpr int kB3A = kB3I + 4 * 512;                    // chain accumulators dW1 / dW4x [chain wave 4][2][4][lane 64][4]
constexpr int kB3W5 = kB3A + 4 * 2 * 1024;              // gradient waves' dW5 / b5 partials [wave 4][lane 64][8]
constexpr int kLdsBwd3 = (kB3W5 + 4 * 64 * 8) * 4;      // 130,048 B
static_assert(kLdsBwd3 <= 160 * 1024, "bwd3 LDS budget");

typedef float f32x4v __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4v mfma16(float a, float b, f32x4v c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// 16-B buffer load: descriptor in SGPRs, one 32-bit lane offset + a
// wave-uniform byte offset (no 64-bit per-lane address arithmetic)
__device__ __forceinline__ float4 bload4(__amdgpu_buffer_rsrc_t rs, int voff, int soff) {
    const auto v = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, 0);
    return make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc_of(const float *p, int64_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p), 0, (int)bytes, 0x00020000);
}

// acc[ob] += Wᵀ blocks (ob, kb) of the image at float offset `img_off` · in[kb]
// (16 × 16 × 4 MFMAs; the A operands stream from L2 through a ring D k-blocks deep)
template <int NKB, int NOB, int D>
__device__ __forceinline__ void gemm16(__amdgpu_buffer_rsrc_t rs, int img_off, const f32x4v (&in)[NKB],
                                       f32x4v (&acc)[NOB], int lane) {
    auto ld = [&](int kb, int ob) { return bload4(rs, lane * 16, (img_off + (ob * NKB + kb) * 256) * 4); };
    float4 ring[D + 1][NOB];
#pragma unroll
    for (int s = 0; s < D; ++s)
#pragma unroll
        for (int ob = 0; ob < NOB; ++ob) ring[s][ob] = ld(s, ob);
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
        const int cs = kb % (D + 1);
        if (kb + D < NKB) {
#pragma unroll
            for (int ob = 0; ob < NOB; ++ob) ring[(kb + D) % (D + 1)][ob] = ld(kb + D, ob);
        }
#pragma unroll
        for (int ob = 0; ob < NOB; ++ob) acc[ob] = mfma16(ring[cs][ob].x, in[kb][0], acc[ob]);
#pragma unroll
        for (int ob = 0; ob < NOB; ++ob) acc[ob] = mfma16(ring[cs][ob].y, in[kb][1], acc[ob]);
#pragma unroll
        for (int ob = 0; ob < NOB; ++ob) acc[ob] = mfma16(ring[cs][ob].z, in[kb][2], acc[ob]);
#pragma unroll
        for (int ob = 0; ob < NOB; ++ob) acc[ob] = mfma16(ring[cs][ob].w, in[kb][3], acc[ob]);
        if (kb + D < NKB) __builtin_amdgcn_sched_group_barrier(0x020, NOB, 0);  // the prefetch
        __builtin_amdgcn_sched_group_barrier(0x008, 4 * NOB, 0);                // this block's MFMAs
        __builtin_amdgcn_sched_barrier(0);
    }
}

// acc[ob] += W blocks (ob, kb) of the image at `img_off` · in[kb] for NOB output
// blocks, streamed as one sequence of (output-block pair, kb) steps with the
// A-operand ring D steps deep running across the pairs (one ring fill per
// GEMM, not one per pair; 2 · 4 · (D + 1) ring registers)
template <int NKB, int NOB, int D>
__device__ __forceinline__ void gemm16_stream(__amdgpu_buffer_rsrc_t rs, int img_off, const f32x4v (&in)[NKB],
                                              f32x4v (&acc)[NOB], int lane) {
    static_assert(NOB % 2 == 0, "output blocks in pairs");
    constexpr int kSteps = NOB / 2 * NKB;
    auto ld = [&](int st, int i) {
        const int ob = 2 * (st / NKB) + i, kb = st % NKB;
        return bload4(rs, lane * 16, (img_off + (ob * NKB + kb) * 256) * 4);
    };
    float4 ring[D + 1][2];
#pragma unroll
    for (int st = 0; st < D; ++st)
#pragma unroll
        for (int i = 0; i < 2; ++i) ring[st][i] = ld(st, i);
#pragma unroll
    for (int st = 0; st < kSteps; ++st) {
        const int cs = st % (D + 1), ob = 2 * (st / NKB), kb = st % NKB;
        if (st + D < kSteps) {
#pragma unroll
            for (int i = 0; i < 2; ++i) ring[(st + D) % (D + 1)][i] = ld(st + D, i);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[ob + i] = mfma16(ring[cs][i].x, in[kb][0], acc[ob + i]);
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[ob + i] = mfma16(ring[cs][i].y, in[kb][1], acc[ob + i]);
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[ob + i] = mfma16(ring[cs][i].z, in[kb][2], acc[ob + i]);
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[ob + i] = mfma16(ring[cs][i].w, in[kb][3], acc[ob + i]);
        if (st + D < kSteps) __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);  // the prefetch
        __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);                      // this step's MFMAs
        __builtin_amdgcn_sched_barrier(0);
    }
}

template <int N>
__device__ __forceinline__ void zero4(f32x4v (&v)[N]) {
#pragma unroll
    for (int b = 0; b < N; ++b) v[b] = f32x4v{0.f, 0.f, 0.f, 0.f};
}

// ReLU mask of a 128-feature activation: feature 16·ob + 4q + j is bit
// 8·ob + j of w (the forward's mask word of lane-half q & 1, shifted by 4·(q >> 1))
__device__ __forceinline__ void mask16(f32x4v (&v)[8], uint64_t w) {
#pragma unroll
    for (int ob = 0; ob < 8; ++ob)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t keep = 0u - (uint32_t)((w >> (8 * ob + j)) & 1u);
            v[ob][j] = __uint_as_float(__float_as_uint(v[ob][j]) & keep);
        }
}

__device__ __forceinline__ uint64_t relu16(f32x4v (&v)[8]) {
    uint64_t w = 0;
#pragma unroll
    for (int ob = 0; ob < 8; ++ob)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool on = v[ob][j] > 0.0f;
            w |= (uint64_t)on << (8 * ob + j);
            v[ob][j] = on ? v[ob][j] : 0.0f;
        }
    return w;
}

// a chain wave's activation → its unit image (rows 16·ob + 4q + j; `wb` = the
// lane's base: 64q + ((chunk ^ q) << 2) + word), and back
template <int NOB>
__device__ __forceinline__ void lds_u_store(float *img, int wb, const f32x4v (&v)[NOB]) {
#pragma unroll
    for (int ob = 0; ob < NOB; ++ob)
#pragma unroll
        for (int j = 0; j < 4; ++j) img[wb + 256 * ob + 16 * j] = v[ob][j];
}
template <int NOB>
__device__ __forceinline__ void lds_u_load(const float *img, int wb, f32x4v (&v)[NOB]) {
#pragma unroll
    for (int ob = 0; ob < NOB; ++ob)
#pragma unroll
        for (int j = 0; j < 4; ++j) v[ob][j] = img[wb + 256 * ob + 16 * j];
}

// Σ of v over the 16 lanes of the lane's DPP row (the chain's samples n of one
// q group), in every lane of the row: quad xor 1, xor 2, half-row mirror, row mirror
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float x) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float row_sum16(float v) {
    v += dpp_mov<0xB1>(v);   // quad_perm [1, 0, 3, 2]
    v += dpp_mov<0x4E>(v);   // quad_perm [2, 3, 0, 1]
    v += dpp_mov<0x141>(v);  // row_half_mirror
    v += dpp_mov<0x140>(v);  // row_mirror
    return v;
}

// chain wave: acc += δ rows [32c, 32c + 32) of the round's unit images ⊗ the
// units' x images (16 valid columns: lanes ≥ 16 feed zeros); bsum: Σ of the
// rows.  The accumulator lives in LDS between phases (`page`: [4][lane][4]
// floats, this wave's own): read, accumulated, written back — the same bits
// as a register-resident accumulator, 16 registers free in the other phases.
__device__ __forceinline__ void xgrad16(const float *dset, const float *xset, int c, int64_t ubase, int64_t u1,
                                        int lane, float *page, float *bsum) {
    const int i = lane & 31, h = lane >> 5;
    if (ubase >= u1) return;
    f32x16 acc;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float4 v = *reinterpret_cast<const float4 *>(page + (k * 64 + lane) * 4);
        acc[4 * k] = v.x;
        acc[4 * k + 1] = v.y;
        acc[4 * k + 2] = v.z;
        acc[4 * k + 3] = v.w;
    }
    const bool xv = i < 16;
    int ra[2], rx[2];
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        ra[g] = i * kU + (((2 * h + g) ^ ((i >> 2) & 3)) << 2);
        rx[g] = (i & 15) * kU + (((2 * h + g) ^ (((i & 15) >> 2) & 3)) << 2);
    }
#pragma unroll
    for (int up = 0; up < 4; ++up) {
        if (ubase + up >= u1) break;  // wave-uniform
        const float *dl = dset + up * kUImg + 32 * c * kU;
        const float *xl = xset + up * 16 * kU;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const float4 a = *reinterpret_cast<const float4 *>(dl + ra[g]);
            float4 b = *reinterpret_cast<const float4 *>(xl + rx[g]);
            if (!xv) b = make_float4(0.f, 0.f, 0.f, 0.f);
            acc = mfma(a.x, b.x, acc);
            acc = mfma(a.y, b.y, acc);
            acc = mfma(a.z, b.z, acc);
            acc = mfma(a.w, b.w, acc);
            if (bsum) *bsum += (a.x + a.y) + (a.z + a.w);
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        *reinterpret_cast<float4 *>(page + (k * 64 + lane) * 4) =
            make_float4(acc[4 * k], acc[4 * k + 1], acc[4 * k + 2], acc[4 * k + 3]);
}

// byte offset within a CF tile of lane (i, h)'s operand: row 32·blk + i,
// 16-B group h·4 + 2·hf + g (hf: the unit's half of the 32-sample tile).
// Computed, not selected from a table: a runtime index into a register
// array sends the array to scratch.
__device__ __forceinline__ int cf_voff(int blk, int lane, int hf, int g) {
    const int row = 32 * blk + (lane & 31);
    return (row * kTileS + ((((lane >> 5) * 4 + 2 * hf + g) ^ ((row >> 1) & 7)) << 2)) * 4;
}

// gradient wave c (P0, the previous round's units): dW5 column block c +=
// δ5 ⊗ c1 (VALU), b5 partials — in the phase where the gradient waves have
// no GEMM (on the chain, in P2, it lengthened the chain's longest phase); the
// c1 operands of two units in flight at a time
__device__ __forceinline__ void w5_grad(const float *sset, __amdgpu_buffer_rsrc_t c1m, int c, int64_t ubase,
                                        int64_t u1, int lane, float (&w5)[3], float (&b5)[3]) {
    const int h = lane >> 5;
#pragma unroll
    for (int pr = 0; pr < 4; ++pr) {
        float4 cl[1][2];
#pragma unroll
        for (int k = 0; k < 1; ++k) {
            int64_t u = ubase + pr + k;
            if (u >= u1) u = u1 - 1;  // in range (data unused)
#pragma unroll
            for (int g = 0; g < 2; ++g)
                cl[k][g] = bload4(c1m, cf_voff(c, lane, (int)(u & 1), g), (int)((u >> 1) * (kCfTile * 4)));
        }
#pragma unroll
        for (int k = 0; k < 1; ++k) {
            const int up = pr + k;
            if (ubase + up >= u1) break;
            const float *sl = sset + up * 4 * kU + 8 * h;
#pragma unroll
            for (int g = 0; g < 2; ++g)
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const float4 w = *reinterpret_cast<const float4 *>(sl + ch * kU + 4 * g);
                    const float4 a = cl[k][g];
                    w5[ch] += (a.x * w.x + a.y * w.y) + (a.z * w.z + a.w * w.w);
                    b5[ch] += (w.x + w.y) + (w.z + w.w);
                }
        }
    }
}

// gradient wave B operand: step q (unit q >> 1, k-group q & 1) of column block d
__device__ __forceinline__ float4 dw_bsrc(__amdgpu_buffer_rsrc_t act, int64_t ubase, int64_t u1, int d, int lane, int q) {
    int64_t u = ubase + (q >> 1);
    if (u >= u1) u = u1 - 1;  // in range (data unused)
    if (u < 0) u = 0;
    return bload4(act, cf_voff(d, lane, (int)(u & 1), q & 1), (int)((u >> 1) * (kCfTile * 4)));
}

// gradient wave, one job (a phase's layer): acc[ob] += δ (the round's unit
// images, all 4 row blocks) ⊗ the activation's column block d; bsum += Σ of
// row block d; EX = 2 (W3): row0 += δsdf ⊗ h2, b30 += Σ δsdf.  The B
// operands run through a 3-slot ring two steps ahead that continues into
// the next job (its first two loads are issued here, before the barrier):
// step q of a job with ring offset RO uses slot (RO + q) % 3.
template <int EX, int RO>
__device__ __forceinline__ void dw_job(float4 (&ring)[3], const float *dset, const float *sset,
                                       __amdgpu_buffer_rsrc_t act, int64_t ubase, bool on,
                                       __amdgpu_buffer_rsrc_t act_n, int64_t ubase_n, bool has_n, int64_t u1, int d,
                                       int lane, f32x16 (&acc)[kNB], float &bsum, float &row0, float &b30) {
    const int i = lane & 31, h = lane >> 5;
    int ra[2];
#pragma unroll
    for (int g = 0; g < 2; ++g) ra[g] = i * kU + (((2 * h + g) ^ ((i >> 2) & 3)) << 2);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int up = q >> 1, g = q & 1;
        const float4 b = ring[(RO + q) % 3];
        if (q + 2 < 8) ring[(RO + q + 2) % 3] = dw_bsrc(act, ubase, u1, d, lane, q + 2);
        else if (has_n) ring[(RO + q + 2) % 3] = dw_bsrc(act_n, ubase_n, u1, d, lane, q - 6);
        if (on && ubase + up < u1) {  // wave-uniform
            const float *dl = dset + up * kUImg;
            float4 a[kNB];
#pragma unroll
            for (int ob = 0; ob < kNB; ++ob) a[ob] = *reinterpret_cast<const float4 *>(dl + 32 * ob * kU + ra[g]);
#pragma unroll
            for (int ob = 0; ob < kNB; ++ob) acc[ob] = mfma(a[ob].x, b.x, acc[ob]);
#pragma unroll
            for (int ob = 0; ob < kNB; ++ob) acc[ob] = mfma(a[ob].y, b.y, acc[ob]);
#pragma unroll
            for (int ob = 0; ob < kNB; ++ob) acc[ob] = mfma(a[ob].z, b.z, acc[ob]);
#pragma unroll
            for (int ob = 0; ob < kNB; ++ob) acc[ob] = mfma(a[ob].w, b.w, acc[ob]);
            {  // row block d's sum: its own read (a[d] with a runtime d would put a[] in scratch)
                const float4 ad = *reinterpret_cast<const float4 *>(dl + 32 * d * kU + ra[g]);
                bsum += (ad.x + ad.y) + (ad.z + ad.w);
            }
            if (EX == 2) {
                const float4 w = *reinterpret_cast<const float4 *>(sset + up * 4 * kU + 8 * h + 4 * g);
                row0 += (b.x * w.x + b.y * w.y) + (b.z * w.z + b.w * w.w);
                b30 += (w.x + w.y) + (w.z + w.w);
            }
        }
    }
}

// gradient wave, dW2 += δh2 (the round's unit images) ⊗ h1 (the round's CF
// image in LDS), column block d — dw_job's arithmetic with both operands on chip
__device__ __forceinline__ void dw_job_lds(const float *dset, const float *cf, int64_t ubase, int64_t u1, int d,
                                           int lane, f32x16 (&acc)[kNB], float &bsum) {
    const int i = lane & 31, h = lane >> 5;
    int ra[2];
#pragma unroll
    for (int g = 0; g < 2; ++g) ra[g] = i * kU + (((2 * h + g) ^ ((i >> 2) & 3)) << 2);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int up = q >> 1, g = q & 1;
        if (ubase + up >= u1) break;  // wave-uniform
        const float4 b = *reinterpret_cast<const float4 *>(cf + (up >> 1) * kCfTile + cf_voff(d, lane, up & 1, g) / 4);
        const float *dl = dset + up * kUImg;
        float4 a[kNB];
#pragma unroll
        for (int ob = 0; ob < kNB; ++ob) a[ob] = *reinterpret_cast<const float4 *>(dl + 32 * ob * kU + ra[g]);
#pragma unroll
        for (int ob = 0; ob < kNB; ++ob) acc[ob] = mfma(a[ob].x, b.x, acc[ob]);
#pragma unroll
        for (int ob = 0; ob < kNB; ++ob) acc[ob] = mfma(a[ob].y, b.y, acc[ob]);
#pragma unroll
        for (int ob = 0; ob < kNB; ++ob) acc[ob] = mfma(a[ob].z, b.z, acc[ob]);
#pragma unroll
        for (int ob = 0; ob < kNB; ++ob) acc[ob] = mfma(a[ob].w, b.w, acc[ob]);
        const float4 ad = *reinterpret_cast<const float4 *>(dl + 32 * d * kU + ra[g]);
        bsum += (ad.x + ad.y) + (ad.z + ad.w);
    }
}

// write C blocks to the slab (rows offset `row_off` in the layer's matrix)
template <int NR, int NC, bool NT = false>
__device__ __forceinline__ void dw_store(float *slab, int cols, int row_off, int max_col, const int (&rb)[NR],
                                         const int (&cb)[NC], const f32x16 (&acc)[NR][NC], int lane) {
    const int x = lane & 31, h = lane >> 5;
#pragma unroll
    for (int i = 0; i < NR; ++i)
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const int col = 32 * cb[j] + x;
            if (col >= max_col) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (NT) {
                    store_nt(slab, (row_off + 32 * rb[i] + phi(r, h)) * cols + col, acc[i][j][r]);
                } else {
                    slab[(row_off + 32 * rb[i] + phi(r, h)) * cols + col] = acc[i][j][r];
                }
            }
        }
}

}  // namespace
}  // namespace psvo
