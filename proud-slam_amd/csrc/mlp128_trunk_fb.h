// Width-128 decoder, the sparse decoder's class B (mlp128.h: the layer
// equations and layouts): k_mlp_trunk_fb, the sdf trunk's forward and
// backward in one kernel, and its launcher.  Its body also runs on the
// class-B workgroups of mlp_bwd.hip's k_mlp_bwd3<W, H2> (the default); as a
// launch of its own dec128_bwd queues it after k_mlp_bwd3<W>, and
// k_mlp_dw_reduce adds its slabs to that kernel's.
//
// A header of mlp_bwd.hip, not a translation unit of its own: k_mlp_bwd3 and
// this kernel share mlp128_chain16.h's helpers, and compiled apart both come
// out with other device code (the optimiser propagates argument facts over
// all callers of an internal function before it inlines it; same registers,
// other schedule) — both sit on the 256-register limit, so they stay as they
// were measured.
#pragma once
#include "interp_fuse.h"
#include "mlp128_chain16.h"

namespace psvo {
namespace {

using ifuse::interp_bwd_unit;
using ifuse::scatter_unit;

// ---------------------------------------------------------------------------
// The sparse decoder's class B (samples whose only loss term is the direct
// one on their sdf — composite.hip k_select_samples): their colour head's δ's
// are exactly zero (g_rgb = 0, so δ5 = δc1 = δf = 0), so forward and backward
// need the trunk only:
//   h1 = relu(W1 x + b1),  h2 = relu(W2 h1 + b2)                       (forward)
//   δh2 = W3[0]ᵀ dsdf ⊙ [h2 > 0],  δh1 = W2ᵀ δh2 ⊙ [h1 > 0],  dfeat = W1ᵀ δh1
//   dW1 += δh1 ⊗ x,  dW2 += δh2 ⊗ h1,  W3 row 0 += dsdf · h2  (+ b1, b2, b3[0])
// 54 k MACs per sample, in ONE kernel that keeps the activations on chip (no
// activation round trip through HBM, no separate forward launch: the two
// measured 57 + 110 µs at config B).  The forward is recomputed here with the
// chain's 16 × 16 × 4 MFMAs (the sdf came from k_mlp_sdf2: the same values up
// to the accumulation order, which only the ReLU masks' ties could see).
// Rounds of four 16-sample units (unit u0 + 4r + k on chain wave k and
// gradient wave 4 + k), two phases each:
//   phase  chain wave c                                    gradient wave d
//   P(r)   δh2(r) from LDS; δh1 = W2ᵀ δh2 ⊙ [h1 > 0]       dW2 col block d += δh2(r) ⊗ h1(r)
//          → LDS                                           (both operands in LDS)
//   Q(r)   dfeat = W1ᵀ δh1 → the interpolation backward    dW1 row block d += δh1(r) ⊗ x(r); the
//          (dL/dx, the embedding scatter)                  forward of unit d of round r + 1: x → LDS,
//                                                          h1 = relu(W1 x + b1) → LDS (CF tile),
//                                                          h2 = relu(W2 h1 + b2), W3 row 0 += dsdf · h2,
//                                                          δh2 → LDS, the h1 mask words → LDS
// (the forward of round 0 before the loop).  A chain wave and a gradient
// wave share each SIMD's matrix unit: in P both run 128 × 128 GEMMs (W2ᵀ,
// dW2), in Q the gradient wave's forward overlaps the chain's latency-bound
// interpolation backward.  (The forward on the chain waves, with W2ᵀ in one
// phase: 42 k cycles per round, the chain alone in that phase for 62 % of
// it — s_memtime stamps, scripts/trunk_stamps.py.)  Writes one slab per
// workgroup of W1 (+ b1), W2 (+ b2) and W3's row 0 (+ b3[0]) in `slabs` (the
// DwGrid layout; k_mlp_dw_reduce adds these elements only).  m: the class's
// count on the device.
constexpr int kT4H2 = kVecPad;                 // δh2 unit images [unit 4]
constexpr int kT4H1 = kT4H2 + 4 * kUImg;       // δh1 unit images [unit 4]
constexpr int kT4CF = kT4H1 + 4 * kUImg;       // h1 as CF tiles [2] (the round's unit k → tile k / 2, half k % 2)
constexpr int kT4X = kT4CF + 2 * kCfTile;      // x images [round parity 2][unit 4][16 × 16]
constexpr int kT4I = kT4X + 2 * 4 * 16 * kU;   // interpolation backward staging [chain wave 4][512]
constexpr int kT4R = kT4I + 4 * 512;           // W3 row 0 / b3[0] partials [gradient wave 4][132]
constexpr int kT4M = kT4R + 4 * 132;           // h1 mask words [unit 4][lane 64] (u64)
constexpr int kLdsTrunk = (kT4M + 4 * 64 * 2) * 4;  // 123,968 B
static_assert(kLdsTrunk <= 160 * 1024, "trunk kernel LDS budget");

struct TrunkIn {
    float gs;
    float4 x;
    int src;  // the sample's h2 row (h2 given), else 0
};
__device__ __forceinline__ void load_trunk_in(const float *__restrict__ g_sdf, const float *__restrict__ feat,
                                              const int *__restrict__ src, int64_t s, bool valid, int q,
                                              TrunkIn &in) {
    const int64_t sv = valid ? s : 0;
    in.gs = g_sdf[sv];
    in.src = src && valid ? src[sv] : 0;
    in.x = *reinterpret_cast<const float4 *>(feat + (src ? (int64_t)in.src : sv) * kIn + 4 * q);  // (src: feat is
                                                                                                 // the step's rows)
}

// gradient wave k: the trunk forward of unit k of round r (chain layout: lane
// (n, q) holds features 16·ob + 4q + j of sample n) → x image, h1 CF tile,
// δh2 unit image, h1 mask words; W3 row 0 / b3[0] partials into `page3`
template <bool H2>
__device__ __forceinline__ void trunk_fwd_unit(float *lds, __amdgpu_buffer_rsrc_t wrs, const TrunkIn &in, int64_t u,
                                               int64_t u1, int64_t m, int k, int lane, int wb, float *xl,
                                               float *page3, float &b30p, const float *__restrict__ h2) {
    const int n = lane & 15, q = lane >> 4;
    const int64_t s = u * kU + n;
    const bool active = u < u1;  // wave-uniform
    const bool valid = active && s < m;
    const float dsdf = valid ? in.gs : 0.0f;
    const float4 xv = valid ? in.x : make_float4(0.f, 0.f, 0.f, 0.f);
    xl[wb + 0] = xv.x;
    xl[wb + 16] = xv.y;
    xl[wb + 32] = xv.z;
    xl[wb + 48] = xv.w;
    if (!active) return;
    f32x4v fb[8];
    f32x4v xin[1] = {f32x4v{xv.x, xv.y, xv.z, xv.w}};
    f32x4v hb[8];
#pragma unroll
    for (int ob = 0; ob < 8; ++ob) {
        const float4 bb = *reinterpret_cast<const float4 *>(lds + kOffB1 + 16 * ob + 4 * q);
        hb[ob] = f32x4v{bb.x, bb.y, bb.z, bb.w};
    }
    gemm16_stream<1, 8, 3>(wrs, kImgT1, xin, hb, lane);  // h1 = W1 x + b1
    if (H2) {  // h2 read: features 16 ob + 4q .. + 3 of the sample's row (in flight under h1's ReLU and stores)
        const float *row = h2 + (int64_t)in.src * kW;
#pragma unroll
        for (int ob = 0; ob < 8; ++ob) {
            float4 v = *reinterpret_cast<const float4 *>(row + 16 * ob + 4 * q);
            if (!valid) v = make_float4(0.f, 0.f, 0.f, 0.f);
            fb[ob] = f32x4v{v.x, v.y, v.z, v.w};
        }
    }
    const uint64_t m1 = relu16(hb);
    reinterpret_cast<uint64_t *>(lds + kT4M)[k * 64 + lane] = m1;
    {  // h1 → the CF tile (dW2's B operand; k_mlp_fwd2's layout): row 16 ob + 4q + j,
       // sample n at group 4 (n & 1) + 2 (k & 1) + n / 8, element (n / 2) & 3;
       // the row's swizzle (row >> 1) & 7 does not depend on ob
        const int grp = 4 * (n & 1) + 2 * (k & 1) + (n >> 3), el = (n >> 1) & 3;
        float *const tile = lds + kT4CF + (k >> 1) * kCfTile;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float *const cj = tile + (4 * q + j) * kTileS + ((grp ^ ((2 * q + (j >> 1)) & 7)) << 2) + el;
#pragma unroll
            for (int ob = 0; ob < 8; ++ob) cj[16 * ob * kTileS] = hb[ob][j];
        }
    }
    if (!H2) {
#pragma unroll
        for (int ob = 0; ob < 8; ++ob) {
            const float4 bb = *reinterpret_cast<const float4 *>(lds + kOffB2 + 16 * ob + 4 * q);
            fb[ob] = f32x4v{bb.x, bb.y, bb.z, bb.w};
        }
        // h2 = W2 h1 + b2: output-block pairs, one ring across them (beside the dW2
        // accumulators a ring over all 8 output blocks spills)
        gemm16_stream<8, 8, 3>(wrs, kImgT2, hb, fb, lane);
    }
    const uint64_t m2 = relu16(fb);
    {  // W3 row 0 += Σ_n dsdf · h2 (the unit's 16 samples by DPP row sums, into the page)
        f32x4v r0[8];
#pragma unroll
        for (int ob = 0; ob < 8; ++ob)
#pragma unroll
            for (int j = 0; j < 4; ++j) r0[ob][j] = row_sum16(fb[ob][j] * dsdf);
        if (n == 0) {
#pragma unroll
            for (int ob = 0; ob < 8; ++ob) {
                float4 *pp = reinterpret_cast<float4 *>(page3 + 16 * ob + 4 * q);
                const float4 o = *pp;
                *pp = make_float4(o.x + r0[ob][0], o.y + r0[ob][1], o.z + r0[ob][2], o.w + r0[ob][3]);
            }
        }
    }
    b30p += dsdf;
#pragma unroll
    for (int ob = 0; ob < 8; ++ob) {  // δh2 = W3[0]ᵀ dsdf ⊙ [h2 > 0] (k_mlp_bwd3's δf = 0 case)
        const float4 w = *reinterpret_cast<const float4 *>(lds + kOffW3r0 + 16 * ob + 4 * q);
        fb[ob] = f32x4v{__fmul_rn(w.x, dsdf), __fmul_rn(w.y, dsdf), __fmul_rn(w.z, dsdf), __fmul_rn(w.w, dsdf)};
    }
    mask16(fb, m2);
    lds_u_store<8>(lds + kT4H2 + k * kUImg, wb, fb);
}

//
// The body is a device function of its workgroup's place: workgroup `wg` of
// the `n_wg` that share the m samples, writing slab `b` (k_mlp_trunk_fb below:
// the whole grid; mlp_bwd.hip's k_mlp_bwd3<W, H2>: the grid's class-B part).
template <bool H2>
__device__ __forceinline__ void mlp_trunk_fb_body(const unsigned wg, const unsigned n_wg, const int b, const int64_t m,
                                                  const float *__restrict__ img, const float *__restrict__ g_sdf,
                                                  const float *__restrict__ feat, const DwGrid &g,
                                                  float *__restrict__ slabs, const InterpFuse &ip,
                                                  const float *__restrict__ h2, const int *__restrict__ h2_src) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t n_units = (m + kU - 1) / kU;
    const int64_t u0 = n_units * wg / n_wg, u1 = n_units * (wg + 1) / n_wg;
    const int n_rounds = (int)((u1 - u0 + 3) / 4);
    float *const h2set = lds + kT4H2, *const h1set = lds + kT4H1, *const cf = lds + kT4CF;
    auto xset = [&](int par) { return lds + kT4X + (par & 1) * 4 * 16 * kU; };
    stage8(lds, img + kImgVec, kVecPad, wave, lane);
    wait_vm(0);
    raw_barrier();
    const int i = lane & 31, h = lane >> 5;
    const int n = lane & 15, q = lane >> 4;
    const int sn = (n & 1) * 8 + (n >> 1);                     // the sample's slot in a unit image
    const int wb = 64 * q + ((((sn >> 2) ^ q) << 2) | (sn & 3));  // + 256 ob + 16 j
    const __amdgpu_buffer_rsrc_t wrs = rsrc_of(img, (int64_t)kImgTotal * 4);
    const bool fuse = ip.gx != nullptr;  // uniform
    [[maybe_unused]] constexpr int kStampK = 2;
    PSVO_STAMP_DECL;
    if (wave < 4) {
        // ================= chain wave c
        const int c = wave;
        f32x4v w1acc[8];  // dW1 partials of this wave's units: rows 16 t + 4 (lane >> 4) + j, column lane & 15
        zero4(w1acc);
        float b1p[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // b1 partials: rows 16 t + (lane & 15)
        int lf_n = 0, ro_n = 0;
        float ts_n = 0.f;
        {
            const int64_t u = u0 + c;
            const int64_t s = u * kU + n;
            if (fuse && u < u1 && s < m) {
                lf_n = ip.leaf[s];
                ro_n = ip.ray_of[s];
                ts_n = ip.t[s];
            }
        }
        for (int r = 0; r < n_rounds; ++r) {
            PSVO_STAMP(0);
            const int64_t u = u0 + 4 * (int64_t)r + c;
            const bool active = u < u1;  // wave-uniform
            const int64_t s = u * kU + n;
            const bool valid = active && s < m;
            const int lf = lf_n, ro = ro_n;
            const float ts = ts_n;
            int4 vid0 = make_int4(0, 0, 0, 0), vid1 = make_int4(0, 0, 0, 0);
            float cen[3] = {0.f, 0.f, 0.f};
            int row = 0;
            if (fuse && valid) {
                vid0 = *reinterpret_cast<const int4 *>(ip.vertex_idx + (int64_t)lf * 8);
                vid1 = *reinterpret_cast<const int4 *>(ip.vertex_idx + (int64_t)lf * 8 + 4);
#pragma unroll
                for (int a = 0; a < 3; ++a) cen[a] = ip.centres[(int64_t)lf * 3 + a];
                row = ip.rank_ray[ro];
            }
            raw_barrier();  // the round's forward (gradient waves) is in LDS
            PSVO_STAMP(1);
            // ---- P: δh1 = W2ᵀ δh2 ⊙ [h1 > 0] → LDS
            f32x4v fa[8];
            if (active) {
                f32x4v fb[8];
                lds_u_load<8>(h2set + c * kUImg, wb, fb);
                const uint64_t m1 = reinterpret_cast<const uint64_t *>(lds + kT4M)[c * 64 + lane];
                zero4(fa);
                gemm16<8, 8, 2>(wrs, kImgC2, fb, fa, lane);  // one ring over all 8 output blocks
                mask16(fa, m1);
                lds_u_store<8>(h1set + c * kUImg, wb, fa);
            }
            PSVO_STAMP(2);
            raw_barrier();
            PSVO_STAMP(3);
            // ---- Q: dfeat = W1ᵀ δh1 → the interpolation backward; the next unit's inputs
            if (r + 1 < n_rounds) {
                const int64_t un = u + 4;
                const int64_t snx = un * kU + n;
                if (fuse && un < u1 && snx < m) {
                    lf_n = ip.leaf[snx];
                    ro_n = ip.ray_of[snx];
                    ts_n = ip.t[snx];
                }
            }
            if (active) {
                f32x4v t1[1];
                zero4(t1);
                gemm16<8, 1, 4>(wrs, kImgC1, fa, t1, lane);
                // dW1 += δh1 ⊗ x of this unit (16 × 16 × 4 MFMAs over its 16 samples: lane (m, kq)
                // feeds slots 4 kq .. 4 kq + 3 of row 16 t + m, one 16-B chunk of each image)
                {
                    const int mr = lane & 15, kq = lane >> 4;
                    const float *dl = h1set + c * kUImg, *xl = xset(r) + c * 16 * kU;
                    const float4 bx = *reinterpret_cast<const float4 *>(xl + mr * kU + ((kq ^ ((mr >> 2) & 3)) << 2));
#pragma unroll
                    for (int t = 0; t < 8; ++t) {
                        const int rw = 16 * t + mr;
                        const float4 a = *reinterpret_cast<const float4 *>(dl + rw * kU + ((kq ^ ((rw >> 2) & 3)) << 2));
                        w1acc[t] = mfma16(a.x, bx.x, w1acc[t]);
                        w1acc[t] = mfma16(a.y, bx.y, w1acc[t]);
                        w1acc[t] = mfma16(a.z, bx.z, w1acc[t]);
                        w1acc[t] = mfma16(a.w, bx.w, w1acc[t]);
                        b1p[t] += (a.x + a.y) + (a.z + a.w);
                    }
                }
                PSVO_STAMP(4);
                const float4 gf = make_float4(t1[0][0], t1[0][1], t1[0][2], t1[0][3]);
                if (fuse) {
                    float ro3[3] = {0.f, 0.f, 0.f}, rd3[3] = {0.f, 0.f, 0.f};
                    float4 ev[8];
                    const int vid[8] = {vid0.x, vid0.y, vid0.z, vid0.w, vid1.x, vid1.y, vid1.z, vid1.w};
#pragma unroll
                    for (int k = 0; k < 8; ++k) ev[k] = reinterpret_cast<const float4 *>(ip.emb)[(int64_t)vid[k] * 4 + q];
                    if (valid) {
#pragma unroll
                        for (int a = 0; a < 3; ++a) {
                            ro3[a] = ip.rays_o[(int64_t)row * 3 + a];
                            rd3[a] = ip.rays_d[(int64_t)row * 3 + a];
                        }
                    }
                    interp_bwd_unit(ip, lds + kT4I + c * 512, m, s, valid, n, q, ts, ro3, rd3, cen, vid0, vid1, ev,
                                    gf);
                    PSVO_STAMP(5);
                    if (ip.grad_emb != nullptr) {
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // the staging is this wave's own
                        __builtin_amdgcn_wave_barrier();
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                        scatter_unit(ip, lds + kT4I + c * 512, u, m, lane, lf);
                    }
                }
            }
            PSVO_STAMP(6);
            PSVO_STAMP_FLUSH(0);
        }
        // this wave's dW1 / b1 partials → LDS (the CF tiles and mask words: read in P only)
        float *const pw = lds + kT4CF + c * 2048;
#pragma unroll
        for (int t = 0; t < 8; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) pw[(16 * t + 4 * (lane >> 4) + j) * 16 + (lane & 15)] = w1acc[t][j];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            float v = b1p[t];
            v += __shfl_xor(v, 16, 64);
            v += __shfl_xor(v, 32, 64);
            if (lane < 16) lds[kT4M + c * 128 + 16 * t + lane] = v;
        }
    } else {
        // ================= gradient wave: column block d of W2, row block d of W1, the forward of unit d
        const int d = wave - 4;
        f32x16 acc2[kNB];
        zero(acc2);
        float b2p = 0.f, b30p = 0.f;
        float *const page3 = lds + kT4R + d * 132;   // W3 row 0 (+ b3[0]) partials of this wave's units
        if (lane < 33) *reinterpret_cast<float4 *>(page3 + 4 * lane) = make_float4(0.f, 0.f, 0.f, 0.f);
        TrunkIn nin;
        auto load_in = [&](int r) {
            const int64_t u = u0 + 4 * (int64_t)r + d;
            const int64_t s = u * kU + n;
            load_trunk_in(g_sdf, feat, H2 ? h2_src : nullptr, s, u < u1 && s < m, q, nin);
        };
        if (n_rounds > 0) {  // the forward of round 0
            load_in(0);
            const TrunkIn in = nin;
            if (n_rounds > 1) load_in(1);
            trunk_fwd_unit<H2>(lds, wrs, in, u0 + d, u1, m, d, lane, wb, xset(0) + d * 16 * kU, page3, b30p, h2);
        }
        for (int r = 0; r < n_rounds; ++r) {
            PSVO_STAMP(0);
            const int64_t ubase = u0 + 4 * (int64_t)r;
            raw_barrier();
            PSVO_STAMP(1);
            // P (beside the chain's W2ᵀ): dW2 += δh2 ⊗ h1 of this round
            dw_job_lds(h2set, cf, ubase, u1, d, lane, acc2, b2p);
            PSVO_STAMP(2);
            raw_barrier();
            PSVO_STAMP(3);
            // Q (beside the chain's interpolation backward): the next round's forward
            PSVO_STAMP(4);
            if (r + 1 < n_rounds) {
                const TrunkIn in = nin;
                if (r + 2 < n_rounds) load_in(r + 2);
                trunk_fwd_unit<H2>(lds, wrs, in, ubase + 4 + d, u1, m, d, lane, wb, xset(r + 1) + d * 16 * kU,
                                   page3, b30p, h2);
            }
            PSVO_STAMP(6);
            PSVO_STAMP_FLUSH(0);
        }
        // b3[0]: Σ dsdf (every sample's in each of the 4 q rows: row 0's)
        const float bs = row_sum16(b30p);
        if (lane == 0) page3[128] = bs;
        const int rb[kNB] = {0, 1, 2, 3}, cb[1] = {d};
        float *s2 = slabs + g.slab_off[1] + (int64_t)b * g.slab_len[1];
        {
            f32x16 t[kNB][1];
#pragma unroll
            for (int k = 0; k < kNB; ++k) t[k][0] = acc2[k];
            dw_store<kNB, 1, true>(s2, 128, 0, 128, rb, cb, t, lane);
        }
        const float v2 = b2p + __shfl_xor(b2p, 32, 64);
        if (h == 0) store_nt(s2, 128 * 128 + 32 * d + i, v2);
    }
    // W3 row 0 (+ b3[0]): the gradient waves' pages; W1 (+ b1): the chain
    // waves' partials — each summed in wave order
    __syncthreads();
    {
        float *s1 = slabs + g.slab_off[0] + (int64_t)b * g.slab_len[0];
        for (int e = threadIdx.x; e < 128 * 16 + 128; e += kF2Threads) {
            float v = 0.f;
            if (e < 128 * 16) {
#pragma unroll
                for (int k = 0; k < 4; ++k) v += lds[kT4CF + k * 2048 + e];
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) v += lds[kT4M + k * 128 + e - 128 * 16];
            }
            store_nt(s1, e, v);
        }
    }
    if (wave >= 4) {
        const int d = wave - 4;
        float *s3 = slabs + g.slab_off[2] + (int64_t)b * g.slab_len[2];
        if (h == 0) {
            float v = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) v += lds[kT4R + k * 132 + 32 * d + i];
            store_nt(s3, 32 * d + i, v);
        }
        if (d == 0 && lane == 0) {
            float v = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) v += lds[kT4R + k * 132 + 128];
            store_nt(s3, 129 * 128, v);
        }
    }
}

template <bool H2>
__global__ __launch_bounds__(kF2Threads, 1) void k_mlp_trunk_fb(const int *__restrict__ m_dev,
                                                                const float *__restrict__ img,
                                                                const float *__restrict__ g_sdf,
                                                                const float *__restrict__ feat, DwGrid g,
                                                                float *__restrict__ slabs, InterpFuse ip,
                                                                const float *__restrict__ h2,
                                                                const int *__restrict__ h2_src) {
    const int64_t m = __builtin_amdgcn_readfirstlane(*m_dev);
    mlp_trunk_fb_body<H2>(blockIdx.x, gridDim.x, blockIdx.x, m, img, g_sdf, feat, g, slabs, ip, h2, h2_src);
}

// one slab of g's layout per workgroup (the caller binds the stop event and checks the launch)
void launch_trunk_fb(hipStream_t st, int grid, const float *images, const TrunkBwd &tb, const DwGrid &g,
                     float *slabs) {
    const InterpFuse ip = tb.ip ? *tb.ip : InterpFuse{};
    if (tb.h2)
        launch_lds<k_mlp_trunk_fb<true>>(dim3(grid), dim3(kF2Threads), kLdsTrunk, st, tb.m_dev, images, tb.g_sdf,
                                         tb.feat, g, slabs, ip, tb.h2, tb.src);
    else
        launch_lds<k_mlp_trunk_fb<false>>(dim3(grid), dim3(kF2Threads), kLdsTrunk, st, tb.m_dev, images, tb.g_sdf,
                                          tb.feat, g, slabs, ip, tb.h2, tb.src);
}

}  // namespace
}  // namespace psvo
