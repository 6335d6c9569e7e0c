// Width-128 decoder, backward (mlp128.h: the layer equations and layouts):
//   k_mlp_bwd3<W>      the δ chain and the weight gradients in one persistent
//                      kernel, one slab of every layer per workgroup
//   k_mlp_bwd3<W, H2>  the same body on a part of the grid and the sparse
//                      decoder's class-B body (mlp128_trunk_fb.h, compiled
//                      here) on the rest: both sample classes in one launch
//   k_mlp_dw_reduce    the slab sum
// and dec128_bwd, the one host function that chooses between that launch and
// the two it replaces (k_mlp_bwd3<W>, then k_mlp_trunk_fb) and sequences them
// with the dfeat_ready event and the slab sum.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "interp_fuse.h"
#include "mlp128_chain16.h"
#include "mlp128_trunk_fb.h"
#include "psvo_common.h"

namespace psvo {
namespace {

// slabs_b (or null): k_mlp_trunk_fb's slabs (the same layout), whose W1, W2, W3
// row 0 and b3[0] elements are added (the rest of its slabs is not written).
// A workgroup sums 64 elements: wave k over the k-th quarter of the slabs
// (batches of 8 independent loads, lane = element: 256-B rows), then the
// quarters in order — a fixed order, so deterministic.  (One thread per
// element over all 2 × 256 slabs left ≈ 150 workgroups on 256 CUs, each
// thread with up to 512 loads in flight one batch at a time: 132 µs.)
constexpr int kDwRedEl = 64;
__device__ __forceinline__ float dw_sum_range(const float *__restrict__ p, int64_t stride, int b, int e) {
    float v = 0.0f;
    int sp = b;
    for (; sp + 8 <= e; sp += 8) {
        float q[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) q[u] = p[(sp + u) * stride];
#pragma unroll
        for (int u = 0; u < 8; ++u) v += q[u];
    }
    for (; sp < e; ++sp) v += p[sp * stride];
    return v;
}
//
// cnt (or null; then no slabs_b): the slabs are the one-launch backward's
// (k_mlp_bwd3<W, H2>), whose workgroups [0, nA) are class A's and [nA, G) class
// B's, nA = bwd_split_na of the two counts as in that kernel: the elements
// k_mlp_trunk_fb writes are summed over all G slabs, every other element over
// the first nA only (a class-B slab's are not written and never read; nA = 0:
// exact zeros) — quarters of that range, in order.
__global__ __launch_bounds__(256) void k_mlp_dw_reduce(DwGrid g, const float *__restrict__ slabs, DwDst dst,
                                                       int accumulate, const float *__restrict__ slabs_b,
                                                       const int *__restrict__ cnt, const int *__restrict__ cnt_b,
                                                       BwdSplitCost cost) {
    __shared__ float part[4][kDwRedEl];
    const int lane = threadIdx.x & 63, k = threadIdx.x >> 6;
    const int e = blockIdx.x * kDwRedEl + lane;
    const bool in = e < dst.elem_begin[5];
    int L = 0;
#pragma unroll
    for (int l = 1; l < 5; ++l) L += (e >= dst.elem_begin[l]);
    const int rel = in ? e - dst.elem_begin[L] : 0;
    const bool trunk_el = L < 2 || (L == 2 && (rel < 128 || rel == 129 * 128));  // k_mlp_trunk_fb's elements
    int n_split = g.n_split[L];
    if (cnt) {
        const int64_t m_a = __builtin_amdgcn_readfirstlane(*cnt), m_b = __builtin_amdgcn_readfirstlane(*cnt_b);
        const int n_a = bwd_split_na((m_a + kU - 1) / kU, (m_b + kU - 1) / kU, n_split, cost);
        if (!trunk_el) n_split = n_a;
    }
    const int64_t stride = g.slab_len[L];
    const int b = n_split * k / 4, en = n_split * (k + 1) / 4;
    float v = 0.0f;
    if (in) {
        v = dw_sum_range(slabs + g.slab_off[L] + rel, stride, b, en);
        if (slabs_b && trunk_el) v += dw_sum_range(slabs_b + g.slab_off[L] + rel, stride, b, en);
    }
    part[k][lane] = v;
    __syncthreads();
    if (k != 0 || !in) return;
    v = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
    const int nw = dst.rows[L] * dst.cols[L];
    float *out = rel < nw ? dst.w[L] + rel : dst.b[L] + (rel - nw);
    *out = accumulate ? *out + v : v;
}

struct BwdIn16 {
    uint64_t mk[3];  // the forward's mask words of lane-half q & 1
    float y[3], g[3], gs;
    float4 x;        // x features 4q .. 4q + 3
};

__device__ __forceinline__ void load_bwd_in16(const float *__restrict__ rgb_in, const uint64_t *__restrict__ masks,
                                              const float *__restrict__ g_sdf, const float *__restrict__ g_rgb,
                                              const float *__restrict__ feat, int64_t s, bool valid, int q,
                                              BwdIn16 &in, const int *__restrict__ x_src = nullptr) {
    const int64_t sv = valid ? s : 0;
    const uint64_t *mk = masks + (sv * 2 + (q & 1)) * 3;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        in.mk[i] = mk[i];
        in.y[i] = rgb_in[sv * 3 + i];
        in.g[i] = g_rgb[sv * 3 + i];
    }
    in.gs = g_sdf[sv];
    const int64_t xr = x_src ? (int64_t)x_src[sv] : sv;  // x_src: the sample's feature row (no compact copy)
    in.x = *reinterpret_cast<const float4 *>(feat + xr * kIn + 4 * q);
}

struct Bwd3Src {
    const float *rgb, *g_sdf, *g_rgb, *feat;
    const uint64_t *masks;
    const float *act;  // CF [h1 | h2 | f | c1]
    float *dfeat;
    const int *x_src;  // or null: sample s's x is row x_src[s] of feat
};

// ---------------------------------------------------------------------------
// Fused backward: the δ chain AND the weight gradients in one persistent
// kernel, the δ's handed from the chain to the weight-gradient MFMAs through
// LDS instead of HBM (as separate kernels they moved 2 KB/sample of δ's out
// and back: ≈ 1.1 GB per step at config B).
//
// The chain needs features on the MFMA reduction axis (accumulator = next B
// operand, lane = sample); a weight gradient Σ_s δ[o][s] a[i][s] needs the
// samples there (lane = feature).  So every δ crosses lanes once: the chain
// wave writes its δ tile into LDS and the gradient MFMAs read it back
// transposed.  The chain runs v_mfma_f32_16x16x4_f32 on 16-sample units
// (an activation is 8 blocks × 4 = 32 registers, half of the 32-sample
// 32x32x2 form's 64 — the register file has to hold the weight-gradient
// accumulators too), lane (n, q) holding features 16·ob + 4q + j of sample n
// (j = register); its weights stream from L2 as MFMA A operands (Wᵀ images
// kImgC4..kImgC1, every CU reads the same 213 KB).
//
// One 8-wave workgroup per CU loops over rounds of four 16-sample units.
// Waves 0-3 (one per SIMD) run the chain of one unit each and own the
// gradients whose other operand is x or c1: W1 and the x columns of W4 (row
// block = wave), W5 (column block = wave); waves 4-7 (one per SIMD) own
// column block d = wave − 4 of W2, W3 and W4 (4 row blocks each, 192
// accumulator registers) and the biases of row block d.  A round is four
// phases separated by one barrier; a phase's exports are read in the next:
//   phase  chain wave c (unit u0 + 4r + c)                       gradient waves (the round's 4 units)
//   P0     δ5, δc1, x → LDS; δ[f; x] = W4ᵀ δc1; dW1 += δh1(r−1) ⊗ x
//   P1     δf, δsdf → LDS; δh2 = (W3ᵀ [δsdf; δf]) ⊙ m2;          dW4 += δc1 ⊗ f
//          dW4x += δc1 ⊗ x
//   P2     δh2 → LDS; δh1 = W2ᵀ δh2 ⊙ m1; dW5 += δ5 ⊗ c1         dW3 += [δsdf; δf] ⊗ h2
//   P3     δh1 → LDS; dfeat = W1ᵀ δh1 + δx_c (+ interp bwd)       dW2 += δh2 ⊗ h1
// plus a last P0 for the final round's dW1.  Per accumulator the MFMA
// order is fixed (rounds, units, k-steps in order): deterministic.  Each
// workgroup writes one slab of every layer; k_mlp_dw_reduce sums them.
//
// W = false (frozen decoder: dfeat only, e.g. tracking): all 8 waves run the
// chain (8 units per round), no exports, no gradients — the same chain
// arithmetic, so dfeat is bit-identical to the training call's.
//
// With ip.gx set (W only; the mapping engine) the chain wave also runs the
// interpolation backward of its unit in P3, right after dfeat (which is then
// not stored): the samples' leaf / ray / vertex rows load during P2, the 8
// embedding rows at the start of P3 (beside the W1ᵀ GEMM), then dL/dx per
// sample (ip.gx, summed per ray by k_interp_rays_gx) and the embedding
// scatter, summed over each leaf run of the unit first (k_interp_bwd's
// scheme: lanes own (corner, dim), whole 64-B rows per atomic instruction).
//
// The body is a device function of its workgroup's place: workgroup `wg` of
// the `n_wg` that share the m samples, writing slab `b` (k_mlp_bwd3<W> below:
// the whole grid; k_mlp_bwd3<W, H2>: the grid's class-A part).
template <bool W>
__device__ __forceinline__ void mlp_bwd3_body(const unsigned wg, const unsigned n_wg, const int b, const int64_t m,
                                              const float *__restrict__ img, const Bwd3Src &src, const DwGrid &g,
                                              float *__restrict__ slabs, const InterpFuse &ip) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t n_tiles = (m + kCh - 1) / kCh * 2;  // CF tiles (32 samples)
    const int64_t tstride = n_tiles * kCfTile;
    const int64_t tb = tstride * 4;
    const int64_t n_units = (m + kU - 1) / kU;
    const int64_t u0 = n_units * wg / n_wg, u1 = n_units * (wg + 1) / n_wg;
    constexpr int kPer = W ? 4 : 8;  // units per round
    const int n_rounds = (int)((u1 - u0 + kPer - 1) / kPer);
    float *const slot = lds + kB3Slot, *const small = lds + kB3Small, *const xim = lds + kB3X;
    auto dset = [&](int s) { return slot + s * 4 * kUImg; };
    // the chain's 4 exports per round alternate over 2 sets (export e = 4r + phase → set e mod 2):
    // each is read in the phase after its write, the next write to its set is a phase later
    auto eset = [&](int e) { return dset(((e % 2) + 2) % 2); };
    auto sset = [&](int s) { return small + s * 4 * 4 * kU; };
    auto xset = [&](int par) { return xim + par * 4 * 16 * kU; };
    stage8(lds, img + kImgVec, kVecPad, wave, lane);
    wait_vm(0);
    raw_barrier();
    const int i = lane & 31, h = lane >> 5;
    if (!W || wave < 4) {
        // ================= chain wave c
        const __amdgpu_buffer_rsrc_t wrs = rsrc_of(img, (int64_t)kImgTotal * 4);
        const int c = wave;
        const int n = lane & 15, q = lane >> 4;
        const int sn = (n & 1) * 8 + (n >> 1);                     // the sample's slot
        const int wb = 64 * q + ((((sn >> 2) ^ q) << 2) | (sn & 3));  // + 256 ob + 16 j
        float *const page1 = lds + kB3A + c * 2048, *const page4x = page1 + 1024;  // dW1, dW4x accumulators
        if (W) {
#pragma unroll
            for (int k = 0; k < 8; ++k)
                *reinterpret_cast<float4 *>(page1 + (k * 64 + lane) * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        float b1p = 0.f;
        BwdIn16 nin;
        {
            const int64_t u = u0 + c;
            const int64_t s = u * kU + n;
            load_bwd_in16(src.rgb, src.masks, src.g_sdf, src.g_rgb, src.feat, s, u < u1 && s < m, q, nin, src.x_src);
        }
        [[maybe_unused]] constexpr int kStampK = 1;
        PSVO_STAMP_DECL;
        for (int r = 0; r <= n_rounds; ++r) {
            PSVO_STAMP(0);
            const int64_t ubase = u0 + kPer * (int64_t)r;
            const int64_t u = ubase + c;
            const bool active = r < n_rounds && u < u1;  // wave-uniform
            const int64_t s = u * kU + n;
            const bool valid = active && s < m;
            // ---- P0: δ5 / δc1 / x → LDS; δ[f; x] = W4ᵀ δc1; dW1 of the previous round
            f32x4v fa[8], fb[8], dxc[1];
            float dsdf = 0.f;
            uint64_t m1 = 0, m2 = 0;
            if (r < n_rounds) {
                const BwdIn16 in = nin;
                float d5[3];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch)  // roundings spelled out: both instantiations give the same bits
                    d5[ch] = valid ? __fmul_rn(in.g[ch], __fmul_rn(in.y[ch], __fsub_rn(1.0f, in.y[ch]))) : 0.0f;
                dsdf = valid ? in.gs : 0.0f;
                const int sh = 4 * (q >> 1);
                m1 = valid ? in.mk[0] >> sh : 0;
                m2 = valid ? in.mk[1] >> sh : 0;
                const uint64_t m4 = valid ? in.mk[2] >> sh : 0;
                if (W) {
                    float *xl = xset(r & 1) + c * 16 * kU;
                    xl[wb + 0] = valid ? in.x.x : 0.f;
                    xl[wb + 16] = valid ? in.x.y : 0.f;
                    xl[wb + 32] = valid ? in.x.z : 0.f;
                    xl[wb + 48] = valid ? in.x.w : 0.f;
                }
                if (W && q == 0) {  // δ5: rows 0..2 of the round's small set (read by dW5 a round later)
                    float *sl = sset(r & 1) + c * 4 * kU;
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) sl[ch * kU + sn] = d5[ch];
                }
                if (active) {
#pragma unroll
                    for (int ob = 0; ob < 8; ++ob) {  // δc1 = W5ᵀ δ5 ⊙ mask
                        const int k = 16 * ob + 4 * q;
                        const float4 w0 = *reinterpret_cast<const float4 *>(lds + kOffW5 + k);
                        const float4 w1 = *reinterpret_cast<const float4 *>(lds + kOffW5 + 128 + k);
                        const float4 w2 = *reinterpret_cast<const float4 *>(lds + kOffW5 + 256 + k);
                        auto dot3 = [&](float a0, float a1, float a2) {
                            return fmaf(a2, d5[2], fmaf(a1, d5[1], __fmul_rn(a0, d5[0])));
                        };
                        fb[ob] = f32x4v{dot3(w0.x, w1.x, w2.x), dot3(w0.y, w1.y, w2.y), dot3(w0.z, w1.z, w2.z),
                                        dot3(w0.w, w1.w, w2.w)};
                    }
                    mask16(fb, m4);
                    if (W) lds_u_store<8>(eset(4 * r) + c * kUImg, wb, fb);
                    zero4(fa);
                    zero4(dxc);
                    gemm16<8, 4, 2>(wrs, kImgC4, fb, *reinterpret_cast<f32x4v(*)[4]>(&fa[0]), lane);  // δf
                    gemm16<8, 4, 2>(wrs, kImgC4 + 4 * 8 * 256, fb, *reinterpret_cast<f32x4v(*)[4]>(&fa[4]), lane);
                    gemm16<8, 1, 4>(wrs, kImgC4 + 8 * 8 * 256, fb, dxc, lane);  // δx_c
                }
            }
            if (W && r > 0) xgrad16(eset(4 * r - 1), xset((r - 1) & 1), c, ubase - 4, u1, lane, page1, &b1p);
            PSVO_STAMP(1);
            raw_barrier();
            PSVO_STAMP(2);
            if (r == n_rounds) break;
            // ---- P1: δf / δsdf → LDS; δh2 = W3ᵀ [δsdf; δf] ⊙ m2; dW4x, dW5
            if (W && q == 0) sset(r & 1)[c * 4 * kU + 3 * kU + sn] = dsdf;  // row 3
            if (active) {
                if (W) lds_u_store<8>(eset(4 * r + 1) + c * kUImg, wb, fa);
#pragma unroll
                for (int ob = 0; ob < 8; ++ob) {
                    const float4 w = *reinterpret_cast<const float4 *>(lds + kOffW3r0 + 16 * ob + 4 * q);
                    fb[ob] = f32x4v{__fmul_rn(w.x, dsdf), __fmul_rn(w.y, dsdf), __fmul_rn(w.z, dsdf), __fmul_rn(w.w, dsdf)};
                }
                gemm16<8, 4, 2>(wrs, kImgC3, fa, *reinterpret_cast<f32x4v(*)[4]>(&fb[0]), lane);
                gemm16<8, 4, 2>(wrs, kImgC3 + 4 * 8 * 256, fa, *reinterpret_cast<f32x4v(*)[4]>(&fb[4]), lane);
                mask16(fb, m2);  // δh2
            }
            if (W) {
                xgrad16(eset(4 * r), xset(r & 1), c, ubase, u1, lane, page4x, nullptr);
            }
            // the interpolation backward's sample data, one dependent level per phase
            const bool fuse = W && ip.gx != nullptr;  // uniform
            int lf = 0, ro = 0;
            float ts = 0.f;
            if (fuse && valid) {
                lf = ip.leaf[s];
                ro = ip.ray_of[s];
                ts = ip.t[s];
            }
            PSVO_STAMP(3);
            raw_barrier();
            PSVO_STAMP(4);
            // ---- P2: δh2 → LDS; δh1 = W2ᵀ δh2 ⊙ m1 (+ the interpolation backward's sample data)
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
            if (active) {
                if (W) lds_u_store<8>(eset(4 * r + 2) + c * kUImg, wb, fb);
                zero4(fa);
                gemm16<8, 4, 2>(wrs, kImgC2, fb, *reinterpret_cast<f32x4v(*)[4]>(&fa[0]), lane);
                gemm16<8, 4, 2>(wrs, kImgC2 + 4 * 8 * 256, fb, *reinterpret_cast<f32x4v(*)[4]>(&fa[4]), lane);
                mask16(fa, m1);  // δh1
            }
            float ro3[3] = {0.f, 0.f, 0.f}, rd3[3] = {0.f, 0.f, 0.f};
            float4 ev[8];
            if (fuse) {  // the 8 embedding rows (used in P3)
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
            }
            PSVO_STAMP(5);
            raw_barrier();
            PSVO_STAMP(6);
            // ---- P3: δh1 → LDS; dfeat = W1ᵀ δh1 + δx_c; the next unit's inputs
            if (W && active) lds_u_store<8>(eset(4 * r + 3) + c * kUImg, wb, fa);
            if (r + 1 < n_rounds) {
                const int64_t un = u + kPer;
                const int64_t snx = un * kU + n;
                load_bwd_in16(src.rgb, src.masks, src.g_sdf, src.g_rgb, src.feat, snx, un < u1 && snx < m, q, nin,
                              src.x_src);
            }
            if (active) {
                f32x4v t1[1];
                zero4(t1);
                gemm16<8, 1, 4>(wrs, kImgC1, fa, t1, lane);
                const float4 gf = make_float4(__fadd_rn(t1[0][0], dxc[0][0]), __fadd_rn(t1[0][1], dxc[0][1]),
                                              __fadd_rn(t1[0][2], dxc[0][2]), __fadd_rn(t1[0][3], dxc[0][3]));
                if (!fuse) {
                    if (valid) *reinterpret_cast<float4 *>(src.dfeat + s * kIn + 4 * q) = gf;
                } else {
                    interp_bwd_unit(ip, lds + kB3I + c * 512, m, s, valid, n, q, ts, ro3, rd3, cen, vid0, vid1, ev,
                                    gf);
                    if (ip.grad_emb != nullptr) {
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // the staging is this wave's own
                        __builtin_amdgcn_wave_barrier();
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                        scatter_unit(ip, lds + kB3I + c * 512, u, m, lane, lf);
                    }
                }
            }
            PSVO_STAMP(7);
            raw_barrier();
            PSVO_STAMP(8);
            PSVO_STAMP_FLUSH(1);
        }
        if (!W) return;
        // ---- slabs: W1 row block c + b1; W4's x columns of row block c; W5 column block c (+ b5)
        float *s1 = slabs + g.slab_off[0] + (int64_t)b * g.slab_len[0];
        float *s4 = slabs + g.slab_off[3] + (int64_t)b * g.slab_len[3];
        if (i < 16) {
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) {
                const int row = 32 * c + phi(rr, h);
                const int pos = ((rr >> 2) * 64 + lane) * 4 + (rr & 3);
                store_nt(s1, row * 16 + i, page1[pos]);
                store_nt(s4, row * 144 + 128 + i, page4x[pos]);
            }
        }
        const float bv = b1p + __shfl_xor(b1p, 32, 64);
        if (h == 0) store_nt(s1, 128 * 16 + 32 * c + i, bv);
    } else {
        // ================= gradient wave: column block d of W2 / W3 / W4, biases of row block d
        const int d = wave - 4;
        f32x16 acc2[kNB], acc3[kNB], acc4[kNB];
        zero(acc2);
        zero(acc3);
        zero(acc4);
        float b2p = 0.f, b3p = 0.f, b4p = 0.f, r0 = 0.f, b30 = 0.f, unused0 = 0.f, unused1 = 0.f;
        // dW5 / b5 partials live in LDS between rounds (registers are full with dW2..4)
        float *const page5 = lds + kB3W5 + d * 512 + lane * 8;
        *reinterpret_cast<float4 *>(page5) = make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4 *>(page5 + 4) = make_float4(0.f, 0.f, 0.f, 0.f);
        const __amdgpu_buffer_rsrc_t c1m = rsrc_of(src.act + 3 * tstride, tb);
        const __amdgpu_buffer_rsrc_t h1m = rsrc_of(src.act, tb), h2m = rsrc_of(src.act + tstride, tb),
                                     fm = rsrc_of(src.act + 2 * tstride, tb);
        [[maybe_unused]] constexpr int kStampK = 1;
        PSVO_STAMP_DECL;
        float4 ring[3];  // B operands, continuous across the jobs (see dw_job)
        ring[0] = dw_bsrc(fm, u0, u1, d, lane, 0);
        ring[1] = dw_bsrc(fm, u0, u1, d, lane, 1);
        for (int r = 0; r <= n_rounds; ++r) {
            const int64_t ubase = u0 + 4 * (int64_t)r;
            PSVO_STAMP(0);
            // P0: dW5 of the previous round (δ5 in its small set), beside the chain's W4ᵀ and dW1
            if (r > 0) {
                float w5[3] = {0.f, 0.f, 0.f}, b5[3] = {0.f, 0.f, 0.f};
                w5_grad(sset((r - 1) & 1), c1m, d, ubase - 4, u1, lane, w5, b5);
                float4 p0 = *reinterpret_cast<float4 *>(page5), p1 = *reinterpret_cast<float4 *>(page5 + 4);
                p0.x += w5[0]; p0.y += w5[1]; p0.z += w5[2];
                p1.x += b5[0]; p1.y += b5[1]; p1.z += b5[2];
                *reinterpret_cast<float4 *>(page5) = p0;
                *reinterpret_cast<float4 *>(page5 + 4) = p1;
            }
            PSVO_STAMP(1);
            raw_barrier();
            PSVO_STAMP(2);
            if (r == n_rounds) break;
            // P1: dW4 (δc1: export 0)
            dw_job<0, 0>(ring, eset(4 * r), nullptr, fm, ubase, true, h2m, ubase, true, u1, d, lane, acc4, b4p,
                         unused0, unused1);
            PSVO_STAMP(3);
            raw_barrier();
            PSVO_STAMP(4);
            // P2: dW3 (δf, δsdf: export 1)
            dw_job<2, 2>(ring, eset(4 * r + 1), sset(r & 1) + 3 * kU, h2m, ubase, true, h1m, ubase, true, u1, d, lane, acc3, b3p,
                         r0, b30);
            PSVO_STAMP(5);
            raw_barrier();
            PSVO_STAMP(6);
            // P3: dW2 (δh2: export 2), beside the chain's W1ᵀ and interpolation backward
            dw_job<0, 1>(ring, eset(4 * r + 2), nullptr, h1m, ubase, true, fm, ubase + 4, r + 1 < n_rounds, u1, d,
                         lane, acc2, b2p, unused0, unused1);
            PSVO_STAMP(7);
            raw_barrier();
            PSVO_STAMP(8);
            PSVO_STAMP_FLUSH(1);
        }
        const int rb[kNB] = {0, 1, 2, 3}, cb[1] = {d};
        float *s2 = slabs + g.slab_off[1] + (int64_t)b * g.slab_len[1];
        float *s3 = slabs + g.slab_off[2] + (int64_t)b * g.slab_len[2];
        float *s4 = slabs + g.slab_off[3] + (int64_t)b * g.slab_len[3];
        {
            f32x16 t[kNB][1];
#pragma unroll
            for (int k = 0; k < kNB; ++k) t[k][0] = acc2[k];
            dw_store<kNB, 1, true>(s2, 128, 0, 128, rb, cb, t, lane);
#pragma unroll
            for (int k = 0; k < kNB; ++k) t[k][0] = acc3[k];
            dw_store<kNB, 1, true>(s3, 128, 1, 128, rb, cb, t, lane);
#pragma unroll
            for (int k = 0; k < kNB; ++k) t[k][0] = acc4[k];
            dw_store<kNB, 1, true>(s4, 144, 0, 144, rb, cb, t, lane);
        }
        const float v2 = b2p + __shfl_xor(b2p, 32, 64), v3 = b3p + __shfl_xor(b3p, 32, 64),
                    v4 = b4p + __shfl_xor(b4p, 32, 64), vr0 = r0 + __shfl_xor(r0, 32, 64),
                    v30 = b30 + __shfl_xor(b30, 32, 64);
        if (h == 0) {
            store_nt(s2, 128 * 128 + 32 * d + i, v2);
            store_nt(s3, 129 * 128 + 1 + 32 * d + i, v3);
            store_nt(s4, 128 * 144 + 32 * d + i, v4);
            store_nt(s3, 32 * d + i, vr0);  // W3 row 0 (sdf)
        }
        if (d == 0 && lane == 0) store_nt(s3, 129 * 128, v30);
        // W5 column block d (+ b5)
        float *s5 = slabs + g.slab_off[4] + (int64_t)b * g.slab_len[4];
        const float4 p0 = *reinterpret_cast<const float4 *>(page5), p1 = *reinterpret_cast<const float4 *>(page5 + 4);
        const float w5[3] = {p0.x, p0.y, p0.z}, b5[3] = {p1.x, p1.y, p1.z};
        float v5[3], t5[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            v5[ch] = w5[ch] + __shfl_xor(w5[ch], 32, 64);
            t5[ch] = b5[ch] + __shfl_xor(b5[ch], 32, 64);  // every lane of a half holds its half's Σ δ5
        }
        if (h == 0) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) store_nt(s5, ch * 128 + 32 * d + i, v5[ch]);
        }
        if (d == 0 && lane == 0) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) store_nt(s5, 3 * 128 + ch, t5[ch]);
        }
    }
}

template <bool W>
__global__ __launch_bounds__(kF2Threads, 1) void k_mlp_bwd3(int64_t m, const float *__restrict__ img, Bwd3Src src,
                                                            DwGrid g, float *__restrict__ slabs, InterpFuse ip,
                                                            const int *__restrict__ m_dev) {
    if (m_dev) m = __builtin_amdgcn_readfirstlane(*m_dev);  // the sparse decoder's kept samples (<= m)
    mlp_bwd3_body<W>(blockIdx.x, gridDim.x, blockIdx.x, m, img, src, g, slabs, ip);
}

// ---------------------------------------------------------------------------
// Both sample classes of the sparse decoder in ONE launch: workgroups
// [0, nA) run k_mlp_bwd3<true>'s body over nA shares of class A's units,
// workgroups [nA, G) run k_mlp_trunk_fb<H2>'s body over G − nA shares of class
// B's, nA = bwd_split_na of the two device counts (psvo_common.h: the modelled
// finish times meet).  As two launches each class quantised on its own over
// all G workgroups (8 rounds of 7,875 units, then 3 of 2,750 with the trunk
// kernel's fixed cost on the critical path) and the chip waited for both
// tails at a kernel boundary.  Nothing passes between workgroups and none
// waits for another: the result does not depend on the dispatch order, only
// the balance assumes one workgroup per CU (as the two kernels do).  Workgroup
// b writes slab b of ONE slab set: a class-B workgroup only the elements
// k_mlp_trunk_fb writes — k_mlp_dw_reduce (n_a) reads no others of it.
struct TrunkSrc {
    const int *m_dev;
    const float *g_sdf, *feat, *h2;
    const int *h2_src;
};
template <bool W, bool H2>
__global__ __launch_bounds__(kF2Threads, 1) void k_mlp_bwd3(int64_t m, const float *__restrict__ img, Bwd3Src src,
                                                            DwGrid g, float *__restrict__ slabs, InterpFuse ip,
                                                            const int *__restrict__ m_dev, TrunkSrc tk,
                                                            InterpFuse ip_b, BwdSplitCost cost) {
    static_assert(W, "the two-class launch is a training launch");
    const int n_wg = gridDim.x, b = blockIdx.x;
    if (m_dev) m = __builtin_amdgcn_readfirstlane(*m_dev);
    const int64_t m_b = __builtin_amdgcn_readfirstlane(*tk.m_dev);
    const int n_a = bwd_split_na((m + kU - 1) / kU, (m_b + kU - 1) / kU, n_wg, cost);
    if (b < n_a)
        mlp_bwd3_body<true>(b, n_a, b, m, img, src, g, slabs, ip);
    else
        mlp_trunk_fb_body<H2>(b - n_a, n_wg - n_a, b, m_b, img, tk.g_sdf, tk.feat, g, slabs, ip_b, tk.h2, tk.h2_src);
}

// k_mlp_bwd3: one workgroup per CU (at most one per round of 4 units), each
// writing a slab of every layer
int bwd3_grid(int64_t m) {
    const int64_t rounds = (m + 4 * kU - 1) / (4 * kU);
    return persistent_grid(rounds > 0 ? rounds : 1);
}
constexpr int kDwRows[5] = {128, 128, 129, 128, 3};
constexpr int kDwCols[5] = {16, 128, 128, 144, 128};
void dw_grid_uniform(int n, DwGrid *g, int *slab_floats) {
    int off = 0;
    for (int l = 0; l < 5; ++l) {
        g->n_split[l] = n;
        g->slab_off[l] = off;
        g->slab_len[l] = kDwRows[l] * kDwCols[l] + kDwRows[l];
        off += n * g->slab_len[l];
    }
    *slab_floats = off;
}

}  // namespace

int64_t dec128_workspace_floats(int64_t m) {
    DwGrid g;
    int slab;
    dw_grid_uniform(bwd3_grid(m), &g, &slab);
    return m * 3 + 2 * (int64_t)slab;  // k_mlp_bwd3's slabs, then k_mlp_trunk_fb's (the sparse decoder's class B)
}

// Full decoder backward: grads of the 10 parameters (overwritten, or added
// to when `accumulate`) and dfeat [M,16], from the training forward's rgb,
// activations and masks.  `workspace`: 3 m floats, then the slabs
// (psvo_mlp_workspace_floats).
int dec128_bwd(hipStream_t st, int64_t m, const float *feat, const float *images, const float *rgb, const float *act,
               const uint64_t *masks, const float *g_sdf, const float *g_rgb, float *dfeat, float *const gw[5],
               float *const gb[5], int accumulate, int n_split, float *workspace, hipEvent_t dfeat_ready,
               const InterpFuse *ip, hipStream_t reduce_stream, const int *m_dev, const TrunkBwd *tb,
               const int *x_src) {
    PSVO_REQUIRE(m >= 0 && n_split > 0, "mlp_bwd: bad sizes");
    PSVO_REQUIRE(images != nullptr, "mlp_bwd: images of the training forward required");
    const bool want_w = gw[0] != nullptr;  // NULL weight gradients: δ chain / dfeat only (frozen decoder)
    PSVO_REQUIRE(!want_w || act != nullptr, "mlp_bwd: weight gradients need the forward's activations");
    DwGrid g;
    int slab_floats;
    PSVO_REQUIRE(tb == nullptr || (gw[0] != nullptr && tb->m_dev && tb->g_sdf && tb->feat),
                 "mlp_bwd: the trunk backward needs the weight-gradient path and its inputs");
    float *slabs_b = nullptr;
    const int *cnt_a = nullptr, *cnt_b = nullptr;  // set: the one-launch backward's slabs
    const BwdSplitCost cost = bwd_split_cost();
    auto reduce = [&](float *slabs, hipStream_t rs) {
        DwDst d;
        int e = 0;
        for (int l = 0; l < 5; ++l) {
            d.w[l] = gw[l];
            d.b[l] = gb[l];
            d.rows[l] = kDwRows[l];
            d.cols[l] = kDwCols[l];
            d.elem_begin[l] = e;
            e += kDwRows[l] * kDwCols[l] + kDwRows[l];
        }
        d.elem_begin[5] = e;
        psvo::launch(k_mlp_dw_reduce, dim3(div_up(e, kDwRedEl)), dim3(256), 0, rs, g, slabs, d, accumulate,
                     static_cast<const float *>(slabs_b), cnt_a, cnt_b, cost);
        return check_launch("mlp_dw_reduce");
    };
    Bwd3Src src{rgb, g_sdf, g_rgb, feat, masks, act, dfeat, x_src};
    if (!want_w) {
        if (m > 0) {
            launch_lds<k_mlp_bwd3<false>>(dim3(persistent_grid(div_up(div_up(m, kU), 8))), dim3(kF2Threads), kLdsBwd3,
                                          st, m, images, src, g, nullptr, InterpFuse{}, m_dev);
            const int rc = check_launch("mlp_bwd3");
            if (rc) return rc;
        }
        if (dfeat_ready && hipEventRecord(dfeat_ready, st) != hipSuccess)
            return set_error(PSVO_E_LAUNCH, "mlp_bwd: event record failed");
        return PSVO_OK;
    }
    const int grid = bwd3_grid(m);
    dw_grid_uniform(grid, &g, &slab_floats);
    float *slabs = workspace + m * 3;
    // dfeat_ready marks the last kernel's completion through its dispatch
    // (psvo::launch's stop event): no marker packet between the decoder's
    // backward and the per-ray sums that follow it on st
    static const bool bind_env = [] {
        const char *v = getenv("PSVO_BIND_DFEAT");
        return !(v && v[0] == '0');
    }();
    const bool trunk_last = tb && m > 0;
    bool bound = false;
    const hipEvent_t bind_ev = bind_env ? dfeat_ready : nullptr;  // offered to the last kernel only
    // both classes in one launch (k_mlp_bwd3<W, H2>); two launches: no split of one workgroup, the
    // count on the host only, or asked for (PSVO_PATH_BWD_TWO_LAUNCH)
    const bool one_launch = trunk_last && grid >= 2 && m_dev && !tb->two_launch;
    if (one_launch) {
        PSVO_REQUIRE(!tb->h2 || tb->src, "mlp_bwd: the trunk's h2 rows need their source index");
        cnt_a = m_dev;
        cnt_b = tb->m_dev;
        const TrunkSrc tk{tb->m_dev, tb->g_sdf, tb->feat, tb->h2, tb->src};
        const InterpFuse ip_a = ip ? *ip : InterpFuse{}, ip_b = tb->ip ? *tb->ip : InterpFuse{};
        constexpr int kLdsAb = kLdsBwd3 > kLdsTrunk ? kLdsBwd3 : kLdsTrunk;
        psvo::StopBind sb(bind_ev);
        if (tb->h2)
            launch_lds<k_mlp_bwd3<true, true>>(dim3(grid), dim3(kF2Threads), kLdsAb, st, m, images, src, g, slabs,
                                               ip_a, m_dev, tk, ip_b, cost);
        else
            launch_lds<k_mlp_bwd3<true, false>>(dim3(grid), dim3(kF2Threads), kLdsAb, st, m, images, src, g, slabs,
                                                ip_a, m_dev, tk, ip_b, cost);
        bound = sb.consumed();
        const int rc = check_launch("mlp_bwd3 (both classes)");
        if (rc) return rc;
    } else if (m > 0) {
        psvo::StopBind sb(trunk_last ? nullptr : bind_ev);
        launch_lds<k_mlp_bwd3<true>>(dim3(grid), dim3(kF2Threads), kLdsBwd3, st, m, images, src, g, slabs,
                                     ip ? *ip : InterpFuse{}, m_dev);
        bound = sb.consumed();
        const int rc = check_launch("mlp_bwd3");
        if (rc) return rc;
    } else if (hipMemsetAsync(slabs, 0, (size_t)slab_floats * sizeof(float), st) != hipSuccess) {
        return set_error(PSVO_E_LAUNCH, "mlp_bwd: memset failed");
    }
    if (trunk_last && !one_launch) {  // the sparse decoder's class B: the trunk forward + backward, its own slabs
        slabs_b = slabs + slab_floats;
        PSVO_REQUIRE(!tb->h2 || tb->src, "mlp_bwd: the trunk's h2 rows need their source index");
        psvo::StopBind sb(bind_ev);
        launch_trunk_fb(st, grid, images, *tb, g, slabs_b);
        bound = sb.consumed();
        const int rc = check_launch("mlp_trunk_fb");
        if (rc) return rc;
    }
    if (dfeat_ready && !bound && hipEventRecord(dfeat_ready, st) != hipSuccess)
        return set_error(PSVO_E_LAUNCH, "mlp_bwd: event record failed");
    if (reduce_stream && reduce_stream != st) {  // the slab sum beside the caller's next work on st
        PSVO_REQUIRE(dfeat_ready != nullptr, "mlp_bwd: a separate reduce stream needs the dfeat_ready event");
        if (hipStreamWaitEvent(reduce_stream, dfeat_ready, 0) != hipSuccess)
            return set_error(PSVO_E_LAUNCH, "mlp_bwd: stream wait failed");
        return reduce(slabs, reduce_stream);
    }
    return reduce(slabs, st);
}

}  // namespace psvo
