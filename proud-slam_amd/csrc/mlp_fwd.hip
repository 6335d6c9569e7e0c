// Width-128 decoder, forward (mlp128.h: the layer equations and layouts):
//   k_mlp_prep   every layer's operand image, once per weight update
//   k_mlp_fwd2   the whole forward, persistent and double-buffered; for
//                training it also stores the CF activations and ReLU masks
//   k_mlp_sdf2   h1, h2 and the sdf row of W3 only (the same sdf bits)
// and their launchers: dec128_fwd (psvo_common.h) and the two forwards that
// interpolate their own features (interp_load.h).
#include <hip/hip_runtime.h>

#include "interp_load.h"
#include "mlp128_chain32.h"
#include "psvo_common.h"

namespace psvo {
namespace {

__device__ __forceinline__ void inv_perm_acc(int pos, int nkb, int &i, int &k) {
    const int c = pos & 3, lane = (pos >> 2) & 63, rest = pos >> 8;
    const int rg = rest & 3, blk = rest >> 2;
    const int kb = blk % nkb, ib = blk / nkb;
    const int h = lane >> 5;
    i = ib * 32 + (lane & 31);
    k = kb * 32 + c + 4 * h + 8 * rg;
}
__device__ __forceinline__ void inv_perm_x(int pos, int &i, int &k) {
    const int c = pos & 3, lane = (pos >> 2) & 63, rest = pos >> 8;
    const int tg = rest & 1, ib = rest >> 1;
    i = ib * 32 + (lane & 31);
    k = 2 * (tg * 4 + c) + (lane >> 5);
}

struct MlpParams {
    const float *w1, *b1, *w2, *b2, *w3, *b3, *w4, *b4, *w5, *b5;
};

// element e (< kVecPad) of the vector image = LDS float e of the kOff* carve
__device__ __forceinline__ float vec_elem(const MlpParams &p, int e) {
    if (e < kOffB2) return p.b1[e - kOffB1];
    if (e < kOffB3) return p.b2[e - kOffB2];
    if (e < kOffB4) return e - kOffB3 < 129 ? p.b3[e - kOffB3] : 0.0f;
    if (e < kOffB5) return p.b4[e - kOffB4];
    if (e < kOffW3r0) return e - kOffB5 < 3 ? p.b5[e - kOffB5] : 0.0f;
    if (e < kOffW5) return p.w3[e - kOffW3r0];
    if (e < kOffW) return p.w5[e - kOffW5];
    return 0.0f;
}

__global__ __launch_bounds__(256) void k_mlp_prep(MlpParams p, float *__restrict__ img) {
    const float *w1 = p.w1, *w2 = p.w2, *w3 = p.w3, *w4 = p.w4;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= kImgTotal) return;
    int i, k;
    float v = 0.0f;
    if (e >= kImgT1) {  // the trunk kernel's forward images: W[o][in], [ob][kb][lane (m, q)][4]
        const bool t1 = e < kImgT2;
        const int pos = e - (t1 ? kImgT1 : kImgT2);
        const int j = pos & 3, ln = (pos >> 2) & 63, blk = pos >> 8;
        const int nkb = t1 ? 1 : 8;
        const int o = 16 * (blk / nkb) + (ln & 15), in = 16 * (blk % nkb) + 4 * (ln >> 4) + j;
        img[e] = t1 ? p.w1[o * 16 + in] : w2[o * 128 + in];
        return;
    }
    if (e >= kImgC4) {  // chain16 images: [ob][kb][lane (m, q)][4]
        const int sec = e < kImgC3 ? 4 : e < kImgC2 ? 3 : e < kImgC1 ? 2 : 1;
        const int pos = e - (sec == 4 ? kImgC4 : sec == 3 ? kImgC3 : sec == 2 ? kImgC2 : kImgC1);
        const int j = pos & 3, ln = (pos >> 2) & 63, blk = pos >> 8;
        const int o = 16 * (blk >> 3) + (ln & 15), in = 16 * (blk & 7) + 4 * (ln >> 4) + j;  // Wᵀ[o][in]
        img[e] = sec == 4 ? w4[in * 144 + o] : sec == 3 ? w3[(1 + in) * 128 + o] : sec == 2 ? w2[in * 128 + o]
                                                                                             : p.w1[in * 16 + o];
        return;
    }
    if (e >= kImgVec) {
        img[e] = vec_elem(p, e - kImgVec);
        return;
    }
    if (e < kImgF2) {
        inv_perm_x(e - kImgF1, i, k);
        v = w1[i * 16 + k];
    } else if (e < kImgF3) {
        inv_perm_acc(e - kImgF2, 4, i, k);
        v = w2[i * 128 + k];
    } else if (e < kImgF4) {
        inv_perm_acc(e - kImgF3, 4, i, k);
        v = w3[(i + 1) * 128 + k];
    } else {
        const int pos = e - kImgF4;
        if (pos < 16384) {
            inv_perm_acc(pos, 4, i, k);
            v = w4[i * 144 + k];
        } else {
            inv_perm_x(pos - 16384, i, k);
            v = w4[i * 144 + 128 + k];
        }
    }
    img[e] = v;
}

// ---------------------------------------------------------------------------
// forward, persistent + double-buffered: one 512-thread workgroup per CU
// loops over 256-sample tiles (8 waves × 32 samples, each wave its own
// chain).  The vectors and W1 stay resident in LDS; W2, W3, W4 stream
// through two 72-KB buffers with global_load_lds issued one layer ahead
// (W2 of the next tile during W4 of this one), so no wave waits for weight
// staging; each layer's activation stores are issued after the barrier that
// opens the next layer and drain behind its MFMAs.  LDS: 5 + 8 + 2 × 72 KB.
//
// IP (the frame renderer, csrc/render.hip): x is interpolated on chip from
// `ip` (interp_load.h) instead of read from feat; inference only — no masks
// are stored, so none are formed (relu_values: the same activations)
template <bool H2, bool IP = false>
__global__ __launch_bounds__(kF2Threads, 1) void k_mlp_fwd2(int64_t m, const float *__restrict__ feat,
                                                            const float *__restrict__ img,
                                                            float *__restrict__ sdf_out, float *__restrict__ rgb_out,
                                                            float *__restrict__ act, uint64_t *__restrict__ masks,
                                                            const int *__restrict__ m_dev,
                                                            const float *__restrict__ h2_rows,
                                                            const int *__restrict__ h2_src, InterpSrc ip) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    static_assert(!(H2 && IP), "the h2 hand-over reads the step's feature rows");
    if (m_dev) m = __builtin_amdgcn_readfirstlane(*m_dev);  // the sparse decoder's kept samples (<= m)
    // h2_rows: h2 of every sample of the step (k_mlp_sdf2's, the same
    // instructions: the same bits), sample s's row h2_src[s] — the W2 layer
    // is read instead of recomputed (W3 / W4 stream through the buffers)
    constexpr bool h2_given = H2;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = lane >> 5;
    const bool save = act != nullptr;         // CF activations (weight gradients)
    constexpr bool kMask = !IP;               // the ReLUs form their masks
    const bool save_mask = kMask && masks != nullptr;  // ReLU masks (δ chain)
    const int64_t n_tiles = (m + kCh - 1) / kCh * 2;  // CF 32-sample tiles
    const int64_t tstride = n_tiles * 32 * 128;
    const int64_t tbytes = tstride * 4;
    // Balanced split: workgroup b owns the 32-sample units [u0, u1), so every
    // wave slot gets floor or ceil of n_units / (8 · grid) and the last
    // iteration is a partial one (waves past u1 skip their MFMAs but keep the
    // staging and barriers) instead of a whole extra 256-sample round on a
    // few CUs while the rest of the chip waits at the kernel boundary.
    const int64_t n_units = (m + kTileS - 1) / kTileS;
    const int64_t u0 = n_units * blockIdx.x / gridDim.x, u1 = n_units * (blockIdx.x + 1) / gridDim.x;
    const int n_it = (int)((u1 - u0 + kF2Waves - 1) / kF2Waves);
    auto buf = [&](int i) { return lds + ((i & 1) ? kF2Buf1 : kF2Buf0); };
    int seq = 0;  // staged layers so far: W(seq) sits in buf(seq)
    float xn[8];
    int srcn = 0;
    {
        const int64_t u = u0 + wave;
        const int64_t s = u * kTileS + (lane & 31);
        if (h2_given && u < u1 && s < m) srcn = h2_src[s];
        if constexpr (IP)
            iload::load_x_interp(ip, s, u < u1 && s < m, h, xn);
        else
            load_x(feat, h2_given ? (int64_t)srcn : s, u < u1 && s < m, h, xn);  // (h2 given: feat is the step's rows)
    }
    stage8(lds, img + kImgVec, kVecPad, wave, lane);
    stage8(lds + kF2W1, img + kImgF1, 2048, wave, lane);
    stage8(buf(0), img + (h2_given ? kImgF3 : kImgF2), 16384, wave, lane);
    wait_vm(0);
    raw_barrier();
    [[maybe_unused]] constexpr int kStampK = 0;
    PSVO_STAMP_DECL;
    for (int it = 0; it < n_it; ++it) {
        if (!H2) PSVO_STAMP(0);  // (the h2-reading instantiation: no stamps — the diagnostic build hit a backend error there)
        const int64_t u = u0 + (int64_t)it * kF2Waves + wave;
        const bool active = u < u1;  // wave-uniform
        const int64_t s = u * kTileS + (lane & 31);
        const bool valid = active && s < m;
        const bool more = it + 1 < n_it;
        float x[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) x[i] = xn[i];
        const int src = srcn;
        const CfStore cfs(u, lane, n_tiles);
        f32x16 a[kNB], bacc[kNB];
        uint64_t m1 = 0, m2 = 0;
        float sdf = 0.f;
        // h2 read (its row of the step's h2): in flight under the W1 layer
        if (h2_given && active) load_rows(h2_rows, src, valid, bacc, h);
        // h1 = relu(W1 x + b1): resident W1
        if (active) {
            init_bias(a, lds + kOffB1, h);
            gemm_x(lds + kF2W1, x, a, lane);
            if constexpr (kMask) m1 = relu(a);
            else relu_values(a);
        }
        if (h2_given) {  // h1's stores; h2's mask
            if (active) {
                if (save) cfs.store(act, tbytes, a);
                m2 = relu(bacc);  // post-ReLU values: the same values and mask bits
            }
        } else {
            // h2 = relu(W2 h1 + b2)
            wait_vm(0);
            raw_barrier();
            stage8(buf(seq + 1), img + kImgF3, 16384, wave, lane);
            if (active) {
                init_bias(bacc, lds + kOffB2, h);
                gemm_acc<kNB, kNB>(buf(seq), a, bacc, lane, CfQueue(cfs, act, tbytes, save, a));  // + h1 stores
                if constexpr (kMask) m2 = relu(bacc);
                else relu_values(bacc);
            }
            ++seq;
        }
        // [sdf | f] = W3 h2 + b3
        wait_vm(0);
        raw_barrier();
        stage8(buf(seq + 1), img + kImgF4, 18432, wave, lane);
        if (active) {
            sdf = __fadd_rn(lds[kOffB3], row_dot(lds + kOffW3r0, bacc, h));
            init_bias(a, lds + kOffB3 + 1, h);
            gemm_acc<kNB, kNB>(buf(seq), bacc, a, lane, CfQueue(cfs, act + tstride, tbytes, save, bacc));  // + h2
        }
        ++seq;
        // c1 = relu(W4 [f; x] + b4); the next tile's W2 and x start loading
        wait_vm(0);
        raw_barrier();
        if (more) {
            stage8(buf(seq + 1), img + (h2_given ? kImgF3 : kImgF2), 16384, wave, lane);
            const int64_t un = u + kF2Waves;
            const int64_t sn = un * kTileS + (lane & 31);
            if (h2_given && un < u1 && sn < m) srcn = h2_src[sn];
            if constexpr (IP)
                iload::load_x_interp(ip, sn, un < u1 && sn < m, h, xn);
            else
                load_x(feat, h2_given ? (int64_t)srcn : sn, un < u1 && sn < m, h, xn);
        }
        if (!active) {
            ++seq;
            if (!H2) PSVO_STAMP(8);
            PSVO_STAMP_FLUSH(0);
            continue;
        }
        init_bias(bacc, lds + kOffB4, h);
        uint32_t half4[2] = {0u, 0u};
        {
            const float *wl4 = buf(seq);
            const float *fm = act + 2 * tstride, *cm = act + 3 * tstride;
            l4_block<0, kMask>(wl4, a, x, bacc, lane, L4Queue<0>(cfs, fm, cm, tbytes, save, a, bacc), half4);
            l4_block<1, kMask>(wl4, a, x, bacc, lane, L4Queue<1>(cfs, fm, cm, tbytes, save, a, bacc), half4);
            l4_block<2, kMask>(wl4, a, x, bacc, lane, L4Queue<2>(cfs, fm, cm, tbytes, save, a, bacc), half4);
            l4_block<3, kMask>(wl4, a, x, bacc, lane, L4Queue<3>(cfs, fm, cm, tbytes, save, a, bacc), half4);
            if (save && cfs.ok) {  // c1 block 3
                const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(
                    const_cast<float *>(cm), 0, __builtin_amdgcn_readfirstlane((int)tbytes), 0x00020000);
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(bacc[3][r]), rc,
                                                          cfs.voff[((r >> 1) & 1) + 2 * ((r >> 2) & 1)],
                                                          4096 * 3 + 1024 * (r >> 2) + 128 * (r & 3), 0);
            }
        }
        ++seq;
        const uint64_t m4 = (uint64_t)mask_word(half4[0]) | ((uint64_t)mask_word(half4[1]) << 32);
        if (save_mask && valid) {
            uint64_t *mk = masks + (s * 2 + h) * 3;
            mk[0] = m1;
            mk[1] = m2;
            mk[2] = m4;
        }
        float rgb[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) rgb[c] = sigmoidf(lds[kOffB5 + c] + row_dot(lds + kOffW5 + 128 * c, bacc, h));
        if (valid && h == 0) {
            sdf_out[s] = sdf;
            rgb_out[s * 3 + 0] = rgb[0];
            rgb_out[s * 3 + 1] = rgb[1];
            rgb_out[s * 3 + 2] = rgb[2];
        }
        if (!H2) PSVO_STAMP(8);
        PSVO_STAMP_FLUSH(0);
    }
    wait_vm(0);
}

// sdf only (Decoder.get_sdf; mesh lattices): h1, h2 and the sdf row of W3 —
// 18.3 of the 53.7 k MACs per sample.  W1 and W2 stay resident (77 KB of
// LDS, no staging in the loop); the same instruction sequence as
// k_mlp_fwd2's first two layers, so the sdf is bit-identical to its output.
//
// IP: as k_mlp_fwd2's — the frame renderer's trunk pass.  FS (with IP: the
// mapping engine's device-sized trunk): `feat` is written, not read — the
// interpolated rows, k_interp_fwd's table, for the kernels after the selection
template <bool IP = false, bool FS = false>
__global__ __launch_bounds__(kF2Threads, 1) void k_mlp_sdf2(int64_t m_host,
                                                            std::conditional_t<FS, float, const float> *__restrict__ feat,
                                                            const float *__restrict__ img,
                                                            float *__restrict__ sdf_out, const int *__restrict__ m_dev,
                                                            float *__restrict__ h2_out, InterpSrc ip) {
    static_assert(IP || !FS, "the feature rows are stored by the interpolating operand load");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    // m_dev: the count on the device, m_host the buffers' capacity (a larger
    // batch: nothing here, the host-sized launch after the read-back)
    int64_t m = m_dev ? (int64_t)__builtin_amdgcn_readfirstlane(*m_dev) : m_host;
    if (m > m_host) m = 0;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int h = lane >> 5;
    float *w2 = lds + kF2Buf0;
    // the balanced split of k_mlp_fwd2: workgroup b owns the
    // 32-sample tiles [u0, u1), wave w the tiles u0 + w, u0 + w + 8, …
    const int64_t n_units = (m + kTileS - 1) / kTileS;
    const int64_t u0 = n_units * blockIdx.x / gridDim.x, u1 = n_units * (blockIdx.x + 1) / gridDim.x;
    float xn[8];
    {
        const int64_t s = (u0 + wave) * kTileS + (lane & 31);
        if constexpr (FS)
            iload::load_x_interp<true>(ip, s, u0 + wave < u1 && s < m, h, xn, feat);
        else if constexpr (IP)
            iload::load_x_interp(ip, s, u0 + wave < u1 && s < m, h, xn);
        else
            load_x(feat, s, u0 + wave < u1 && s < m, h, xn);
    }
    stage8(lds, img + kImgVec, kVecPad, wave, lane);
    stage8(lds + kF2W1, img + kImgF1, 2048, wave, lane);
    stage8(w2, img + kImgF2, 16384, wave, lane);
    wait_vm(0);
    raw_barrier();
    for (int64_t u = u0 + wave; u < u1; u += kF2Waves) {  // no barriers below
        const int64_t s = u * kTileS + (lane & 31);
        const bool valid = s < m;
        float x[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) x[i] = xn[i];
        if (u + kF2Waves < u1) {
            const int64_t sn = (u + kF2Waves) * kTileS + (lane & 31);
            if constexpr (FS)
                iload::load_x_interp<true>(ip, sn, sn < m, h, xn, feat);
            else if constexpr (IP)
                iload::load_x_interp(ip, sn, sn < m, h, xn);
            else
                load_x(feat, sn, sn < m, h, xn);
        }
        f32x16 a[kNB], bacc[kNB];
        init_bias(a, lds + kOffB1, h);
        gemm_x(lds + kF2W1, x, a, lane);
        relu_values(a);  // no masks: nothing reads them
        init_bias(bacc, lds + kOffB2, h);
        gemm_acc<kNB, kNB>(w2, a, bacc, lane);
        relu_values(bacc);
        const float sdf = __fadd_rn(lds[kOffB3], row_dot(lds + kOffW3r0, bacc, h));
        if (valid && h == 0) sdf_out[s] = sdf;
        if (h2_out) store_rows(h2_out, s, valid, kW, bacc, h);  // (the sparse decoder's later layers read it)
    }
    wait_vm(0);
}

void launch_prep(hipStream_t st, const float *const *dec, float *images) {
    MlpParams p{dec[0], dec[1], dec[2], dec[3], dec[4], dec[5], dec[6], dec[7], dec[8], dec[9]};
    psvo::launch(k_mlp_prep, dim3(div_up(kImgTotal, 256)), dim3(256), 0, st, p, images);
}
// the persistent forward kernels' grid: one workgroup per CU, or per 256-sample tile if fewer
int fwd_grid(int64_t m) { return persistent_grid(div_up(m, kF2Tile)); }

}  // namespace

int64_t dec128_image_floats() { return kImgTotal; }
int64_t dec128_act_floats(int64_t m) { return (m + kCh - 1) / kCh * kCh * 4 * 128; }
int64_t dec128_mask_words(int64_t m) { return m * 6; }

int dec128_images(hipStream_t st, const float *const *dec, float *images) {
    launch_prep(st, dec, images);
    return check_launch("mlp_images");
}

int dec128_fwd(hipStream_t st, int64_t m, const float *feat, const float *const *dec, float *images, float *sdf,
               float *rgb, float *act, uint64_t *masks, const int *m_dev, const H2Rows *h2) {
    PSVO_REQUIRE(m >= 0, "mlp_fwd: m < 0");
    PSVO_REQUIRE(images != nullptr, "mlp_fwd: images workspace required (psvo_mlp_image_floats floats)");
    PSVO_REQUIRE(act == nullptr || masks != nullptr, "mlp_fwd: act needs masks");
    PSVO_REQUIRE(m <= kMaxSamples, "mlp_fwd: m = %lld > %lld (32-bit CF offsets)", (long long)m,
                 (long long)kMaxSamples);
    if (m == 0) return PSVO_OK;
    if (dec) launch_prep(st, dec, images);
    if (rgb == nullptr) {  // sdf only (inference)
        PSVO_REQUIRE(act == nullptr && masks == nullptr, "mlp_fwd: the sdf-only forward is inference only");
        launch_lds<k_mlp_sdf2<false>>(dim3(fwd_grid(m)), dim3(kF2Threads), kLdsSdf2, st, m, feat, images, sdf, m_dev,
                                      h2 ? h2->out : nullptr, InterpSrc{});
        return check_launch("mlp_fwd");
    }
    const int grid = fwd_grid(m);  // ≥ 8 units per workgroup
    PSVO_REQUIRE(!h2 || !h2->rows || h2->src, "mlp_fwd: h2 rows need their source index");
    if (h2 && h2->rows)
        launch_lds<k_mlp_fwd2<true>>(dim3(grid), dim3(kF2Threads), kLdsFwd2, st, m, feat, images, sdf, rgb, act, masks,
                                     m_dev, h2->rows, h2->src, InterpSrc{});
    else
        launch_lds<k_mlp_fwd2<false>>(dim3(grid), dim3(kF2Threads), kLdsFwd2, st, m, feat, images, sdf, rgb, act,
                                      masks, m_dev, nullptr, nullptr, InterpSrc{});
    return check_launch("mlp_fwd");
}

// The frame renderer's width-128 decoder passes (csrc/render.hip): the sdf
// trunk (rgb null) or the whole forward (rgb given) on the m_dev[0] <= m_cap
// samples of `ip`, their features interpolated in the operand load.  m_cap
// only sizes the grid (no activations are stored: no CF offsets).
int mlp_fwd_interp(hipStream_t st, int64_t m_cap, const int *m_dev, const InterpSrc &ip, const float *images,
                   float *sdf, float *rgb) {
    PSVO_REQUIRE(m_cap >= 0 && m_dev && images && sdf, "mlp_fwd_interp: bad arguments");
    if (m_cap == 0) return PSVO_OK;
    const dim3 grid(fwd_grid(m_cap)), block(kF2Threads);
    if (rgb == nullptr)
        launch_lds<k_mlp_sdf2<true>>(grid, block, kLdsSdf2, st, m_cap, nullptr, images, sdf, m_dev, nullptr, ip);
    else
        launch_lds<k_mlp_fwd2<false, true>>(grid, block, kLdsFwd2, st, m_cap, nullptr, images, sdf, rgb, nullptr,
                                            nullptr, m_dev, nullptr, nullptr, ip);
    return check_launch("mlp_fwd_interp");
}
// The mapping engine's device-sized sdf trunk (engine_step.cpp
// device_forward): interp_fwd_dev + the plain trunk in one launch — the same
// sdf, h2 rows and feature rows, bit for bit; rows >= m_dev[0], and every row
// when m_dev[0] > m_cap, are left as they were.
int mlp_trunk_interp(hipStream_t st, int64_t m_cap, const int *m_dev, const InterpSrc &ip, const float *images,
                     float *sdf, float *h2_out, float *feat_out) {
    PSVO_REQUIRE(m_cap >= 0 && m_dev && images && sdf && h2_out && feat_out && ip.leaf && ip.t && ip.ray_of &&
                     ip.ray_index && ip.voxel_size > 0.f,
                 "mlp_trunk_interp: bad arguments");
    PSVO_REQUIRE(m_cap <= kMaxSamples, "mlp_trunk_interp: m_cap = %lld > %lld", (long long)m_cap,
                 (long long)kMaxSamples);
    if (m_cap == 0) return PSVO_OK;
    launch_lds<k_mlp_sdf2<true, true>>(dim3(fwd_grid(m_cap)), dim3(kF2Threads), kLdsSdf2, st, m_cap, feat_out, images,
                                       sdf, m_dev, h2_out, ip);
    return check_launch("mlp_trunk_interp");
}

}  // namespace psvo
