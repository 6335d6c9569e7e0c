// The interpolation forward (interp.hip's k_interp_fwd arithmetic) as the
// operand load of the width-128 decoder's forward kernels (mlp_fwd.hip k_mlp_sdf2
// / k_mlp_fwd2, the frame renderer's instantiations): a sample's 16 features
// are formed in registers from (leaf, t, ray) and the embedding rows and go
// straight into the W1 MFMAs — no [M,16] feature rows read back from HBM (the
// renderer keeps none at all; the mapping engine's trunk leaves them for the
// kernels after the selection).
#pragma once

#include "psvo_common.h"

namespace psvo {

// where a forward kernel's x comes from when it is not a feature row: the
// samples' leaf / depth / ray-of-sample (ray-major), the ray of hit row r at
// ray_index[r], and the map
struct InterpSrc {
    const int *leaf, *ray_of, *ray_index, *vertex_idx;
    const float *t, *rays_o, *rays_d, *centres;
    const float4 *emb;
    float voxel_size;
};

// mlp_fwd.hip: the sdf trunk (rgb null) or the whole width-128 forward on the
// m_dev[0] <= m_cap samples of `ip`; m_cap only sizes the grid
int mlp_fwd_interp(hipStream_t st, int64_t m_cap, const int *m_dev, const InterpSrc &ip, const float *images,
                   float *sdf, float *rgb);
// mlp_fwd.hip: the mapping engine's device-sized sdf trunk — as mlp_fwd_interp's,
// and it leaves what interp_fwd_dev + the plain trunk leave: every sample's
// h2 row (h2_out [m_cap][128]) and feature row (feat_out [m_cap][16]).
// m_dev[0] > m_cap: nothing is written
int mlp_trunk_interp(hipStream_t st, int64_t m_cap, const int *m_dev, const InterpSrc &ip, const float *images,
                     float *sdf, float *h2_out, float *feat_out);

namespace iload {

// One lane's half row: features 8h .. 8h + 7 of sample s into f (zeroed by
// the caller) — k_interp_fwd's formula and order: p = (o + d·t − c) / voxel +
// 0.5, w_k = (a_x · a_y) · a_z, f = Σ_k w_k · E_k summed from 0 in corner
// order.  The text is shared; whether each operation is rounded on its own is
// decided where it is expanded: plain operators, which the compiler contracts
// to FMAs unless the enclosing block says `fp contract(off)` (HIP's __fmul_rn
// / __fadd_rn are the same plain operators inside the header's functions, out
// of such a pragma's reach: they never kept these products and sums apart).
#define PSVO_ILOAD_FEAT8(ip, s, h, f)                                                                            \
    const int lf = ip.leaf[s];                                                                                   \
    const int r = ip.ray_index[ip.ray_of[s]];                                                                    \
    const float ts = ip.t[s];                                                                                    \
    float p[3];                                                                                                  \
    _Pragma("unroll") for (int a = 0; a < 3; ++a) {                                                              \
        const float xa = ip.rays_o[(int64_t)r * 3 + a] + ip.rays_d[(int64_t)r * 3 + a] * ts;                     \
        p[a] = __fdiv_rn(xa - ip.centres[(int64_t)lf * 3 + a], ip.voxel_size) + 0.5f;                            \
    }                                                                                                            \
    const float ax[2] = {1.0f - p[0], p[0]};                                                                     \
    const float ay[2] = {1.0f - p[1], p[1]};                                                                     \
    const float az[2] = {1.0f - p[2], p[2]};                                                                     \
    const int4 v0 = *reinterpret_cast<const int4 *>(ip.vertex_idx + (int64_t)lf * 8);                            \
    const int4 v1 = *reinterpret_cast<const int4 *>(ip.vertex_idx + (int64_t)lf * 8 + 4);                        \
    const int vid[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};                                         \
    float4 e0[8], e1[8];                                                                                         \
    _Pragma("unroll") for (int k = 0; k < 8; ++k) { /* the 16 loads in flight together */                        \
        e0[k] = ip.emb[(int64_t)vid[k] * 4 + 2 * h];                                                             \
        e1[k] = ip.emb[(int64_t)vid[k] * 4 + 2 * h + 1];                                                         \
    }                                                                                                            \
    _Pragma("unroll") for (int k = 0; k < 8; ++k) {                                                              \
        const float w = (ax[(k >> 2) & 1] * ay[(k >> 1) & 1]) * az[k & 1];                                       \
        f[0] = f[0] + w * e0[k].x;                                                                               \
        f[1] = f[1] + w * e0[k].y;                                                                               \
        f[2] = f[2] + w * e0[k].z;                                                                               \
        f[3] = f[3] + w * e0[k].w;                                                                               \
        f[4] = f[4] + w * e1[k].x;                                                                               \
        f[5] = f[5] + w * e1[k].y;                                                                               \
        f[6] = f[6] + w * e1[k].z;                                                                               \
        f[7] = f[7] + w * e1[k].w;                                                                               \
    }

// Lane (n = lane & 31, h = lane >> 5) of a 32-sample unit gets x[t] = feature
// 2t + h of sample s (mlp128.h load_x's layout).  The lane forms features
// 8h .. 8h + 7 itself — two 16-B loads per embedding row, the wave reads whole
// 64-B rows — and the two lanes of a sample swap the halves the other one
// needs.  All 64 lanes must call it (the swap is a cross-lane read); !valid:
// x = 0.
// STORE = false (the frame renderer): k_interp_fwd's values up to the
// compiler's contraction — o + d·t and the 64 multiply-adds of the corner sum
// are FMAs there (v_pk_fma_f32), so a feature can differ from the table's in
// the last bits; the renderer is pinned to render_rays within a tolerance.
// STORE = true (the mapping engine's trunk): contraction off, every operation
// rounded on its own as interp.hip compiles k_interp_fwd — the same bits —
// and a valid sample's features also go to row s of feat_out [·][16], the
// table the later decoder kernels read a kept sample's x from, before the
// swap, while the lane holds 8h .. 8h + 7 contiguously: two 16-B stores, the
// lane pair a whole 64-B row.
template <bool STORE = false>
__device__ __forceinline__ void load_x_interp(const InterpSrc &ip, int64_t s, bool valid, int h, float (&x)[8],
                                              float *feat_out = nullptr) {
    float f[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = 0.0f;
    if (valid) {
        if constexpr (STORE) {
#pragma clang fp contract(off)
            PSVO_ILOAD_FEAT8(ip, s, h, f)
            float4 *row = reinterpret_cast<float4 *>(feat_out + s * 16 + 8 * h);
            row[0] = make_float4(f[0], f[1], f[2], f[3]);
            row[1] = make_float4(f[4], f[5], f[6], f[7]);
        } else {
            PSVO_ILOAD_FEAT8(ip, s, h, f)
        }
    }
    // h = 0 holds features 0..7 and needs the even ones of 0..15: its own
    // 0, 2, 4, 6 and the partner's 8, 10, 12, 14; h = 1 holds 8..15 and needs
    // the odd ones: the partner's 1, 3, 5, 7 and its own 9, 11, 13, 15
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float send = h ? f[2 * j] : f[2 * j + 1];
        const float recv = __shfl_xor(send, 32, 64);
        x[j] = h ? recv : f[2 * j];
        x[4 + j] = h ? f[2 * j + 1] : recv;
    }
}

#undef PSVO_ILOAD_FEAT8

}  // namespace iload
}  // namespace psvo
