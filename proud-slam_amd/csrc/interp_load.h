// The interpolation forward (interp.hip's k_interp_fwd arithmetic) as the
// operand load of the width-128 decoder's forward kernels (mlp.hip k_mlp_sdf2
// / k_mlp_fwd2, the frame renderer's instantiations): a sample's 16 features
// are formed in registers from (leaf, t, ray) and the embedding rows and go
// straight into the W1 MFMAs — no [M,16] feature rows in HBM.
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

// mlp.hip: the sdf trunk (rgb null) or the whole width-128 forward on the
// m_dev[0] <= m_cap samples of `ip`; m_cap only sizes the grid
int mlp_fwd_interp(hipStream_t st, int64_t m_cap, const int *m_dev, const InterpSrc &ip, const float *images,
                   float *sdf, float *rgb);

namespace iload {

// Lane (n = lane & 31, h = lane >> 5) of a 32-sample unit gets x[t] = feature
// 2t + h of sample s (mlp.hip load_x's layout).  The lane forms features
// 8h .. 8h + 7 itself — two 16-B loads per embedding row, the wave reads whole
// 64-B rows — and the two lanes of a sample swap the halves the other one
// needs.  Every value is k_interp_fwd's: p = (o + d·t − c) / voxel + 0.5, w_k
// = (a_x · a_y) · a_z, f = Σ_k w_k · E_k summed from 0 in corner order, each
// operation rounded on its own (interp.hip compiles with contraction off).
// All 64 lanes must call it (the swap is a cross-lane read); !valid: x = 0.
__device__ __forceinline__ void load_x_interp(const InterpSrc &ip, int64_t s, bool valid, int h, float (&x)[8]) {
    float f[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = 0.0f;
    if (valid) {
        const int lf = ip.leaf[s];
        const int r = ip.ray_index[ip.ray_of[s]];
        const float ts = ip.t[s];
        float p[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float xa = __fadd_rn(ip.rays_o[(int64_t)r * 3 + a], __fmul_rn(ip.rays_d[(int64_t)r * 3 + a], ts));
            p[a] = __fadd_rn(__fdiv_rn(__fsub_rn(xa, ip.centres[(int64_t)lf * 3 + a]), ip.voxel_size), 0.5f);
        }
        const float ax[2] = {__fsub_rn(1.0f, p[0]), p[0]};
        const float ay[2] = {__fsub_rn(1.0f, p[1]), p[1]};
        const float az[2] = {__fsub_rn(1.0f, p[2]), p[2]};
        const int4 v0 = *reinterpret_cast<const int4 *>(ip.vertex_idx + (int64_t)lf * 8);
        const int4 v1 = *reinterpret_cast<const int4 *>(ip.vertex_idx + (int64_t)lf * 8 + 4);
        const int vid[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
        float4 e0[8], e1[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {  // the 16 loads in flight together
            e0[k] = ip.emb[(int64_t)vid[k] * 4 + 2 * h];
            e1[k] = ip.emb[(int64_t)vid[k] * 4 + 2 * h + 1];
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float w = __fmul_rn(__fmul_rn(ax[(k >> 2) & 1], ay[(k >> 1) & 1]), az[k & 1]);
            f[0] = __fadd_rn(f[0], __fmul_rn(w, e0[k].x));
            f[1] = __fadd_rn(f[1], __fmul_rn(w, e0[k].y));
            f[2] = __fadd_rn(f[2], __fmul_rn(w, e0[k].z));
            f[3] = __fadd_rn(f[3], __fmul_rn(w, e0[k].w));
            f[4] = __fadd_rn(f[4], __fmul_rn(w, e1[k].x));
            f[5] = __fadd_rn(f[5], __fmul_rn(w, e1[k].y));
            f[6] = __fadd_rn(f[6], __fmul_rn(w, e1[k].z));
            f[7] = __fadd_rn(f[7], __fmul_rn(w, e1[k].w));
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

}  // namespace iload
}  // namespace psvo
