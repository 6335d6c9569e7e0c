// The decoder's width dispatch and C ABI (include/psvo.h psvo_mlp_*): every
// call goes to dec128_* (mlp_fwd.hip, mlp_bwd.hip, mlp128_trunk_fb.h) or
// dec256_* (mlp256.hip), which check their own arguments and launch their
// own kernels — nothing is launched from here.
#include <hip/hip_runtime.h>

#include "interp_load.h"
#include "psvo_common.h"

namespace psvo {

int device_cus() {
    static int cus = 0;
    if (cus == 0) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
            cus = 256;
    }
    return cus;
}

// dec: the ten parameter tensors W1, b1, ..., W5, b5, or null: `images` already holds them (mlp_images)
static int mlp_fwd_impl(void *stream, int64_t m, int width, const float *feat, const float *const *dec, float *images,
                        float *sdf, float *rgb, float *act, uint64_t *masks, const int *m_dev = nullptr,
                        const H2Rows *h2 = nullptr) {
    hipStream_t st = as_stream(stream);
    if (width == 256) return dec256_fwd(st, m, feat, dec, images, sdf, rgb, act, masks, m_dev);
    PSVO_REQUIRE(width == 128, "mlp_fwd: width %d unsupported (fused paths: 128, 256)", width);
    return dec128_fwd(st, m, feat, dec, images, sdf, rgb, act, masks, m_dev, h2);
}

int mlp_images(void *stream, int width, const float *const *dec, float *images) {
    if (width == 256) return dec256_images(as_stream(stream), dec, images);
    return dec128_images(as_stream(stream), dec, images);
}
int mlp_fwd_prepared(void *stream, int64_t m, int width, const float *feat, float *images, float *sdf, float *rgb,
                     float *act, uint64_t *masks, const int *m_dev, const H2Rows *h2) {
    return mlp_fwd_impl(stream, m, width, feat, nullptr, images, sdf, rgb, act, masks, m_dev, h2);
}
int mlp_fwd(void *stream, int64_t m, int width, const float *feat, const float *const *dec, float *images, float *sdf,
            float *rgb, float *act, uint64_t *masks) {
    return mlp_fwd_impl(stream, m, width, feat, dec, images, sdf, rgb, act, masks);
}

int mlp_bwd(void *stream, int64_t m, int width, const float *feat, const float *images, const float *rgb,
            const float *act, const uint64_t *masks, const float *g_sdf, const float *g_rgb, float *dfeat,
            float *const *grads, int accumulate, int n_split, float *workspace, hipEvent_t dfeat_ready,
            const InterpFuse *ip, hipStream_t reduce_stream, const int *m_dev, const TrunkBwd *tb, const int *x_src) {
    float *gw[5], *gb[5];  // grads = {gW1, gb1, ..., gW5, gb5}
    for (int l = 0; l < 5; ++l) {
        gw[l] = grads ? grads[2 * l] : nullptr;
        gb[l] = grads ? grads[2 * l + 1] : nullptr;
    }
    PSVO_REQUIRE(ip == nullptr || ((width == 256 || width == 128) && gw[0] != nullptr),
                 "mlp_bwd: the fused interpolation backward needs a fused weight-gradient path");
    hipStream_t st = as_stream(stream);
    if (width == 256)
        return dec256_bwd(st, m, feat, images, rgb, act, masks, g_sdf, g_rgb, dfeat, gw, gb, accumulate, workspace,
                          dfeat_ready, ip, m_dev);
    PSVO_REQUIRE(width == 128, "mlp_bwd: width %d unsupported (fused paths: 128, 256)", width);
    return dec128_bwd(st, m, feat, images, rgb, act, masks, g_sdf, g_rgb, dfeat, gw, gb, accumulate, n_split,
                      workspace, dfeat_ready, ip, reduce_stream, m_dev, tb, x_src);
}

// width 128: the interpolation backward runs inside k_mlp_bwd3; width 256:
// k_interp_bwd beside the weight-gradient kernel (measured faster than inside
// k_dec256_bwd: there the scatter's atomics overlap the dW MFMAs)
bool mlp_bwd_fuses_interp(int width) { return width == 128; }
bool mlp_bwd_split_tail(int width) { return width == 128; }

}  // namespace psvo

using namespace psvo;

extern "C" int64_t psvo_mlp_image_floats(void) { return dec128_image_floats(); }
extern "C" int64_t psvo_mlp_image_floats_w(int width) {
    return width == 128 ? dec128_image_floats() : width == 256 ? dec256_image_floats() : -1;
}
extern "C" int64_t psvo_mlp_act_floats(int64_t m, int width) {
    return width == 128 ? dec128_act_floats(m) : width == 256 ? dec256_act_floats(m) : -1;
}
extern "C" int64_t psvo_mlp_mask_words(int64_t m, int width) {
    return width == 128 ? dec128_mask_words(m) : width == 256 ? dec256_mask_words(m) : -1;
}
extern "C" int64_t psvo_mlp_workspace_floats(int64_t m, int n_split) {
    (void)n_split;  // accepted for compatibility: one slab per workgroup, whatever it says
    return dec128_workspace_floats(m);
}
extern "C" int64_t psvo_mlp_workspace_floats_w(int64_t m, int width, int n_split) {
    return width == 128 ? psvo_mlp_workspace_floats(m, n_split) : width == 256 ? dec256_workspace_floats(m) : -1;
}

// tests only: the device-sized trunk on its own — fused = 1 the engine's one
// launch, fused = 0 the two kernels it replaces, into the same outputs
extern "C" int psvo_debug_trunk_interp(void *stream, int fused, int64_t m_cap, const int *m_dev, const int *leaf,
                                       const float *t, const int *ray_of, const int *ray_index, const float *rays_o,
                                       const float *rays_d, const float *centres, const int *vertex_idx,
                                       const float *emb, float voxel_size, const float *w1, const float *b1,
                                       const float *w2, const float *b2, const float *w3, const float *b3,
                                       const float *w4, const float *b4, const float *w5, const float *b5,
                                       float *images, float *sdf, float *h2, float *feat) {
    PSVO_REQUIRE(m_dev && images && sdf && h2 && feat, "debug_trunk_interp: null argument");
    hipStream_t st = as_stream(stream);
    const float *const dec[10] = {w1, b1, w2, b2, w3, b3, w4, b4, w5, b5};
    int rc = psvo::mlp_images(stream, 128, dec, images);
    if (rc) return rc;
    if (fused) {
        const InterpSrc ip{leaf, ray_of, ray_index, vertex_idx, t, rays_o, rays_d, centres,
                           reinterpret_cast<const float4 *>(emb), voxel_size};
        return psvo::mlp_trunk_interp(st, m_cap, m_dev, ip, images, sdf, h2, feat);
    }
    rc = psvo::interp_fwd_dev(st, m_cap, m_dev, voxel_size, leaf, t, ray_of, ray_index, rays_o, rays_d, centres,
                              vertex_idx, emb, feat);
    if (rc) return rc;
    const H2Rows h2o{h2, nullptr, nullptr};
    return psvo::mlp_fwd_prepared(stream, m_cap, 128, feat, images, sdf, nullptr, nullptr, nullptr, m_dev, &h2o);
}

extern "C" int psvo_mlp_fwd(void *stream, int64_t m, int width, const float *feat, const float *w1, const float *b1,
                            const float *w2, const float *b2, const float *w3, const float *b3, const float *w4,
                            const float *b4, const float *w5, const float *b5, float *images, float *sdf, float *rgb,
                            float *act, uint64_t *masks) {
    const float *const dec[10] = {w1, b1, w2, b2, w3, b3, w4, b4, w5, b5};
    return psvo::mlp_fwd(stream, m, width, feat, dec, images, sdf, rgb, act, masks);
}

extern "C" int psvo_mlp_bwd(void *stream, int64_t m, int width, const float *feat, const float *w1, const float *b1,
                            const float *w2, const float *b2, const float *w3, const float *b3, const float *w4,
                            const float *b4, const float *w5, const float *b5, const float *images, const float *rgb,
                            const float *act, const uint64_t *masks, const float *g_sdf, const float *g_rgb, float *dfeat, float *gw1,
                            float *gb1, float *gw2, float *gb2, float *gw3, float *gb3, float *gw4, float *gb4,
                            float *gw5, float *gb5, int accumulate, int n_split, float *workspace) {
    // (the weights are not read: `images` holds them)
    float *const grads[10] = {gw1, gb1, gw2, gb2, gw3, gb3, gw4, gb4, gw5, gb5};
    return psvo::mlp_bwd(stream, m, width, feat, images, rgb, act, masks, g_sdf, g_rgb, dfeat, grads, accumulate,
                         n_split, workspace, nullptr);
}
