// Device functions shared by the mapping step's sample selection
// (composite.hip k_select_samples) and the frame renderer's (render.hip):
// one definition of z_min, so both select the same composited set.
#pragma once

#include "psvo_common.h"

namespace psvo {
namespace sel {

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v = min(v, __shfl_xor(v, s, 64));
    return v;
}

// the ray's z_min (k_composite_loss's first sign change of the padded sdf
// row): the ray's ns samples at sdf_s[off ..], its depths z[0 .. ns), the row
// padded with sdf = 1 up to s_max columns (strict comparisons,
// the ±0 products, the padding of 1).  One wave per ray.
__device__ __forceinline__ float sel_zmin(int lane, int s_max, int ns, int off, const float *z,
                                          const float *__restrict__ sdf_s) {
    const int lim = ns < s_max ? ns : s_max;
    auto sdf_at = [&](int s) { return s < ns ? sdf_s[off + s] : 1.0f; };
    int first = s_max;
    for (int s = lane; s < lim; s += 64) {
        const float v = sdf_at(s);
        const float v1 = s + 1 < s_max ? sdf_at(s + 1) : 0.f;
        if (s + 1 < s_max && v1 * v < 0.0f) first = min(first, s);
    }
    first = wave_min(first);
    const int f0 = first == s_max ? 0 : first;
    return f0 < ns ? z[f0] : kMaxDepthFill;
}

}  // namespace sel
}  // namespace psvo
