// Keyframe covisibility on gfx950: which leaf voxels a depth frame sees, as a
// bitset over node ids, and the overlap counts between such sets.
//
// V(frame, tree) = the leaves the reference's walk (intersect_gpu.cu:191-270:
// a node is tested iff its parent passed the slab test) emits for some ray of
// the frame, kept when t_in <= depth + truncation and !(t_in > max_distance).
// Unlike the query stage (query_trace.hip) there is NO cap on the leaves per
// ray: the 50-leaf cap keeps the first 50 leaves of the depth-first order
// (children popped 7→0), which along a row of voxels are the farthest ones.
// A set does not depend on the order the leaves are found in, so the walk
// needs no keys, no hit list, no sort and no look-back.
//
// MI355X design: one lane per ray, a 16 x 16 tile of the frame's sampled
// pixels per workgroup (a wave = 16 x 4 neighbouring pixels: they descend
// the same nodes, so the walk diverges little and its record loads hit the
// same lines).  The per-lane level stack lives in LDS, [level][lane].  Bits:
// when the set fits (words <= kCovisLdsWords) the workgroup collects its bits
// in LDS and merges the non-zero words into the frame's row once — a tile's
// rays see the same few voxels —; larger trees (config E: 2.7 M nodes,
// 340 KB per set) set them in global memory directly.  Either way a word is
// read (past the L1: another CU may have set the bit since) before the
// atomicOr, which runs at the memory side, so once a voxel is marked its
// later sightings cost a load.
//
// No subtree is skipped on the depth bound: the fp32 centres of a child and
// its parent are rounded separately, so a child's box is not exactly inside
// its parent's and t_lo(parent) > bound does not prove t_in(leaf) > bound for
// every leaf below.  The walk is exactly the reference's; only the emitted
// leaves are filtered.
//
// Arithmetic: contraction off and IEEE division, as query_trace.hip — the
// slab test is the shared one (query_common.h) and the ray directions are
// formed product by product (include/psvo.h), so every t_in is the CPU
// oracle's bit for bit and the sets compare exactly.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include "query.h"
#include "query_common.h"

namespace psvo {
namespace {

constexpr int kCovisTile = 16;                        // sampled pixels per tile side
constexpr int kCovisThreads = kCovisTile * kCovisTile;
constexpr int kCovisLdsWords = 2048;                  // 8 KB: sets of up to 65,536 nodes are staged in LDS
constexpr int kCovisFrames = 64;                      // frames per launch (their image pointers are launch arguments)

struct CovisFrames {
    const float *depth[kCovisFrames];
};

template <bool LDSBITS>
__device__ __forceinline__ void mark(uint32_t *bits, int ref, int64_t n_nodes) {
    if (ref < 0 || ref >= n_nodes) return;  // a corrupt id marks nothing
    const uint32_t b = 1u << (ref & 31);
    uint32_t *wd = bits + (ref >> 5);
    if constexpr (LDSBITS) {
        if (!(*wd & b)) atomicOr(wd, b);
    } else {
        if (!((uint32_t)ld_wt(reinterpret_cast<const int *>(wd)) & b)) atomicOr(wd, b);
    }
}

template <bool PACKED, bool LDSBITS>
__global__ __launch_bounds__(kCovisThreads) void k_frames_visible(int h, int w, int px_step, CovisFrames frames,
                                                                   const float *__restrict__ dirs_cam,
                                                                   const float *__restrict__ poses34, int64_t n_nodes,
                                                                   const PackRec *__restrict__ packed,
                                                                   const float *__restrict__ centres,
                                                                   const int *__restrict__ structure, float voxel_size,
                                                                   float truncation, float max_distance, int64_t words,
                                                                   uint32_t *__restrict__ bits, int *__restrict__ flags) {
    // level l of lane t: PACKED (next child record, one past the last), else (node, children still to visit)
    __shared__ int l_a[kLevels * kCovisThreads];
    __shared__ int l_b[kLevels * kCovisThreads];
    __shared__ uint32_t s_bits[LDSBITS ? kCovisLdsWords : 1];
    const int t = threadIdx.x;
    const int f = blockIdx.z;
    uint32_t *row = bits + (int64_t)f * words;
    if constexpr (LDSBITS) {
        for (int i = t; i < words; i += kCovisThreads) s_bits[i] = 0u;
        __syncthreads();
    }
    uint32_t *dst = LDSBITS ? s_bits : row;

    const int64_t x = ((int64_t)blockIdx.x * kCovisTile + (t & (kCovisTile - 1))) * px_step;
    const int64_t y = ((int64_t)blockIdx.y * kCovisTile + t / kCovisTile) * px_step;
    bool active = x < w && y < h;
    const int64_t pix = active ? y * w + x : 0;
    const float depth = active ? frames.depth[f][pix] : 0.0f;
    active = active && depth > 0.0f;  // NaN: not a ray
    bool overflow = false;
    if (active) {
        const float *P = poses34 + (int64_t)f * 12;
        const float c0 = dirs_cam[pix * 3 + 0], c1 = dirs_cam[pix * 3 + 1], c2 = dirs_cam[pix * 3 + 2];
        float o[3], inv[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float d = (c0 * P[j * 4 + 0] + c1 * P[j * 4 + 1]) + c2 * P[j * 4 + 2];
            o[j] = P[j * 4 + 3];
            inv[j] = __fdiv_rn(1.0f, d);
        }
        const float bound = depth + truncation;
        const float half = voxel_size * 0.5f;
        int *sa = l_a + t, *sb = l_b + t;
        int lvl = -1;
        {  // the root
            float t0 = 0.f, t1 = 0.f;
            int side, ref = 0, first = 0, cmask = 0;
            bool hit;
            if constexpr (PACKED) {
                const float4 pc = packed[0].c;
                const int4 pi = packed[0].i;
                side = __float_as_int(pc.w);
                ref = pi.x;
                first = pi.y;
                cmask = pi.z;
                hit = ray_aabb_nb(o, inv, pc.x, pc.y, pc.z, half * (float)side, t0, t1);
            } else {
                side = structure[8];
                hit = ray_aabb_nb(o, inv, centres[0], centres[1], centres[2], half * (float)side, t0, t1);
                if (hit && side != 1) {
#pragma unroll
                    for (int u = 0; u < 8; ++u) cmask |= (structure[u] > -1) ? (1 << u) : 0;
                }
            }
            if (hit) {
                if (side == 1) {
                    if (t0 <= bound && !(t0 > max_distance)) mark<LDSBITS>(dst, ref, n_nodes);
                } else if (cmask) {
                    lvl = 0;
                    sa[0] = PACKED ? first : 0;
                    sb[0] = PACKED ? first + __popc(cmask) : cmask;
                }
            }
        }
        while (lvl >= 0) {
            int k;
            if constexpr (PACKED) {
                k = sa[lvl * kCovisThreads];
                if (k >= sb[lvl * kCovisThreads]) {
                    --lvl;
                    continue;
                }
                sa[lvl * kCovisThreads] = k + 1;
            } else {
                const int m = sb[lvl * kCovisThreads];
                if (m == 0) {
                    --lvl;
                    continue;
                }
                const int u = 31 - __clz(m);
                sb[lvl * kCovisThreads] = m & ~(1 << u);
                k = structure[(int64_t)sa[lvl * kCovisThreads] * 9 + u];
            }
            if (k < 0 || k >= n_nodes) continue;  // a corrupt link is not followed
            float t0 = 0.f, t1 = 0.f;
            int side, ref = k, first = 0, cmask = 0;
            bool hit;
            if constexpr (PACKED) {
                const float4 pc = packed[k].c;
                const int4 pi = packed[k].i;
                side = __float_as_int(pc.w);
                ref = pi.x;
                first = pi.y;
                cmask = pi.z;
                hit = ray_aabb_nb(o, inv, pc.x, pc.y, pc.z, half * (float)side, t0, t1);
            } else {
                const float *pc = centres + (int64_t)k * 3;
                side = structure[(int64_t)k * 9 + 8];
                hit = ray_aabb_nb(o, inv, pc[0], pc[1], pc[2], half * (float)side, t0, t1);
            }
            if (!hit) continue;
            if (side == 1) {
                if (t0 <= bound && !(t0 > max_distance)) mark<LDSBITS>(dst, ref, n_nodes);
                continue;
            }
            if (lvl + 1 >= kLevels) {  // deeper than the level stack: reported, never stored past it
                overflow = true;
                continue;
            }
            if constexpr (!PACKED) {
                const int *rw = structure + (int64_t)k * 9;
#pragma unroll
                for (int u = 0; u < 8; ++u) cmask |= (rw[u] > -1) ? (1 << u) : 0;
            }
            if (!cmask) continue;
            ++lvl;
            sa[lvl * kCovisThreads] = PACKED ? first : k;
            sb[lvl * kCovisThreads] = PACKED ? first + __popc(cmask) : cmask;
        }
    }
    if (overflow && flags) atomicOr(flags, kStatFlagDfsOverflow);
    if constexpr (LDSBITS) {
        __syncthreads();
        for (int i = t; i < words; i += kCovisThreads) {
            const uint32_t v = s_bits[i];
            if (v && (v & ~(uint32_t)ld_wt(reinterpret_cast<const int *>(row + i)))) atomicOr(row + i, v);
        }
    }
}

// out[k] = {|S_k ∩ Q|, |S_k|} for k < n_sets, out[n_sets] = {|Q|, |Q|}: one
// workgroup per row, every word read once, no atomics
constexpr int kOvThreads = 256;

__global__ __launch_bounds__(kOvThreads) void k_visibility_overlap(int n_sets, int64_t words,
                                                                   const uint32_t *__restrict__ sets,
                                                                   const uint32_t *__restrict__ query,
                                                                   int *__restrict__ out) {
    __shared__ int s_i[kOvThreads / kWave], s_n[kOvThreads / kWave];
    const int k = blockIdx.x;
    const uint32_t *s = k < n_sets ? sets + (int64_t)k * words : query;
    int inter = 0, size = 0;
    for (int64_t i = threadIdx.x; i < words; i += kOvThreads) {
        const uint32_t a = s[i], q = query[i];
        inter += __popc(a & q);
        size += __popc(a);
    }
    inter = wave_sum(inter);
    size = wave_sum(size);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        s_i[threadIdx.x / kWave] = inter;
        s_n[threadIdx.x / kWave] = size;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int a = 0, b = 0;
        for (int j = 0; j < kOvThreads / kWave; ++j) {
            a += s_i[j];
            b += s_n[j];
        }
        out[2 * k + 0] = a;
        out[2 * k + 1] = b;
    }
}

}  // namespace
}  // namespace psvo

using namespace psvo;

extern "C" int64_t psvo_visibility_words(int64_t n_nodes) { return n_nodes > 0 ? (n_nodes + 31) / 32 : 0; }

extern "C" int psvo_frames_visible(void *stream, int n_frames, int h, int w, int px_step, const float *const *depth,
                                   const float *dirs_cam, const float *poses34, int64_t n_nodes, const void *packed,
                                   const float *centres, const int *structure, float voxel_size, float truncation,
                                   float max_distance, uint32_t *bits, int *flags) {
    PSVO_REQUIRE(n_frames >= 0 && h > 0 && w > 0 && px_step > 0, "frames_visible: bad sizes n_frames=%d h=%d w=%d px_step=%d",
                 n_frames, h, w, px_step);
    PSVO_REQUIRE((int64_t)h * w <= (int64_t)1 << 24, "frames_visible: h*w exceeds 2^24");
    PSVO_REQUIRE(n_nodes > 0 && n_nodes <= 0x7fffffff, "frames_visible: bad node count %lld", (long long)n_nodes);
    PSVO_REQUIRE(voxel_size > 0.0f, "frames_visible: voxel_size must be > 0");
    PSVO_REQUIRE(depth && dirs_cam && poses34 && centres && structure && bits, "frames_visible: null pointer");
    PSVO_REQUIRE(((uintptr_t)packed & 15) == 0, "frames_visible: packed records must be 16-B aligned");
    for (int f = 0; f < n_frames; ++f) PSVO_REQUIRE(depth[f], "frames_visible: frame %d has no depth image", f);
    if (n_frames == 0) return PSVO_OK;
    hipStream_t st = as_stream(stream);
    const int64_t words = psvo_visibility_words(n_nodes);
    if (hipMemsetAsync(bits, 0, sizeof(uint32_t) * (size_t)(words * n_frames), st) != hipSuccess)
        return set_error(PSVO_E_LAUNCH, "frames_visible: memset failed");
    // sampled pixels per row / column (64-bit: px_step may be anything up to INT_MAX)
    const int sw = (int)(((int64_t)w + px_step - 1) / px_step), sh = (int)(((int64_t)h + px_step - 1) / px_step);
    const bool lds = words <= kCovisLdsWords;
    auto kernel = packed ? (lds ? k_frames_visible<true, true> : k_frames_visible<true, false>)
                         : (lds ? k_frames_visible<false, true> : k_frames_visible<false, false>);
    // one launch for up to kCovisFrames frames (the image pointers travel as launch arguments)
    for (int f0 = 0; f0 < n_frames; f0 += kCovisFrames) {
        const int nf = n_frames - f0 < kCovisFrames ? n_frames - f0 : kCovisFrames;
        CovisFrames fr = {};
        for (int f = 0; f < nf; ++f) fr.depth[f] = depth[f0 + f];
        psvo::launch(kernel, dim3(div_up(sw, kCovisTile), div_up(sh, kCovisTile), nf), dim3(kCovisThreads), 0, st, h, w,
                     px_step, fr, dirs_cam, poses34 + (int64_t)f0 * 12, n_nodes, static_cast<const PackRec *>(packed),
                     centres, structure, voxel_size, truncation, max_distance, words, bits + (int64_t)f0 * words, flags);
    }
    return check_launch("frames_visible");
}

extern "C" int psvo_visibility_overlap(void *stream, int n_sets, int64_t words, const uint32_t *sets,
                                       const uint32_t *query, int *out) {
    PSVO_REQUIRE(n_sets >= 0 && words > 0, "visibility_overlap: bad sizes n_sets=%d words=%lld", n_sets, (long long)words);
    PSVO_REQUIRE((sets || n_sets == 0) && query && out, "visibility_overlap: null pointer");
    psvo::launch(k_visibility_overlap, dim3(n_sets + 1), dim3(kOvThreads), 0, as_stream(stream), n_sets, words, sets,
                 query, out);
    return check_launch("visibility_overlap");
}
