// Internal helpers shared by the psvo HIP translation units (gfx950 only).
// The ray-query stage's own interface is query.h.
#pragma once

#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/psvo.h"

namespace psvo {

// Kernel-bound timing (the engine's timed regions, psvo_engine_set_timing):
// while a region is armed every kernel launched through psvo::launch gets
// events bound to its own dispatch (hipExtLaunchKernel) — no marker packets
// between the kernels.  Default: every kernel gets a (start, stop) pair and
// a region is the sum of its kernels' spans (what rocprofv3's kernel trace
// reports for them); PSVO_TIMING_SPAN=1: an instance of a region is timed
// from its first kernel's start to its last kernel's end (only the first
// kernel carries a start event; the gaps between the kernels count).  One
// host thread queues a timed step; regions nest (the innermost open instance
// owns a launch).
struct KernelClock {
    static constexpr int kMax = 192, kMaxInst = 64;
    hipEvent_t ev[kMax][2] = {};
    int region[kMax] = {};        // sum mode: the pair's region
    int n = 0;                    // pairs taken since the last full collection
    struct Inst {
        int region, first, last;  // pair indices (−1: no kernel yet)
    } inst[kMaxInst] = {};
    int n_inst = 0;
    int stack[8] = {};            // open instances (span mode) / regions (sum mode), innermost last
    int depth = 0;
    bool sum = false;
    bool overflow = false;        // more launches / instances than slots: the surplus ran untimed
    hipStream_t streams[4] = {};  // the arming engine's streams: launches on any other stream are not its own
    bool owns(hipStream_t st) const {
        for (hipStream_t s : streams)
            if (s == st) return true;
        return false;
    }
};
// engine.cpp: set while an engine with timing on queues a step, on the thread
// that queues it (another thread's launches, e.g. a tracking engine's, are
// never attributed to it)
extern thread_local KernelClock *g_kclock;

// set by the engine around one launch: that launch's completion records this
// event (bound to the dispatch, no marker packet), unless a kernel clock
// needs the slot — then it is recorded right after the launch, or, with
// g_stop_share, not at all: g_stop_bound names the clock's stop event, which
// marks the same completion (the caller waits on that one before the clock
// reuses it)
extern thread_local hipEvent_t g_stop_event;
extern thread_local bool g_stop_share;
extern thread_local hipEvent_t g_stop_bound;

template <typename... KArgs, typename... A>
inline void launch(void (*k)(KArgs...), dim3 grid, dim3 block, uint32_t lds, hipStream_t st, A &&...a) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    KernelClock *c = g_kclock;
    if (c && c->depth > 0 && c->owns(st)) {
        if (c->n < KernelClock::kMax) {
            const int i = c->n++;
            e1 = c->ev[i][1];
            if (c->sum) {
                c->region[i] = c->stack[c->depth - 1];
                e0 = c->ev[i][0];
            } else {
                KernelClock::Inst &I = c->inst[c->stack[c->depth - 1]];
                if (I.first < 0) {
                    I.first = i;
                    e0 = c->ev[i][0];
                }
                I.last = i;
            }
        } else {
            c->overflow = true;
        }
    }
    hipEvent_t late = nullptr;
    if (g_stop_event) {
        if (!e1)
            e1 = g_stop_bound = g_stop_event;
        else if (g_stop_share)
            g_stop_bound = e1;
        else
            late = g_stop_bound = g_stop_event;
        g_stop_event = nullptr;
    }
    hipExtLaunchKernelGGL(k, grid, block, lds, st, e0, e1, 0u, static_cast<KArgs>(a)...);
    if (late) (void)hipEventRecord(late, st);
}

// The binding above, scoped to one launch: `ev` (null: nothing to bind) is
// offered to the next psvo::launch on this thread and all three words are
// cleared when the scope ends, whichever way it ends — an event never stays
// behind for a later, unrelated launch.
struct __attribute__((visibility("hidden"))) StopBind {
    explicit StopBind(hipEvent_t ev, bool share = false) : ev_(ev) {
        g_stop_event = ev;
        g_stop_share = share;
        g_stop_bound = nullptr;
    }
    ~StopBind() {
        g_stop_event = nullptr;
        g_stop_share = false;
        g_stop_bound = nullptr;
    }
    StopBind(const StopBind &) = delete;
    StopBind &operator=(const StopBind &) = delete;
    // a launch took the event: it marks that launch's completion (bound to
    // the dispatch, shared with the clock's, or recorded right after it);
    // false: nothing was launched, the caller records the event itself
    bool consumed() const { return ev_ && g_stop_event == nullptr; }
    // the event that marks the completion (the clock's own when shared)
    hipEvent_t bound() const { return g_stop_bound; }

  private:
    hipEvent_t ev_;
};

// Set the thread-local error message; returns `code` for tail calls.
int set_error(int code, const char *fmt, ...);

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

// Check the most recent launch.  Never exits the process (the reference's
// CUDA_CHECK_ERRORS calls exit(-1), cuda_utils.h:37-48): the binding raises.
int check_launch(const char *what);

// the look-back controls of site 1 (traversal), 2 (sampler) or 4 (sample
// selection): lookback.h's kLbSpinMax and no delay unless
// psvo_debug_set_lookback set them
struct LbCtl;
LbCtl lb_ctl(int site);
// look-back blocks helped (lookback.h) by the selection (query.h: the query's)
int lb_helps_select(int64_t *out1, bool reset);

// multi-tensor Adam launch (optim.hip): per-tensor lr, optional per-tensor
// step numbers (steps: else `step` for all), optional gradient zeroing
int adam_launch(hipStream_t st, int n_tensors, float *const *params, const float *const *grads, float *const *exp_avg,
                float *const *exp_avg_sq, const int64_t *numel, const double *lr, double beta1, double beta2,
                double eps, double weight_decay, int64_t step, const int *zero_grad, const int64_t *steps = nullptr,
                const uint8_t *const *row_flags = nullptr);

constexpr int kWave = 64;
constexpr int kMaxHits = 50;        // voxel_helpers.py:561 (n_max hard-coded)
constexpr int kSamplerG = 200;      // voxel_helpers.py:300
constexpr int kSamplerChunk = 800;  // voxel_helpers.py:331 (4 * G)
constexpr float kMaxDepthFill = 10.0f;  // voxel_helpers.py:24 MAX_DEPTH

inline int div_up(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// records the packed traversal's top start tests per ray (two per lane;
// query_trace.hip top_start, tree_pack.hip k_pt_top): more would cost more
// AABB work than the rounds they save (room0's first 512 records: five times
// the tests of a whole walk)
#ifndef PSVO_PACK_TOP_MAX
#define PSVO_PACK_TOP_MAX 128
#endif
constexpr int kPackTopMax = PSVO_PACK_TOP_MAX;  // a multiple of 64, <= 512

// one octree node as the packed traversal reads it (tree_pack.hip)
struct PackRec {  // 32 B, 16-B aligned
    float4 c;     // centre x, y, z; side (int bits)
    int4 i;       // reference node id, first child record (-1: none), child mask, spare (tree_pack.hip)
};

// one element of the Adam step (k_adam; optim.hip's formulation), shared so
// the fused pose step (pose.hip) computes the same bits
__device__ __forceinline__ void adam_elem(float &p, float g, float &m, float &v, float beta1, float beta2, float omb1,
                                          float omb2, float eps, float wd, float lr_bc1, float bc2_sqrt) {
    if (wd != 0.0f) g = g + wd * p;
    const float mi = beta1 * m + omb1 * g;
    const float vi = beta2 * v + omb2 * g * g;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    p = p - lr_bc1 * mi / denom;
    m = mi;
    v = vi;
}

// torch's floor division of floats (c10 div_floor_floating): a vertex's voxel
// coordinate `points // voxel_size` (mesh_util.py:115, mesh.hip) and a depth
// pixel's voxel key torch.div(points, voxel_size, rounding_mode='floor')
// (mapping.py:264, octree_gpu.hip k_fi_keys) — one copy, so both give torch's bits
__device__ __forceinline__ float div_floor(float a, float b) {
    const float mod = fmodf(a, b);
    float div = (a - mod) / b;
    if (mod != 0.f && ((b < 0.f) != (mod < 0.f))) div -= 1.0f;
    float fl;
    if (div != 0.f) {
        fl = floorf(div);
        if (div - fl > 0.5f) fl += 1.0f;
    } else {
        fl = copysignf(0.f, a / b);
    }
    return fl;
}

// the interpolation forward over the device's sample count m_dev <= m_cap
// (interp.hip; psvo_interp_fwd's arithmetic)
int interp_fwd_dev(hipStream_t st, int64_t m_cap, const int *m_dev, float voxel_size, const int *leaf, const float *t,
                   const int *ray_of_sample, const int *ray_index, const float *rays_o, const float *rays_d,
                   const float *centres, const int *vertex_idx, const float *emb, float *feat);
// the bundle-adjust pose work (pose.hip), over each frame's rays directly
// (ray_rank[r] >= 0: a hit ray; the engine's sums — one fixed order for both
// calls): the frames' pose gradients (k_pose_grad_rays), and the
// look-ahead's whole pose step in one launch, one block per keyframe — the
// gradient, its Adam step when steps[f] >= 1 (k_adam's arithmetic, lr / bc1
// and sqrt(bc2) formed on the host as adam_launch does), then the frame's
// next rays (k_pose_rays_frames) from the updated pose
int pose_grad_frames_rays(hipStream_t st, int n_frames, int64_t rays_per_frame, const int *ray_rank,
                          const float *dirs, const float *g_o, const float *g_d, const float *poses, float *grads);
int pose_step_frames(hipStream_t st, int n_frames, int64_t rays_per_frame, const int *ray_rank, const float *dirs,
                     const float *g_o, const float *g_d, float *poses, float *pose_m, float *pose_v,
                     const int64_t *steps, double lr, double beta1, double beta2, double eps, float *grads,
                     const float *next_dirs, float *rays_o, float *rays_d);

// psvo_criterion_coef split at the count sums (criterion.hip)
int criterion_counts(hipStream_t st, int64_t r_hit, int s_max, float truncation, float max_depth, const int *rank_ray,
                     const float *gt_depth, const float *z_vals, int z_stride, const int *ray_ns, float *workspace,
                     double *sums);
int criterion_coef_from_sums(hipStream_t st, const double *sums, int64_t n_hit, int n_cols, float truncation,
                             float rgb_w, float depth_w, float fs_w, float sdf_w, int flags, float *coef);

// psvo_criterion_coef / psvo_composite_loss reading z from rows of stride
// z_stride >= s_max (the sampler's [R, cap] depth rows, the engine's mapping
// path: no padded [R_hit, S_max] copy; ray_ns: the rows' valid samples, past
// which MAX_DEPTH is implied — the look-back sampler writes no padding)
int criterion_coef_z(void *stream, int64_t r_hit, int s_max, float truncation, float max_depth, const int *rank_ray,
                     const float *gt_depth, const float *z_vals, int z_stride, const int *ray_ns, float rgb_w,
                     float depth_w, float fs_w, float sdf_w, int flags, float *workspace, double *sums, float *coef);
int composite_loss_z(void *stream, int64_t r_hit, int s_max, float truncation, float max_depth, const int *offsets,
                     const int *ray_ns, const float *z_vals, int z_stride, const int *rank_ray, const float *gt_rgb,
                     const float *gt_depth, const float *sdf_s, const float *rgb_s, const float *coef,
                     float *workspace, float *color, float *depth, float *grad_sdf_s, float *grad_rgb_s,
                     bool partials = true,  // false: no loss partials (the loss value is not wanted)
                     const int *cidx = nullptr);  // the sparse decoder's compact sample index (select_samples)
// The sparse decoder's sample selection (composite.hip k_select_samples):
// the samples whose gradients can be non-zero get compact, ray-major indices
// cidx[s] (-1: dropped) — class A (composited: the whole decoder) at
// [0, M_A), class B (only a loss term: the decoder trunk) at [cap, cap + M_B)
// (split = false: every kept sample in class A) —, the classes' compact ray
// offsets offa / offb [R_hit + 1] and compact copies of their features /
// leaf / t / ray ([2 cap] arrays; split: class B's colour rows of rgb_c
// [2 cap][3] are written 0 — their composite weights are 0; src_c [2 cap],
// if not null: each kept sample's index in the step's sample order).  counts[0] = M_A, counts[1] = M_B (the
// compact decoder launches read them on the device), counts[2] |= 8 if the
// look-back wait was abandoned (then both are 0; with host_flag — coherent
// pinned memory — bit 3 is also set there for the host); counts + 4: u64 running
// sums of kept / composited samples and of launches (kSelCountInts ints,
// zeroed once).  desc: select_granules(r_hit) granules, zeroed once; tag
// fresh per launch (≠ 0).
constexpr int kSelCountInts = 10;
int select_samples(hipStream_t st, int64_t r_hit, int s_max, float truncation, float max_depth, const int *offsets,
                   const int *ray_ns, const float *z_vals, int z_stride, const int *rank_ray, const float *gt_depth,
                   const float *sdf_s, const float *feat, const int *leaf, const float *t, const int *ray_of,
                   int64_t cap, bool split, int *cidx, int *offa, int *offb, float *feat_c, int *leaf_c, float *t_c,
                   int *ray_of_c, float *rgb_c, int *src_c, int *counts, unsigned long long *desc, uint32_t tag,
                   int *host_flag = nullptr);
int select_rays_per_wave(int64_t r_hit);
int64_t select_granules(int64_t r_hit);

// ---- the decoder's host glue (decoder.cpp) ----------------------------------
// the device's CU count (256 when it cannot be read); a persistent kernel's grid: min(units, CUs)
int device_cus();
inline int persistent_grid(int64_t units) {
    const int cus = device_cus();
    return (int)(units < cus ? units : cus);
}
// psvo::launch of a kernel with `lds` bytes of dynamic LDS, allowed once per
// kernel (the flag is per instantiation of this template, i.e. per kernel
// address: k_x<true> and k_x<false> each get theirs)
template <auto Kernel, typename... A>
inline void launch_lds(dim3 grid, dim3 block, int lds, hipStream_t st, A &&...a) {
    [[maybe_unused]] static const hipError_t allowed = hipFuncSetAttribute(
        reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    launch(Kernel, grid, block, (uint32_t)lds, st, static_cast<A &&>(a)...);
}

// width-256 decoder (mlp256.hip): sizes, operand images, forward (act /
// masks NULL: inference), backward (gw[0] NULL: δ chain to dfeat only)
int64_t dec256_tiles16(int64_t m);
int64_t dec256_image_floats();
int64_t dec256_act_floats(int64_t m);
int64_t dec256_mask_words(int64_t m);
int64_t dec256_workspace_floats(int64_t m);
// dec: the ten parameter tensors W1, b1, ..., W5, b5 (psvo_map_desc::dec)
int dec256_images(hipStream_t st, const float *const *dec, float *images);
// dec (or null: `images` already holds them): the images are built first.
// rgb, act and masks all null: the sdf trunk only (k_dec256_trunk, the same sdf
// bits).  m_dev: the sample count read on the device (<= m; buffers sized for m)
int dec256_fwd(hipStream_t st, int64_t m, const float *feat, const float *const *dec, float *images, float *sdf,
               float *rgb, float *act, uint64_t *masks, const int *m_dev = nullptr);
struct InterpFuse;
// ip (the mapping engine's width-256 step): the interpolation backward runs
// inside the δ-chain kernel (dfeat is then not stored), as at width 128
int dec256_bwd(hipStream_t st, int64_t m, const float *feat, const float *images, const float *rgb, const float *act,
               const uint64_t *masks, const float *g_sdf, const float *g_rgb, float *dfeat, float *const gw[5],
               float *const gb[5], int accumulate, float *workspace, hipEvent_t dfeat_ready,
               const InterpFuse *ip = nullptr, const int *m_dev = nullptr);

// width-128 decoder (mlp_fwd.hip; dec128_workspace_floats and dec128_bwd:
// mlp_bwd.hip), the same interface plus the sparse decoder's arguments;
// mlp_fwd_interp / mlp_trunk_interp (interp_load.h) are its forwards that
// interpolate their own features
struct H2Rows;
struct TrunkBwd;
int64_t dec128_image_floats();
int64_t dec128_act_floats(int64_t m);
int64_t dec128_mask_words(int64_t m);
int64_t dec128_workspace_floats(int64_t m);
int dec128_images(hipStream_t st, const float *const *dec, float *images);
// rgb null: the sdf only (k_mlp_sdf2, the same sdf bits; inference).  h2: H2Rows below
int dec128_fwd(hipStream_t st, int64_t m, const float *feat, const float *const *dec, float *images, float *sdf,
               float *rgb, float *act, uint64_t *masks, const int *m_dev, const H2Rows *h2);
// the arguments of mlp_bwd below
int dec128_bwd(hipStream_t st, int64_t m, const float *feat, const float *images, const float *rgb, const float *act,
               const uint64_t *masks, const float *g_sdf, const float *g_rgb, float *dfeat, float *const gw[5],
               float *const gb[5], int accumulate, int n_split, float *workspace, hipEvent_t dfeat_ready,
               const InterpFuse *ip, hipStream_t reduce_stream, const int *m_dev, const TrunkBwd *tb,
               const int *x_src);

constexpr int kXchMaxFrames = 64;  // keyframes per psvo_map_step_frames call

// psvo_render_frame (render.hip): its buffers hang off the engine handle
// (engine.cpp: freed with it) and it refuses a data-parallel engine
struct RenderWs;
RenderWs *&engine_render_ws(psvo_engine *e);
bool engine_data_parallel(const psvo_engine *e);
void render_ws_free(RenderWs *ws);  // after the device is idle; null: nothing

// ---- in-launch hand-offs between workgroups --------------------------------
// (cdna_hip_programming.md §6 G16, sc1 form; the per-XCD L2s are not
// coherent).  Every word another workgroup reads in the same launch is stored
// write-through (sc1: a relaxed agent-scope atomic store on a global pointer)
// and read back with sc1 loads, so no release / acquire fence (an L2
// write-back / invalidate) is needed (lookback.h's descriptors).
typedef __attribute__((address_space(1))) int g_i32;
typedef __attribute__((address_space(1))) float g_f32;
typedef __attribute__((address_space(1))) unsigned long long g_u64;
__device__ __forceinline__ void st_wt(int *p, int v) {
    __hip_atomic_store((g_i32 *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_wt(float *p, float v) {
    __hip_atomic_store((g_f32 *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int ld_wt(const int *p) {
    return __hip_atomic_load((g_i32 *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float ld_wt(const float *p) {
    return __hip_atomic_load((g_f32 *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// query statistics to the host: PSVO_STAT_WORDS 8-byte granules {seq, value}
// written by relaxed system-scope stores into coherent pinned memory — each
// word carries its own tag, so no system-scope release (an L2 write-back on
// the critical stream) orders them; the host polls until every tag is seq
__device__ __forceinline__ void stat_to_host(unsigned long long *host, int word, int v, int seq) {
    __hip_atomic_store((g_u64 *)(host + word), ((unsigned long long)(unsigned)seq << 32) | (unsigned)v,
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// the Criterion's backward coefficients from the batch's count sums
// (criterion.py:70-101; k_crit_coef and the sampler's tail share this, so
// both give the same bits): coef = {colour, depth, fs, sdf}; flags PSVO_CRIT_USE_*
__device__ __forceinline__ void crit_coef_from_counts(double n_valid_d, double n_f_d, double n_s_d, double n_hit,
                                                      double n_cols, float rgb_w, float depth_w, float fs_w,
                                                      float sdf_w, float tr, int flags, float *coef) {
    const double n_el = n_hit * n_cols;
    const float n_valid = (float)n_valid_d;
    const float n_f = (float)n_f_d, n_s = (float)n_s_d;
    const float n_tot = n_s + n_f;
    const float fs_weight = 1.0f - n_f / n_tot;
    const float sdf_weight = 1.0f - n_s / n_tot;
    coef[0] = (flags & PSVO_CRIT_USE_COLOR) ? (float)(rgb_w / (3.0 * n_hit)) : 0.0f;
    coef[1] = (flags & PSVO_CRIT_USE_DEPTH) ? depth_w / n_valid : 0.0f;
    coef[2] = (flags & PSVO_CRIT_USE_SDF) ? (float)(2.0 * (double)(fs_w * fs_weight) / n_el) : 0.0f;
    coef[3] = (flags & PSVO_CRIT_USE_SDF) ? (float)(2.0 * (double)(sdf_w * sdf_weight) / n_el) * tr : 0.0f;
}

// The interpolation backward (interp.hip's k_interp_bwd: embedding scatter
// and dL/dx) folded into the width-128 fused decoder backward, per 16-sample
// unit right after its dfeat: grad_emb (zeroed by the caller) += the
// trilinear scatter, gx[M][3] = dL/dx of every sample (psvo_interp_rays_gx
// sums them per ray into d_o / d_d).  Engine only (mlp_bwd `ip`).
struct InterpFuse {
    const int *leaf, *ray_of, *rank_ray, *vertex_idx;
    const float *t, *rays_o, *rays_d, *centres, *emb;
    float voxel_size;
    float *grad_emb;
    float *gx;
    uint8_t *row_flags;  // or null: every embedding row the scatter touches is flagged (sparse-exact Adam)
};

// d_o / d_d of every hit ray from the samples' dL/dx (InterpFuse::gx);
// offsets2 / t2 / gx2 (or null): a second segment of each ray (the sparse
// decoder's class B), summed after the first
int interp_rays_gx(hipStream_t st, int64_t r_hit, const int *offsets, const int *ray_index, const float *t,
                   const float *gx, float *grad_o, float *grad_d, const int *offsets2 = nullptr,
                   const float *t2 = nullptr, const float *gx2 = nullptr);

// psvo_mlp_bwd that records `dfeat_ready` (if not null) on the stream once
// dfeat is written, before the weight-gradient kernels are queued; with `ip`
// (width 128, fused backward) it also runs the interpolation backward and
// dfeat is not stored.  m_dev (width 128; the sparse decoder): the sample
// count is read on the device (select_samples' counts[0] <= m; the buffers
// are sized for m).
// the sparse decoder's class B (k_mlp_trunk_fb after k_mlp_bwd3, width 128:
// the trunk's forward recomputed and its backward in one kernel): its count
// on the device, dL/dsdf, the features and the fused interpolation backward
struct TrunkBwd {
    const int *m_dev;
    const float *g_sdf, *feat;
    const InterpFuse *ip;
    const float *h2 = nullptr;  // or: the step's h2 rows (H2Rows) and each class-B sample's row —
    const int *src = nullptr;   // the W2 layer is read instead of recomputed; feat then holds the
                                // step's rows too (x of sample s: row src[s])
    bool two_launch = false;    // k_mlp_trunk_fb after k_mlp_bwd3 (PSVO_PATH_BWD_TWO_LAUNCH), not one launch
};

// The one-launch backward's split (mlp_bwd.hip k_mlp_bwd3<W, H2>): of n_wg
// workgroups the first nA take class A's units_a 16-sample units, the other
// n_wg − nA class B's units_b, each class split evenly (share w of n: units
// [units·w / n, units·(w + 1) / n)) and run in rounds of four units.  nA
// minimises the modelled finish time
//     max(R_A · a, R_B · b + b0),   R = ceil(ceil(units / n) / 4),
// a : b the per-round cycles of the two bodies and b0 class B's forward of
// round 0, which runs before its loop (s_memtime stamps of both roles inside
// the one launch at the flagship's mix, in k cycles: 75 and 35 — a FULL
// class-B round; k_mlp_trunk_fb's own mean of 26 k over its 3 rounds counts a
// last round of 2 or 3 units; profiles/bwd_ab_stamps.txt).  R_A does not grow
// with nA and R_B does not shrink: the minimum is at the crossing, found by
// bisection — integers only, so the kernel's workgroups, the slab sum and the
// host agree.  An empty class gets no workgroup, a present one at least one;
// n_wg == 1 with both present has no split (the caller launches twice).
struct BwdSplitCost {
    int a, b, b0;
};
constexpr BwdSplitCost kBwdSplitCost = {75, 35, 16};
BwdSplitCost bwd_split_cost();  // kBwdSplitCost unless psvo_debug_set_bwd_split changed it (capi.cpp)
__host__ __device__ inline int64_t bwd_split_rounds(int64_t units, int n) { return ((units + n - 1) / n + 3) / 4; }
__host__ __device__ inline int bwd_split_na(int64_t units_a, int64_t units_b, int n_wg, BwdSplitCost c) {
    if (units_a <= 0) return 0;
    if (units_b <= 0 || n_wg < 2) return n_wg;
    auto t_a = [&](int n) { return bwd_split_rounds(units_a, n) * c.a; };
    auto t_b = [&](int n) { return bwd_split_rounds(units_b, n_wg - n) * c.b + c.b0; };
    int lo = 1, hi = n_wg - 1;  // the smallest n in [1, n_wg − 1] with t_a(n) <= t_b(n), else n_wg − 1
    while (lo < hi) {
        const int mid = (lo + hi) / 2;
        if (t_a(mid) <= t_b(mid))
            hi = mid;
        else
            lo = mid + 1;
    }
    // left of the crossing class A finishes last, from it on class B (or lo is the last candidate)
    auto t = [&](int n) {
        const int64_t ta = t_a(n), tb = t_b(n);
        return ta > tb ? ta : tb;
    };
    return lo > 1 && t(lo - 1) < t(lo) ? lo - 1 : lo;
}
// grads: the ten parameter gradients gW1, gb1, ..., gW5, gb5 (the order of
// psvo_map_desc::dec); a null array or null entries: the δ chain / dfeat only
// (frozen decoder).  The weights themselves are not read: `images` holds them.
int mlp_bwd(void *stream, int64_t m, int width, const float *feat, const float *images, const float *rgb,
            const float *act, const uint64_t *masks, const float *g_sdf, const float *g_rgb, float *dfeat,
            float *const *grads, int accumulate, int n_split, float *workspace, hipEvent_t dfeat_ready,
            const InterpFuse *ip = nullptr, hipStream_t reduce_stream = nullptr, const int *m_dev = nullptr,
            const TrunkBwd *tb = nullptr,
            const int *x_src = nullptr);  // x_src (width 128): sample s's x is row x_src[s] of feat
// whether mlp_bwd can take `ip` for this width (the fused width-128 backward is built and selected)
bool mlp_bwd_fuses_interp(int width);
// the look-ahead's split tail (psvo_map_step_frames): the weight-gradient
// slab sum and the optimiser on the side stream beside the next query — width
// 128 only (the width-256 weight-gradient kernel holds every CU)
bool mlp_bwd_split_tail(int width);

// the decoder's LDS operand images (k_mlp_prep) on their own, and
// psvo_mlp_fwd without rebuilding them (the engine prepares them on its aux
// stream beside the sampler / interpolation kernels)
// (dec: the ten parameter tensors W1, b1, ..., W5, b5, psvo_map_desc::dec)
int mlp_images(void *stream, int width, const float *const *dec, float *images);
// the sparse decoder's h2 hand-over (width 128): the sdf-only forward
// (rgb == nullptr) writes every sample's h2 as row-major rows into `out`
// [m][128]; the full forward (k_mlp_fwd2) reads sample s's h2 from row src[s]
// of `rows` instead of recomputing the W2 layer (the same instructions made
// it: the same bits) — and its x from row src[s] of `feat` (the step's
// features, no compact copy)
struct H2Rows {
    float *out = nullptr;
    const float *rows = nullptr;
    const int *src = nullptr;
};
int mlp_fwd_prepared(void *stream, int64_t m, int width, const float *feat, float *images, float *sdf, float *rgb,
                     float *act, uint64_t *masks, const int *m_dev = nullptr,
                     const H2Rows *h2 = nullptr);  // m_dev: as mlp_bwd (width 128)
// psvo_mlp_fwd with the decoder as one array (it builds the images first)
int mlp_fwd(void *stream, int64_t m, int width, const float *feat, const float *const *dec, float *images, float *sdf,
            float *rgb, float *act, uint64_t *masks);

}  // namespace psvo

#define PSVO_REQUIRE(cond, ...)                                       \
    do {                                                              \
        if (!(cond)) return ::psvo::set_error(PSVO_E_INVALID, __VA_ARGS__); \
    } while (0)
