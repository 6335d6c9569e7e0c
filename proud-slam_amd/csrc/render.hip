// Whole-frame renderer (psvo_render_frame): colour / depth / hit-mask images
// of the map from world rays — Tracking.render_debug_images and a map
// evaluation at full resolution — as a tiled, inference-only pipeline.
//
// Reference: render_helpers.render_rays (render_helpers.py:363-556) on the
// whole ray batch, then fill_in(…, 0) per output.
//
//   pass 1 (frame)   traversal + hit ranks of every ray; ONE read-back of
//                    R_hit, P, max ⌈Σ/step⌉ — the sampler's layout [200, K',
//                    max_steps] and the tile workspace follow from them
//   pass 2 (frame)   counting pre-pass: the range sampler over every tile,
//                    keeping only the per-ray sample counts → S_max of the
//                    FRAME on the device (a ray's padded sdf row ends in an
//                    sdf = 1 element iff its count is below it); skipped when
//                    the frame is one tile (pass 3's own sampler gives it)
//   pass 3 (tile)    range sampler (the hit rows of the tile inside the
//                    frame's layout: the same noise slots as one big batch)
//                    → ray-major compaction → sdf trunk on every sample, the
//                    features interpolated in the operand load (width 128;
//                    interp_load.h) → z_min and the composited set per ray →
//                    scan → compact (leaf, t, ray) of the composited samples
//                    → the whole decoder on those only → weights, colour,
//                    depth per ray, scattered through rank_ray into the images
//
// Everything sized by samples is one tile allocation carved by TileLayout
// (psvo_render_tile_bytes is its size); ray-sized buffers are whole-frame.
// Every kernel after pass 1 reads its sample counts on the device, so the
// host reads back once per frame (and once more for the statistics).
#include <hip/hip_runtime.h>

#include "interp_load.h"
#include "psvo_common.h"
#include "query.h"
#include "select_common.h"

namespace psvo {

// frame-sized buffers
enum RSlot { kRStats, kRHitIdx, kRHitT0, kRHitT1, kRRayNv, kRRayDsum, kRRayRank, kRRankRay, kRBlkOut, kRRayNs,
             kRFrame, kRImages, kRTile, kRSlots };

struct RenderWs {
    void *p[kRSlots] = {};
    size_t cap[kRSlots] = {};
    int *host = nullptr;  // pinned: the statistics read-backs
};

void render_ws_free(RenderWs *ws) {
    if (!ws) return;
    for (void *q : ws->p)
        if (q) (void)hipFree(q);
    if (ws->host) (void)hipHostFree(ws->host);
    delete ws;
}

namespace {

constexpr int64_t kDefaultTileRays = 16384;
constexpr int kSelWavesR = 4;  // rays (waves) per workgroup of the per-ray kernels

// frame accumulators on the device (ints): S_max, then u64 M and M_composited
enum { kFSmax = 0, kFM = 2, kFMc = 4, kFWords = 8 };

inline size_t al256(size_t b) { return (b + 255) / 256 * 256; }

// The tile workspace: rows hit rays × max_steps sample slots.  The sampler's
// rows (s_idx / s_depth) are dead once compacted, so the composited samples'
// compact leaf / t reuse them.
struct TileLayout {
    size_t s_idx, s_depth, leaf, t, ray_of, sdf, ray_c, sdf_c, rgb_c, feat, offsets, nc, offc, zmin, total;
    TileLayout(int64_t rows, int max_steps, int width) {
        const size_t slots = (size_t)rows * (size_t)max_steps;
        size_t o = 0;
        auto take = [&](size_t bytes) {
            const size_t at = o;
            o += al256(bytes);
            return at;
        };
        s_idx = take(slots * 4);    // → leaf_c
        s_depth = take(slots * 4);  // → t_c
        leaf = take(slots * 4);
        t = take(slots * 4);
        ray_of = take(slots * 4);
        sdf = take(slots * 4);
        ray_c = take(slots * 4);
        sdf_c = take(slots * 4);
        rgb_c = take(slots * 12);
        feat = take(width == 256 ? slots * 64 : 0);  // width 256: the per-tile feature rows
        offsets = take(((size_t)rows + 1) * 4);
        nc = take((size_t)rows * 4);
        offc = take(((size_t)rows + 1) * 4);
        zmin = take((size_t)rows * 4);
        total = o;
    }
};

__device__ __forceinline__ float wsum_f(float v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}
__device__ __forceinline__ float sigm_f(float x) { return 1.0f / (1.0f + expf(-x)); }

// after a tile's sampler: its S_max / M into the frame's accumulators
__global__ void k_render_accum(const int *__restrict__ stats, int *__restrict__ fr, int with_m) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    fr[kFSmax] = max(fr[kFSmax], stats[PSVO_STAT_S_MAX]);
    if (with_m) *reinterpret_cast<unsigned long long *>(fr + kFM) += (unsigned long long)stats[PSVO_STAT_M];
}

// Selection for rendering, one wave per hit row of the tile: z_min with the
// FRAME's S_max (select_common.h: k_select_samples' definition) and the
// number of composited samples z < z_min + tr.  No loss masks, no class B.
__global__ __launch_bounds__(64 * kSelWavesR) void k_render_select_count(int n_rows, float tr,
                                                                         const int *__restrict__ offsets,
                                                                         const float *__restrict__ t,
                                                                         const float *__restrict__ sdf_s,
                                                                         const int *__restrict__ frame,
                                                                         float *__restrict__ zmin_out,
                                                                         int *__restrict__ nc_out) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * kSelWavesR + (threadIdx.x >> 6);
    if (r >= n_rows) return;
    const int off = offsets[r], ns = offsets[r + 1] - off;
    const int s_max = frame[kFSmax];
    const float *z = t + off;
    const float zmin = sel::sel_zmin(lane, s_max, ns, off, z, sdf_s);
    int nc = 0;
    for (int s = lane; s < ns; s += 64) nc += z[s] < zmin + tr;
#pragma unroll
    for (int k = 32; k > 0; k >>= 1) nc += __shfl_xor(nc, k, 64);
    if (lane == 0) {
        zmin_out[r] = zmin;
        nc_out[r] = nc;
    }
}

// the composited samples' (leaf, t, ray) at their compact, ray-major places
__global__ __launch_bounds__(64 * kSelWavesR) void k_render_select_emit(int n_rows, float tr,
                                                                        const int *__restrict__ offsets,
                                                                        const int *__restrict__ offc,
                                                                        const int *__restrict__ leaf,
                                                                        const float *__restrict__ t,
                                                                        const float *__restrict__ zmin_in,
                                                                        int *__restrict__ leaf_c,
                                                                        float *__restrict__ t_c,
                                                                        int *__restrict__ ray_c,
                                                                        int *__restrict__ frame) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * kSelWavesR + (threadIdx.x >> 6);
    if (r == 0 && lane == 0)  // the tile's composited samples into the frame's count
        *reinterpret_cast<unsigned long long *>(frame + kFMc) += (unsigned long long)offc[n_rows];
    if (r >= n_rows) return;
    const int off = offsets[r], ns = offsets[r + 1] - off;
    const float zmin = zmin_in[r];
    const uint64_t below = (1ull << lane) - 1ull;
    int base = offc[r];
    for (int s0 = 0; s0 < ns; s0 += 64) {
        const int s = s0 + lane;
        const float zs = s < ns ? t[off + s] : 0.f;
        const bool keep = s < ns && zs < zmin + tr;
        const uint64_t b = __ballot(keep);
        if (keep) {
            const int k = base + __popcll(b & below);
            leaf_c[k] = leaf[off + s];
            t_c[k] = zs;
            ray_c[k] = r;
        }
        base += __popcll(b);
    }
}

// Compositing of one hit row per wave (k_composite_fwd's arithmetic and
// summation order: lane-strided over the ray's own sample index, then the
// wave butterfly — independent of the tile): normalised weights σ(s/tr)·
// σ(−s/tr)/(Σ + 1e-8) over the composited samples, colour Σ w·c (c at the
// sample's compact row), depth Σ w·z; scattered to the ray's image row.
__global__ __launch_bounds__(64 * kSelWavesR) void k_render_composite(int n_rows, float tr,
                                                                      const int *__restrict__ offsets,
                                                                      const int *__restrict__ offc,
                                                                      const float *__restrict__ t,
                                                                      const float *__restrict__ sdf_s,
                                                                      const float *__restrict__ rgb_c,
                                                                      const float *__restrict__ zmin_in,
                                                                      const int *__restrict__ rank_ray,
                                                                      float *__restrict__ color,
                                                                      float *__restrict__ depth,
                                                                      float *__restrict__ zmin_out,
                                                                      uint8_t *__restrict__ mask) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * kSelWavesR + (threadIdx.x >> 6);
    if (r >= n_rows) return;
    const int off = offsets[r], ns = offsets[r + 1] - off;
    const float zmin = zmin_in[r];
    const float *z = t + off;
    const float *sd = sdf_s + off;
    float tot = 0.f;
    for (int s = lane; s < ns; s += 64) {
        const float a = sd[s] / tr;
        float w = sigm_f(a) * sigm_f(-a);
        w = (z[s] < zmin + tr) ? w : 0.0f;
        tot += w;
    }
    tot = wsum_f(tot) + 1e-8f;
    const uint64_t below = (1ull << lane) - 1ull;
    int base = offc[r];
    float cr = 0.f, cg = 0.f, cb = 0.f, dd = 0.f;
    for (int s0 = 0; s0 < ns; s0 += 64) {
        const int s = s0 + lane;
        const bool in = s < ns;
        const float zs = in ? z[s] : 0.f;
        const bool keep = in && zs < zmin + tr;
        const uint64_t b = __ballot(keep);
        if (keep) {
            const float a = sd[s] / tr;
            const float w = sigm_f(a) * sigm_f(-a) / tot;
            const float *c = rgb_c + (int64_t)(base + __popcll(b & below)) * 3;
            cr += w * c[0];
            cg += w * c[1];
            cb += w * c[2];
            dd += w * zs;
        }
        base += __popcll(b);
    }
    cr = wsum_f(cr);
    cg = wsum_f(cg);
    cb = wsum_f(cb);
    dd = wsum_f(dd);
    if (lane == 0) {
        const int64_t o = rank_ray[r];
        color[o * 3 + 0] = cr;
        color[o * 3 + 1] = cg;
        color[o * 3 + 2] = cb;
        depth[o] = dd;
        if (zmin_out) zmin_out[o] = zmin;
        mask[o] = 1;
    }
}

void *ws_buf(RenderWs &w, hipStream_t st, int slot, size_t bytes, int *rc) {
    if (bytes == 0) bytes = 16;
    if (w.cap[slot] >= bytes) return w.p[slot];
    if (w.p[slot]) {  // queued kernels may still read the old buffer
        (void)hipStreamSynchronize(st);
        (void)hipFree(w.p[slot]);
        w.p[slot] = nullptr;
        w.cap[slot] = 0;
    }
    if (hipMalloc(&w.p[slot], bytes) != hipSuccess) {
        *rc = set_error(PSVO_E_LAUNCH, "render_frame: hipMalloc(%zu) failed", bytes);
        return nullptr;
    }
    w.cap[slot] = bytes;
    return w.p[slot];
}

#define R_BUF(T, name, slot, bytes)                                        \
    T *name = reinterpret_cast<T *>(ws_buf(*ws, st, slot, (bytes), &rc)); \
    if (!name) return rc;
#define R_CALL(x)                       \
    do {                                \
        const int _rc = (x);            \
        if (_rc != PSVO_OK) return _rc; \
    } while (0)

int64_t tile_bytes(int64_t tile_rays, int max_steps, int width) {
    if (tile_rays <= 0 || max_steps <= 0 || (width != 128 && width != 256)) return -1;
    return (int64_t)TileLayout(tile_rays, max_steps, width).total;
}

}  // namespace
}  // namespace psvo

using namespace psvo;

extern "C" int64_t psvo_render_tile_bytes(int64_t tile_rays, int max_steps, int width) {
    return tile_bytes(tile_rays, max_steps, width);
}

extern "C" int psvo_render_frame(psvo_engine *e, void *stream, const psvo_map_desc *d, int64_t n_rays,
                                 const float *rays_o, const float *rays_d, const float *noise, uint64_t seed,
                                 const psvo_render_opts *opts, float *color, float *depth, float *z_min,
                                 uint8_t *mask, int64_t *stats_out) {
    PSVO_REQUIRE(e && d, "render_frame: engine / map descriptor required");
    PSVO_REQUIRE(!engine_data_parallel(e), "render_frame: a data-parallel engine cannot render (single GPU only)");
    PSVO_REQUIRE(n_rays >= 0 && n_rays <= (int64_t)1 << 30, "render_frame: n_rays %lld out of range", (long long)n_rays);
    PSVO_REQUIRE(d->width == 128 || d->width == 256, "render_frame: width %d unsupported (128, 256)", d->width);
    PSVO_REQUIRE(d->centres && d->structure && d->vertex_idx && d->emb && d->n_nodes > 0,
                 "render_frame: map arrays required");
    for (int i = 0; i < 10; ++i) PSVO_REQUIRE(d->dec[i], "render_frame: decoder parameter %d is null", i);
    PSVO_REQUIRE(d->voxel_size > 0.f && d->step_size > 0.f && d->truncation > 0.f && d->max_distance > 0.f,
                 "render_frame: voxel_size / step_size / truncation / max_distance must be > 0");
    const bool query_only = opts && (opts->flags & PSVO_RENDER_QUERY_ONLY);
    PSVO_REQUIRE(n_rays == 0 || (rays_o && rays_d), "render_frame: rays required");
    PSVO_REQUIRE(query_only || n_rays == 0 || (color && depth && mask), "render_frame: color / depth / mask required");
    const int64_t tile_rays = opts && opts->tile_rays > 0 ? opts->tile_rays : kDefaultTileRays;
    hipStream_t st = as_stream(stream);
    int64_t so[PSVO_RENDER_STAT_WORDS] = {};
    auto finish = [&]() {
        if (stats_out)
            for (int i = 0; i < PSVO_RENDER_STAT_WORDS; ++i) stats_out[i] = so[i];
        return PSVO_OK;
    };
    if (n_rays == 0) return finish();
    const int64_t R = n_rays;
    if (!query_only) {  // fill_in(…, 0): the rows of rays that hit nothing
        if (hipMemsetAsync(color, 0, (size_t)R * 12, st) != hipSuccess ||
            hipMemsetAsync(depth, 0, (size_t)R * 4, st) != hipSuccess ||
            hipMemsetAsync(mask, 0, (size_t)R, st) != hipSuccess ||
            (z_min && hipMemsetAsync(z_min, 0, (size_t)R * 4, st) != hipSuccess))
            return set_error(PSVO_E_LAUNCH, "render_frame: memset failed");
    }
    RenderWs *&slot = engine_render_ws(e);
    if (!slot) slot = new RenderWs();
    RenderWs *ws = slot;
    if (!ws->host && hipHostMalloc(reinterpret_cast<void **>(&ws->host), 64 * sizeof(int), 0) != hipSuccess)
        return set_error(PSVO_E_LAUNCH, "render_frame: pinned allocation failed");
    int rc = PSVO_OK;
    // ---- pass 1: traversal, ranks, statistics
    const size_t hit_b = (size_t)R * kMaxHits * 4;
    const size_t blk_b = (size_t)div_up(R, 4) * 2 * sizeof(int);
    R_BUF(int, stats, kRStats, PSVO_STAT_WORDS * sizeof(int));
    R_BUF(int, hit_idx, kRHitIdx, hit_b);
    R_BUF(float, hit_t0, kRHitT0, hit_b);
    R_BUF(float, hit_t1, kRHitT1, hit_b);
    R_BUF(int, ray_nv, kRRayNv, (size_t)R * 4);
    R_BUF(float, ray_dsum, kRRayDsum, (size_t)R * 4);
    R_BUF(int, ray_rank, kRRayRank, (size_t)R * 4);
    R_BUF(int, rank_ray, kRRankRay, (size_t)R * 4);
    R_BUF(int, blk_out, kRBlkOut, blk_b);
    R_BUF(int, ray_ns, kRRayNs, (size_t)R * 4);
    R_BUF(int, frame, kRFrame, kFWords * sizeof(int));
    so[PSVO_RENDER_STAT_RAY_BYTES] =
        (int64_t)(3 * hit_b + 5 * (size_t)R * 4 + blk_b + (PSVO_STAT_WORDS + kFWords) * sizeof(int));
    if (hipMemsetAsync(stats, 0, PSVO_STAT_WORDS * sizeof(int), st) != hipSuccess ||
        hipMemsetAsync(frame, 0, kFWords * sizeof(int), st) != hipSuccess)
        return set_error(PSVO_E_LAUNCH, "render_frame: memset failed");
    R_CALL(intersect_ranked(st, R, rays_o, rays_d, d->centres, d->structure, d->voxel_size, d->max_distance,
                            d->step_size, hit_idx, hit_t0, hit_t1, ray_nv, ray_dsum, stats, ray_rank, rank_ray,
                            static_cast<const PackRec *>(d->packed), blk_out, nullptr, 0, nullptr, nullptr,
                            d->n_nodes));
    if (hipMemcpyAsync(ws->host, stats, PSVO_STAT_WORDS * sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return set_error(PSVO_E_LAUNCH, "render_frame: statistics read-back failed");
    if (ws->host[PSVO_STAT_FLAGS] & kStatFlagDfsOverflow)
        return set_error(PSVO_E_OVERFLOW, "render_frame: traversal stack overflow");
    const int P = ws->host[PSVO_STAT_P];
    const int64_t r_hit = ws->host[PSVO_STAT_R_HIT];
    const int max_steps = ws->host[PSVO_STAT_MAX_CEIL] + P;
    so[PSVO_RENDER_STAT_R_HIT] = r_hit;
    so[PSVO_RENDER_STAT_P] = P;
    if (r_hit <= 0 || P <= 0) {  // a view that looks away from the map: all outputs 0
        so[PSVO_RENDER_STAT_R_HIT] = 0;
        return finish();
    }
    PSVO_REQUIRE(max_steps > 0, "render_frame: max_steps %d", max_steps);
    so[PSVO_RENDER_STAT_MAX_STEPS] = max_steps;
    so[PSVO_RENDER_STAT_N_TILES] = (r_hit + tile_rays - 1) / tile_rays;
    so[PSVO_RENDER_STAT_TILE_BYTES] = tile_bytes(tile_rays, max_steps, d->width);
    if (query_only) return finish();
    // ---- the tile workspace (a frame with fewer hit rays than a tile: its rows only)
    const int64_t rows = tile_rays < r_hit ? tile_rays : r_hit;
    const int64_t slots = rows * max_steps;
    // (32-bit sample offsets; width 256: dec256's feature offsets)
    PSVO_REQUIRE(slots <= (d->width == 256 ? ((int64_t)1 << 31) / 256 : (int64_t)1 << 30),
                 "render_frame: a tile of %lld rays x %d steps is too large; lower tile_rays", (long long)rows,
                 max_steps);
    const TileLayout tl(rows, max_steps, d->width);
    R_BUF(char, tile, kRTile, tl.total);
    int *s_idx = reinterpret_cast<int *>(tile + tl.s_idx), *leaf = reinterpret_cast<int *>(tile + tl.leaf);
    int *ray_of = reinterpret_cast<int *>(tile + tl.ray_of), *ray_c = reinterpret_cast<int *>(tile + tl.ray_c);
    int *offsets = reinterpret_cast<int *>(tile + tl.offsets), *nc = reinterpret_cast<int *>(tile + tl.nc);
    int *offc = reinterpret_cast<int *>(tile + tl.offc);
    float *s_depth = reinterpret_cast<float *>(tile + tl.s_depth), *tt = reinterpret_cast<float *>(tile + tl.t);
    float *sdf = reinterpret_cast<float *>(tile + tl.sdf), *sdf_c = reinterpret_cast<float *>(tile + tl.sdf_c);
    float *rgb_c = reinterpret_cast<float *>(tile + tl.rgb_c), *feat = reinterpret_cast<float *>(tile + tl.feat);
    float *zmin_t = reinterpret_cast<float *>(tile + tl.zmin);
    int *leaf_c = s_idx;      // (the sampler's rows are dead once compacted)
    float *t_c = s_depth;
    // ---- decoder operand images (once per frame)
    const int64_t img_floats = psvo_mlp_image_floats_w(d->width);
    R_BUF(float, images, kRImages, (size_t)img_floats * sizeof(float));
    R_CALL(mlp_images(stream, d->width, d->dec, images));
    const int n_tiles = (int)so[PSVO_RENDER_STAT_N_TILES];
    auto sample_tile = [&](int64_t row0, int64_t n) {
        return psvo_sample_rays_range(stream, row0, n, rows, max_steps, rank_ray, hit_idx, hit_t0, hit_t1, ray_dsum,
                                      d->step_size, noise, seed, stats, s_idx, s_depth, nullptr, ray_ns + row0,
                                      offsets);
    };
    // ---- pass 2: the frame's S_max (and M) from a counting pre-pass of the sampler
    // (a single tile is the frame: its own sampler pass gives both, below)
    for (int k = 0; k < n_tiles && n_tiles > 1; ++k) {
        const int64_t row0 = (int64_t)k * tile_rays, n = r_hit - row0 < tile_rays ? r_hit - row0 : tile_rays;
        R_CALL(sample_tile(row0, n));
        psvo::launch(k_render_accum, dim3(1), dim3(1), 0, st, stats, frame, 1);
    }
    R_CALL(check_launch("render_frame (count)"));
    // ---- pass 3: the tiles
    const float tr = d->truncation;
    for (int k = 0; k < n_tiles; ++k) {
        const int64_t row0 = (int64_t)k * tile_rays, n = r_hit - row0 < tile_rays ? r_hit - row0 : tile_rays;
        const int *ray_index = rank_ray + row0;  // tile row → original ray
        const int *m_dev = stats + PSVO_STAT_M;  // the tile's sample count (k_scan_samples)
        R_CALL(sample_tile(row0, n));
        if (n_tiles == 1) psvo::launch(k_render_accum, dim3(1), dim3(1), 0, st, stats, frame, 1);
        R_CALL(compact_rays(st, n, max_steps, s_idx, s_depth, offsets, leaf, tt, ray_of));
        const InterpSrc ip{leaf, ray_of, ray_index, d->vertex_idx, tt, rays_o, rays_d, d->centres,
                           reinterpret_cast<const float4 *>(d->emb), d->voxel_size};
        if (d->width == 128) {
            R_CALL(mlp_fwd_interp(st, slots, m_dev, ip, images, sdf, nullptr));
        } else {
            R_CALL(interp_fwd_dev(st, slots, m_dev, d->voxel_size, leaf, tt, ray_of, ray_index, rays_o, rays_d,
                                  d->centres, d->vertex_idx, d->emb, feat));
            R_CALL(dec256_fwd(st, slots, feat, nullptr, images, sdf, nullptr, nullptr, nullptr, m_dev));
        }
        const dim3 rg(div_up(n, kSelWavesR)), rb(64 * kSelWavesR);
        psvo::launch(k_render_select_count, rg, rb, 0, st, (int)n, tr, offsets, tt, sdf, frame, zmin_t, nc);
        R_CALL(check_launch("render_frame (select)"));
        R_CALL(psvo_scan_counts(stream, n, nc, offc));
        psvo::launch(k_render_select_emit, rg, rb, 0, st, (int)n, tr, offsets, offc, leaf, tt, zmin_t, leaf_c, t_c,
                     ray_c, frame);
        R_CALL(check_launch("render_frame (compact)"));
        const int *mc_dev = offc + n;  // the tile's composited samples
        const InterpSrc ipc{leaf_c, ray_c, ray_index, d->vertex_idx, t_c, rays_o, rays_d, d->centres,
                            reinterpret_cast<const float4 *>(d->emb), d->voxel_size};
        if (d->width == 128) {
            R_CALL(mlp_fwd_interp(st, slots, mc_dev, ipc, images, sdf_c, rgb_c));
        } else {
            R_CALL(interp_fwd_dev(st, slots, mc_dev, d->voxel_size, leaf_c, t_c, ray_c, ray_index, rays_o, rays_d,
                                  d->centres, d->vertex_idx, d->emb, feat));
            R_CALL(dec256_fwd(st, slots, feat, nullptr, images, sdf_c, rgb_c, nullptr, nullptr, mc_dev));
        }
        psvo::launch(k_render_composite, rg, rb, 0, st, (int)n, tr, offsets, offc, tt, sdf, rgb_c, zmin_t, ray_index,
                     color, depth, z_min, mask);
        R_CALL(check_launch("render_frame (composite)"));
    }
    if (!stats_out) return PSVO_OK;
    if (hipMemcpyAsync(ws->host + 32, frame, kFWords * sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return set_error(PSVO_E_LAUNCH, "render_frame: statistics read-back failed");
    so[PSVO_RENDER_STAT_S_MAX] = ws->host[32 + kFSmax];
    so[PSVO_RENDER_STAT_M] = (int64_t) * reinterpret_cast<unsigned long long *>(ws->host + 32 + kFM);
    so[PSVO_RENDER_STAT_M_COMPOSITED] = (int64_t) * reinterpret_cast<unsigned long long *>(ws->host + 32 + kFMc);
    return finish();
}
