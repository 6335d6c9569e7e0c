// One render-and-optimise iteration per C call: the render paths after the
// query (render_track, render_map), the mapping step as a schedule of named
// stages (map_step_impl) and the tracking step.
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "engine_internal.h"
#include "interp_load.h"

using namespace psvo;
using namespace psvo::eng;

namespace {

// the per-sample arrays a step's kernels read: every sample of the batch
// after the render; the kept ones after the sparse selection (step_select)
struct Samples {
    int *offsets = nullptr, *leaf = nullptr, *ray_of = nullptr;
    float *tt = nullptr, *feat = nullptr, *rgb_s = nullptr, *act = nullptr;
    uint64_t *masks = nullptr;
};

// what one render (query + forward) leaves for the loss and the backward
struct Render {
    int64_t r_hit = 0, m = 0;
    int s_max = 0;
    int *rank_ray = nullptr, *ray_rank = nullptr, *ray_ns = nullptr;  // per ray (the query set's)
    float *z_vals = nullptr, *images = nullptr, *sdf_s = nullptr;
    Samples s;  // per sample
    float *sdf = nullptr, *weights = nullptr, *color = nullptr, *depth = nullptr;  // render_track's compositing
    bool z_recorded = false;  // e->z_ready marks the sample compaction on st (aux has not waited yet)
    int z_stride = 0;         // row stride of z_vals: s_max (padded copy) or the sampler's row capacity
    bool sparse = false;      // the decoder ran the sdf trunk only (sdf_s): the rest after select_samples
    float *h2 = nullptr;      // (sparse, width 128) every sample's h2 rows [m][128] from the sdf trunk
};

constexpr int64_t kW128 = 128;  // h2 row length (the width-128 decoder)
constexpr int kCritFlags = PSVO_CRIT_USE_COLOR | PSVO_CRIT_USE_DEPTH | PSVO_CRIT_USE_SDF;

// the read-back's sizes and the query set's per-ray rows into `o`
void render_begin(QuerySet &qset, const Readback &rb, Render &o) {
    o.r_hit = rb.r_hit;
    o.m = rb.m;
    o.s_max = rb.s_max;
    o.rank_ray = static_cast<int *>(qset.a.p[kRankRay]);
    o.ray_rank = static_cast<int *>(qset.a.p[kRayRank]);
    o.ray_ns = static_cast<int *>(qset.a.p[kRayNs]);
    o.s.offsets = static_cast<int *>(qset.a.p[kOffsets]);
}

// the padded [R_hit, S_max] copy the autograd path makes (k_sample_points):
// z and the samples' leaf / t / ray into the step's own buffers
int padded_samples(psvo_engine *e, hipStream_t st, QuerySet &qset, Render &o) {
    int rc = PSVO_OK;
    const size_t RS = (size_t)o.r_hit * o.s_max;
    ENG_BUF(float, z_b, kZ, RS * sizeof(float));
    ENG_BUF(uint8_t, smask, kMask, RS);
    mark(e, st, PSVO_TIME_POINTS, 0);
    ENG_CALL(psvo_sample_points(st, o.r_hit, o.s_max, qset.max_steps, static_cast<const int *>(qset.a.p[kSIdx]),
                                static_cast<const float *>(qset.a.p[kSDepth]), o.ray_ns, o.s.offsets, o.s.leaf, o.s.tt,
                                o.s.ray_of, z_b, smask));
    mark(e, st, PSVO_TIME_POINTS, 1);
    o.z_vals = z_b;
    o.z_stride = o.s_max;
    return PSVO_OK;
}

// render_rays (render_helpers.py:363-556) on the device after the query, as
// the tracking step wants it: everything sized by the read-back — the padded
// sample copy, interpolation, the whole decoder (masks only, no activations:
// the map is frozen) and compositing.  One GPU (psvo_track_step refuses an
// exchange), one stream.
int render_track(psvo_engine *e, hipStream_t st, const psvo_map_desc *d, QuerySet &qset, const float *rays_o,
                 const float *rays_d, int *stats_out, const char *who, Render &o) {
    int rc = PSVO_OK;
    void *stream = st;
    ENG_BUF(float, images, kImages, psvo_mlp_image_floats_w(d->width) * sizeof(float));
    e->images_next = false;
    Readback rb;
    ENG_CALL(query_readback(e, qset, false, stats_out, who, rb));
    render_begin(qset, rb, o);
    const int64_t M = o.m, r_hit = o.r_hit;
    ENG_BUF(int, leaf, kLeaf, M * sizeof(int));
    ENG_BUF(float, tt, kT, M * sizeof(float));
    ENG_BUF(int, ray_of, kRayOf, M * sizeof(int));
    ENG_BUF(float, feat, kFeat, M * 16 * sizeof(float));
    o.s.leaf = leaf;
    o.s.tt = tt;
    o.s.ray_of = ray_of;
    o.s.feat = feat;
    ENG_CALL(padded_samples(e, st, qset, o));
    // ---- forward: interpolation, decoder (after the previous mapping step's
    // optimiser step when its tail ran on aux)
    ENG_CALL(join_adam(e, st, who));
    mark(e, st, PSVO_TIME_INTERP_FWD, 0);
    ENG_CALL(psvo_interp_fwd(stream, M, 16, d->voxel_size, leaf, tt, ray_of, o.rank_ray, rays_o, rays_d, d->centres,
                             d->vertex_idx, d->emb, feat));
    mark(e, st, PSVO_TIME_INTERP_FWD, 1);
    ENG_BUF(float, sdf_s, kSdfS, M * sizeof(float));
    ENG_BUF(float, rgb_s, kRgbS, M * 3 * sizeof(float));
    ENG_BUF(uint64_t, masks, kMasks, (size_t)psvo_mlp_mask_words(M, d->width) * sizeof(uint64_t));
    mark(e, st, PSVO_TIME_MLP_FWD, 0);
    ENG_CALL(mlp_fwd(stream, M, d->width, feat, d->dec, images, sdf_s, rgb_s, nullptr, masks));
    mark(e, st, PSVO_TIME_MLP_FWD, 1);
    o.images = images;
    o.sdf_s = sdf_s;
    o.s.rgb_s = rgb_s;
    o.s.masks = masks;
    const size_t RS = (size_t)r_hit * o.s_max;
    ENG_BUF(float, sdf, kSdf, RS * sizeof(float));
    ENG_BUF(float, weights, kWeights, RS * sizeof(float));
    ENG_BUF(float, color, kColor, (size_t)r_hit * 3 * sizeof(float));
    ENG_BUF(float, depth, kDepth, (size_t)r_hit * sizeof(float));
    ENG_BUF(float, z_min, kZmin, (size_t)r_hit * sizeof(float));
    ENG_CALL(psvo_composite_fwd(stream, r_hit, o.s_max, d->truncation, o.s.offsets, o.ray_ns, o.z_vals, sdf_s, rgb_s,
                                sdf, weights, color, depth, z_min));
    o.sdf = sdf;
    o.weights = weights;
    o.color = color;
    o.depth = depth;
    return PSVO_OK;
}

// ---- the mapping step's render: fused with the loss (compositing is part of
// psvo_composite_loss), activations kept for the weight gradients

// one render_map call's fixed inputs
struct MapRender {
    psvo_engine *e;
    hipStream_t st;
    const psvo_map_desc *d;
    QuerySet &qset;
    const float *rays_o, *rays_d;
    const char *who;
    // no padded [R_hit, S_max] copy — the loss kernels read z from the
    // sampler's depth rows (stride max_steps; the union S_max of a
    // data-parallel step is at most every rank's max_steps) and the samples
    // are compacted ray-major (by the look-back sampler in its own launch,
    // else k_compact_rays: a wave per hit ray over its ≈ 64 valid entries);
    // false (PSVO_PATH_PADDED): the padded copy, as in render_track
    bool rays_path;
    bool sparse;        // the sparse decoder: the sdf trunk only, the rest after the step's selection
    bool need_z_event;  // aux waits for z (e->z_ready) before the loss normalisers
};

// The decoder's operand images depend only on the weights (the previous
// step's Adam is ordered before them on st): kept from the previous
// look-ahead step, or built on aux while the host waits for the query's
// read-back, or (a timed step in mode 1) inline by the decoder forward.
struct Images {
    float *buf = nullptr;
    bool prebuilt = false;  // the previous step built them after its Adam step (e->images_next)
    bool on_aux = false;    // queued on aux now: their first reader on st waits for e->prep_done
    bool ready() const { return prebuilt || on_aux; }
};
int prepare_images(const MapRender &c, Images &im) {
    psvo_engine *e = c.e;
    hipStream_t st = c.st;
    int rc = PSVO_OK;
    ENG_BUF(float, images, kImages, psvo_mlp_image_floats_w(c.d->width) * sizeof(float));
    im.buf = images;
    im.prebuilt = e->images_next && e->images_w0 == c.d->dec[0];
    e->images_next = false;
    im.on_aux = engine_overlap(e) && !im.prebuilt;
    if (im.on_aux) {
        ENG_CALL(fork_join(st, e->aux, e->prep_fork));
        ENG_CALL(mlp_images(e->aux, c.d->width, c.d->dec, images));
        ENG_CALL(ev_record(e->prep_done, e->aux, c.who));
    }
    return PSVO_OK;
}

// The device-sized forward: the interpolation and the sdf trunk (width 128:
// one kernel, the trunk interpolating in its operand load) queued
// BEFORE the host waits for the query's statistics, sized on the device
// (the sampler's M, kMDev) within a capacity grown from earlier batches —
// the GPU runs them straight after the sampler instead of after the
// host's read-back and launch (≈ 19 µs of idle GPU per step at config B).
// A batch beyond the capacity makes them write nothing; the host then
// runs them sized by the read-back (host_forward), as without this path.
struct EarlyFwd {
    bool on = false;  // queued (it opened the PSVO_TIME_MLP_FWD region)
    int64_t cap = 0;  // samples it covers
    float *feat = nullptr, *sdf = nullptr, *h2 = nullptr;  // where it wrote: host_forward's buffers must be these
};
int device_forward(const MapRender &c, const Images &im, Render &o, EarlyFwd &ef) {
    psvo_engine *e = c.e;
    hipStream_t st = c.st;
    const psvo_map_desc *d = c.d;
    QuerySet &qset = c.qset;
    int rc = PSVO_OK;
    const int64_t m_early = std::min<int64_t>(e->m_early, (int64_t)qset.R * qset.max_steps);
    ef.on = c.rays_path && c.sparse && qset.compacted && qset.a.p[kMDev] && m_early > 0 && im.ready() &&
            !(e->paths & PSVO_PATH_QUERY_SPLIT);
    if (!ef.on) return PSVO_OK;
    ef.cap = m_early;
    const int *m_dev = static_cast<const int *>(qset.a.p[kMDev]);
    ENG_BUF(float, fe, kFeat, m_early * 16 * sizeof(float));
    ENG_BUF(float, se, kSdfS, m_early * sizeof(float));
    ef.feat = fe;
    ef.sdf = se;
    // the sparse decoder (width 128): the sdf trunk hands every sample's h2 to
    // the later layers (k_mlp_fwd2 / k_mlp_trunk_fb read it instead of
    // recomputing the W2 layer); width 256's trunk (k_dec256_trunk) is
    // device-sized too but keeps no h2
    if (d->width == 128) {
        ENG_BUF(float, he, kH2, m_early * kW128 * sizeof(float));
        ef.h2 = he;
    }
    ENG_CALL(join_adam(e, st, c.who, 2000.0));
    const int *leaf_q = static_cast<const int *>(qset.a.p[kLeafQ]);
    const float *t_q = static_cast<const float *>(qset.a.p[kTQ]);
    const int *ray_of_q = static_cast<const int *>(qset.a.p[kRayOfQ]);
    const int *rank_ray = static_cast<const int *>(qset.a.p[kRankRay]);
    // width 128: the trunk interpolates in its operand load and leaves the
    // feature rows itself (k_mlp_sdf2<true, true>: k_interp_fwd's bits) — no
    // separate pass over the samples between the sampler and the trunk, and no
    // PSVO_TIME_INTERP_FWD region.  PSVO_PATH_INTERP_PASS and width 256 keep
    // the pass.
    const bool fused = d->width == 128 && !(e->paths & PSVO_PATH_INTERP_PASS);
    if (!fused) {
        mark(e, st, PSVO_TIME_INTERP_FWD, 0);
        ENG_CALL(psvo::interp_fwd_dev(st, m_early, m_dev, d->voxel_size, leaf_q, t_q, ray_of_q, rank_ray, c.rays_o,
                                      c.rays_d, d->centres, d->vertex_idx, d->emb, ef.feat));
        mark(e, st, PSVO_TIME_INTERP_FWD, 1);
    }
    mark(e, st, PSVO_TIME_MLP_FWD, 0);  // stays open: host_forward or, sparse, step_select closes it
    if (im.on_aux) ENG_CALL(st_wait(st, e->prep_done, c.who));
    if (fused) {
        const psvo::InterpSrc ip{leaf_q, ray_of_q, rank_ray, d->vertex_idx, t_q, c.rays_o, c.rays_d, d->centres,
                                 reinterpret_cast<const float4 *>(d->emb), d->voxel_size};
        ENG_CALL(psvo::mlp_trunk_interp(st, m_early, m_dev, ip, im.buf, ef.sdf, ef.h2, ef.feat));
    } else {
        const psvo::H2Rows h2o{ef.h2, nullptr, nullptr};
        ENG_CALL(mlp_fwd_prepared(st, m_early, d->width, ef.feat, im.buf, ef.sdf, nullptr, nullptr, nullptr, m_dev,
                                  &h2o));
    }
    // the loss normalisers need only z (the sampler's rows): aux may start
    // them after these (a marker in front of them delays the interpolation)
    if (engine_overlap(e) && c.need_z_event) {
        ENG_CALL(ev_record(e->z_ready, st, c.who));
        o.z_recorded = true;
    }
    return PSVO_OK;
}

// the batch's samples where the forward reads them (o.s.leaf / tt / ray_of,
// preset to the step's own buffers) and z; e->z_ready once z is there
int place_samples(const MapRender &c, Render &o) {
    psvo_engine *e = c.e;
    hipStream_t st = c.st;
    QuerySet &qset = c.qset;
    if (!c.rays_path) {
        ENG_CALL(padded_samples(e, st, qset, o));
        // the loss normalisers can start now (step_normalisers, on aux)
        if (engine_overlap(e)) {
            ENG_CALL(ev_record(e->z_ready, st, c.who));
            o.z_recorded = true;
        }
        return PSVO_OK;
    }
    if (qset.compacted) {  // the sampler compacted in its launch (look-back offsets)
        o.s.leaf = static_cast<int *>(qset.a.p[kLeafQ]);
        o.s.tt = static_cast<float *>(qset.a.p[kTQ]);
        o.s.ray_of = static_cast<int *>(qset.a.p[kRayOfQ]);
    }
    // the loss normalisers need only z: aux may start them now (a
    // marker packet on st: none when aux has nothing to wait for)
    if (engine_overlap(e) && c.need_z_event && !o.z_recorded) {
        ENG_CALL(ev_record(e->z_ready, st, c.who));
        o.z_recorded = true;
    }
    if (!qset.compacted) {
        mark(e, st, PSVO_TIME_POINTS, 0);
        ENG_CALL(psvo::compact_rays(st, o.r_hit, qset.max_steps, static_cast<const int *>(qset.a.p[kSIdx]),
                                    static_cast<const float *>(qset.a.p[kSDepth]), o.s.offsets, o.s.leaf, o.s.tt,
                                    o.s.ray_of));
        mark(e, st, PSVO_TIME_POINTS, 1);
    }
    o.z_vals = static_cast<float *>(qset.a.p[kSDepth]);
    o.z_stride = qset.max_steps;
    return PSVO_OK;
}

// The forward sized by the read-back (o.m): sample placement, then whatever
// the device-sized forward did not cover — the interpolation and the decoder
// (sparse: its sdf trunk).  The device-sized forward wrote into the buffers
// allocated here; an allocation that moved one of them is an error.
int host_forward(const MapRender &c, const Images &im, const EarlyFwd &ef, Render &o) {
    psvo_engine *e = c.e;
    hipStream_t st = c.st;
    const psvo_map_desc *d = c.d;
    const char *who = c.who;
    int rc = PSVO_OK;
    const int64_t M = o.m;
    // the device-sized forward covered this batch (else: it wrote nothing, run it host-sized below)
    const bool early_done = ef.on && M <= ef.cap;
    if (c.rays_path && c.sparse) e->m_early = std::max<int64_t>(e->m_early, M + M / 4);
    ENG_BUF(int, leaf, kLeaf, M * sizeof(int));
    ENG_BUF(float, tt, kT, M * sizeof(float));
    ENG_BUF(int, ray_of, kRayOf, M * sizeof(int));
    ENG_BUF(float, feat, kFeat, M * 16 * sizeof(float));
    if (early_done && feat != ef.feat) return set_error(PSVO_E_LAUNCH, "%s: feature buffer moved", who);
    o.s.leaf = leaf;
    o.s.tt = tt;
    o.s.ray_of = ray_of;
    o.s.feat = feat;
    ENG_CALL(place_samples(c, o));
    // ---- forward: interpolation, decoder (after the previous step's
    // optimiser step when its tail ran on aux)
    ENG_CALL(join_adam(e, st, who));
    if (!early_done) {  // (a batch beyond the device-sized forward's capacity: no region of its own — the
                        // device-sized forward marked it, or interpolated inside the trunk's region)
        if (!ef.on) mark(e, st, PSVO_TIME_INTERP_FWD, 0);
        ENG_CALL(psvo_interp_fwd(st, M, 16, d->voxel_size, o.s.leaf, o.s.tt, o.s.ray_of, o.rank_ray, c.rays_o, c.rays_d,
                                 d->centres, d->vertex_idx, d->emb, feat));
        if (!ef.on) mark(e, st, PSVO_TIME_INTERP_FWD, 1);
    }
    ENG_BUF(float, sdf_s, kSdfS, M * sizeof(float));
    if (early_done && sdf_s != ef.sdf) return set_error(PSVO_E_LAUNCH, "%s: sdf buffer moved", who);
    float *h2_s = nullptr;
    if (c.sparse && d->width == 128) {
        ENG_BUF(float, hb, kH2, M * kW128 * sizeof(float));
        if (early_done && hb != ef.h2) return set_error(PSVO_E_LAUNCH, "%s: h2 buffer moved", who);
        h2_s = hb;
    }
    // sparse: the sdf trunk (h1, h2, the sdf row: 18.6 of 53.8 k MACs per
    // sample) on every sample — the compositing weights need every sdf — and
    // the full decoder later, on the samples select_samples keeps
    o.sparse = c.sparse;
    if (!c.sparse) {
        ENG_BUF(float, rgb_b, kRgbS, M * 3 * sizeof(float));
        ENG_BUF(float, abuf, kAct, (size_t)psvo_mlp_act_floats(M, d->width) * sizeof(float));
        ENG_BUF(uint64_t, mbuf, kMasks, (size_t)psvo_mlp_mask_words(M, d->width) * sizeof(uint64_t));
        o.s.rgb_s = rgb_b;
        o.s.act = abuf;
        o.s.masks = mbuf;
    }
    if (!ef.on) mark(e, st, PSVO_TIME_MLP_FWD, 0);  // (else the device-sized forward opened it)
    if (early_done) {
        o.h2 = h2_s;
    } else if (im.ready()) {
        if (im.on_aux) ENG_CALL(st_wait(st, e->prep_done, who));
        const psvo::H2Rows h2o{h2_s, nullptr, nullptr};
        ENG_CALL(mlp_fwd_prepared(st, M, d->width, feat, im.buf, sdf_s, o.s.rgb_s, o.s.act, o.s.masks, nullptr, &h2o));
        o.h2 = h2_s;
    } else {
        ENG_CALL(mlp_fwd(st, M, d->width, feat, d->dec, im.buf, sdf_s, o.s.rgb_s, o.s.act, o.s.masks));
    }
    // sparse: the region stays open over the selection (its own, nested
    // region) and the compact forward: step_select closes it
    if (!c.sparse) mark(e, st, PSVO_TIME_MLP_FWD, 1);
    o.images = im.buf;
    o.sdf_s = sdf_s;
    return PSVO_OK;
}

// render_rays on the device for the mapping step: decoder images, the
// device-sized forward, the host's wait for the query, the host-sized forward
// and (data parallel, with samples) the query's late second half
int render_map(const MapRender &c, int *stats_out, Render &o) {
    Images im;
    ENG_CALL(prepare_images(c, im));
    EarlyFwd ef;
    ENG_CALL(device_forward(c, im, o, ef));
    Readback rb;
    ENG_CALL(query_readback(c.e, c.qset, c.rays_path, stats_out, c.who, rb));
    render_begin(c.qset, rb, o);
    if (rb.empty) return PSVO_OK;  // an empty shard still joins the collectives (it just did)
    ENG_CALL(host_forward(c, im, ef, o));
    ENG_CALL(query_readback_late(c.e, c.qset, stats_out, c.who, rb));
    o.s_max = rb.s_max;
    return PSVO_OK;
}

// Criterion forward + backward to the per-sample decoder gradients (d loss =
// 1); dtmp/dthr: tracking's median depth filter or NULL.
int loss_backward(psvo_engine *e, hipStream_t st, const psvo_map_desc *d, const Render &q, const float *gt_rgb,
                  const float *gt_depth, const float *dtmp, const float *dthr, float *loss_out, float **g_sdf_s_out,
                  float **g_rgb_s_out) {
    int rc = PSVO_OK;
    void *stream = st;
    const int64_t r_hit = q.r_hit, M = q.m;
    const int s_max = q.s_max;
    const size_t RS = (size_t)r_hit * s_max;
    ENG_BUF(float, crit_ws, kCritWs, psvo_criterion_workspace_floats(r_hit) * sizeof(float));
    ENG_BUF(double, sums, kSums, 8 * sizeof(double));
    ENG_CALL(psvo_criterion_sums_ex(stream, r_hit, s_max, 0, d->truncation, d->max_depth, q.rank_ray, gt_rgb,
                                    gt_depth, q.color, q.depth, q.sdf, q.z_vals, dtmp, dthr, crit_ws, sums));
    ENG_CALL(psvo_criterion_finalize(stream, sums, r_hit, s_max, d->w_rgb, d->w_depth, d->w_fs, d->w_sdf,
                                     d->truncation, kCritFlags, loss_out));
    ENG_BUF(float, g_loss, kGLoss, sizeof(float));
    if (hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(g_loss), 0x3F800000 /* 1.0f */, 1, st) != hipSuccess)
        return set_error(PSVO_E_LAUNCH, "engine: g_loss fill failed");
    ENG_BUF(float, g_color, kGColor, (size_t)r_hit * 3 * sizeof(float));
    ENG_BUF(float, g_depth, kGDepth, (size_t)r_hit * sizeof(float));
    ENG_BUF(float, g_sdf, kGSdf, RS * sizeof(float));
    ENG_CALL(psvo_criterion_bwd_ex(stream, r_hit, s_max, d->truncation, d->max_depth, q.rank_ray, gt_rgb, gt_depth,
                                   q.color, q.depth, q.sdf, q.z_vals, loss_out, g_loss, dtmp, dthr, g_color, g_depth,
                                   g_sdf));
    ENG_BUF(float, g_sdf_s, kGSdfS, M * sizeof(float));
    ENG_BUF(float, g_rgb_s, kGRgbS, M * 3 * sizeof(float));
    ENG_CALL(psvo_composite_bwd(stream, r_hit, s_max, d->truncation, q.s.offsets, q.ray_ns, q.z_vals, q.sdf, q.weights,
                                q.s.rgb_s, g_color, g_depth, nullptr, g_sdf, g_sdf_s, g_rgb_s));
    *g_sdf_s_out = g_sdf_s;
    *g_rgb_s_out = g_rgb_s;
    return PSVO_OK;
}

// the keyframe poses' part of an iteration (psvo_map_step_frames): per-frame
// gradient from the rays' grad_o / grad_d, then each optimised pose's Adam
int frames_update(psvo_engine *e, hipStream_t st, const psvo_map_desc *d, const psvo_map_frames *fr,
                  const Render &q, const float *grad_od, int64_t R, PoseAdam *pa) {
    int rc = PSVO_OK;
    float *pg = fr->pose_grad;
    if (!pg) {
        ENG_BUF(float, gbuf, kPoseGrad, (size_t)fr->n_frames * 8 * sizeof(float));
        pg = gbuf;
    }
    // data parallel: a keyframe belongs to one rank (each rank passes its own
    // keyframes), so its rays — and its whole pose gradient of the union-batch
    // loss — are local: no exchange
    ENG_CALL(psvo::pose_grad_frames_rays(st, fr->n_frames, fr->rays_per_frame, q.ray_rank, fr->dirs_cam, grad_od,
                                         grad_od + R * 3, fr->poses, pg));
    pa->n = 0;
    pa->lr = fr->lr_pose;
    for (int f = 0; f < fr->n_frames; ++f) {
        if (fr->pose_step[f] < 1) continue;  // stamp 0 / update_pose False: no optimiser (render_helpers.py:594-596)
        const int k = pa->n++;
        pa->p[k] = fr->poses + f * 6;
        pa->m[k] = fr->pose_m + f * 6;
        pa->v[k] = fr->pose_v + f * 6;
        pa->g[k] = pg + f * 8;
        pa->step[k] = fr->pose_step[f];
    }
    return PSVO_OK;
}

// The next iteration's query, queued on `ps` after this step's pose update:
// its rays (the updated poses applied to next_dirs_cam) into the engine's ray
// buffers — this step's last reader of them, the embedding backward, ran
// earlier on `ps` — then intersection + sampling into the free query set.
int frames_lookahead(psvo_engine *e, hipStream_t st, const psvo_map_desc *d, const psvo_map_frames *fr,
                     int64_t R, const Render &cur, const float *grad_od, bool record_done) {
    int rc = PSVO_OK;
    PSVO_REQUIRE(e->q_count == 0, "map_step_frames: a query is already queued");
    QuerySet &q = e->qs[e->q_head];
    // the set's last consumer ran on st itself: stream order suffices (no wait
    // packet between the backward and the pose step)
    ENG_CALL(freed_wait(q, st));
    ENG_BUF(float, rays_o, kRaysO, (size_t)R * 3 * sizeof(float));
    ENG_BUF(float, rays_d, kRaysD, (size_t)R * 3 * sizeof(float));
    float *pg = fr->pose_grad;
    if (!pg) {
        ENG_BUF(float, gbuf, kPoseGrad, (size_t)fr->n_frames * 8 * sizeof(float));
        pg = gbuf;
    }
    // this step's pose gradient, each optimised pose's Adam step and the next
    // rays from the updated poses: one launch (frames_update + pose_adam +
    // psvo_pose_rays_frames, the same arithmetic)
    ENG_CALL(psvo::pose_step_frames(st, fr->n_frames, fr->rays_per_frame, cur.ray_rank, fr->dirs_cam,
                                    grad_od, grad_od + R * 3, fr->poses, fr->pose_m, fr->pose_v, fr->pose_step,
                                    fr->lr_pose, d->beta1, d->beta2, d->eps, pg, fr->next_dirs_cam, rays_o, rays_d));
    ENG_CALL(query_enqueue(e, st, q, d, R, rays_o, rays_d, fr->next_seed, "map_step_frames (look-ahead)", nullptr,
                           record_done, fr->next_gt_depth));
    q.dirs = fr->next_dirs_cam;
    q.pending = true;
    e->q_count++;
    return PSVO_OK;
}

// ---- the mapping step: map_step_impl is its schedule, the stages below its
// bodies, MapStep what they share.  Streams: `st` the caller's; `ax` the side
// work (loss normalisers, embedding backward; data parallel also the loss
// value); `lq` the loss value; `eb` the embedding backward and the
// look-ahead.  Timed in mode 1 they are all st.
struct MapStep {
    psvo_engine *e;
    hipStream_t st;
    const psvo_map_desc *d;
    const psvo_map_frames *fr;
    int flags;
    int64_t R, adam_step;
    const float *rays_o, *rays_d, *gt_rgb, *gt_depth;
    float *loss_out;
    // fixed at the step's entry
    bool overlap = false, dist = false, want_loss = false, wait_next = false, ahead = false, split = false;
    hipStream_t ax = nullptr, lq = nullptr, eb = nullptr;
    const float *counts_gt = nullptr;  // the GT depths the query may have counted the normalisers with
    uint8_t *mark_into = nullptr;      // the embedding rows this step touches are flagged here (or null)
    bool sparse_rows = false;          // ... and its Adam step reads the flags (sparse-exact)
    // the render's result
    QuerySet *qset = nullptr;
    Render q;
    bool empty = false;  // data parallel: no samples on this rank
    int64_t n_hit = 0;   // the (union) batch's hit rays
    // step_select: what the loss pass and the backward read per sample — the
    // kept samples when sparse (class A at [0, M), class B at [M, 2 M)), else q.s
    Samples k;
    int *cidx = nullptr, *sel_cnt = nullptr, *offb = nullptr;
    const int *h2_src = nullptr;  // the kept samples' rows of q.h2
    // step_normalisers / step_loss
    float *crit_ws = nullptr, *coef = nullptr, *g_sdf_s = nullptr, *g_rgb_s = nullptr;
    double *sums = nullptr;
    // step_grad_buffers
    float *grads = nullptr, *grad_od = nullptr;
    float *G[10] = {};

    bool two_class() const { return q.sparse && d->width == 128; }
    int64_t m_rows() const { return q.sparse ? 2 * q.m : q.m; }  // per-sample gradient rows (sparse: at cidx)
    bool join_loss() const { return want_loss && lq != ax; }
    bool no_adam() const { return (flags & PSVO_STEP_NO_ADAM) != 0; }
};

// The sparse decoder: the samples whose gradients can be non-zero get compact
// indices (composite.hip k_select_samples) — class A (composited) at
// [0, M_A): the whole decoder forward; width 128, class B (only the direct
// sdf loss term) at [M, M + M_B): the trunk's forward + backward in one
// kernel (k_mlp_trunk_fb) — sized on the device (the counts never reach the
// host).  Closes the PSVO_TIME_MLP_FWD region the render left open.
int step_select(MapStep &s) {
    psvo_engine *e = s.e;
    hipStream_t st = s.st;
    const psvo_map_desc *d = s.d;
    const Render &q = s.q;
    s.k = q.s;
    if (!q.sparse || s.empty) return PSVO_OK;
    int rc = PSVO_OK;
    const int64_t M = q.m, r_hit = q.r_hit;
    const int64_t M2 = 2 * M;  // the compact rows: class A at [0, M), class B at [M, 2 M)
    ENG_BUF(int, cx, kCidx, M * sizeof(int));
    ENG_BUF(int, offa, kOffB, (size_t)(r_hit + 1) * sizeof(int));
    // the compact feature copy: width 256 only (width 128 reads the step's rows by src_c)
    float *feat_c = nullptr;
    if (!q.h2) {
        ENG_BUF(float, fc, kFeatB, M2 * 16 * sizeof(float));
        feat_c = fc;
    }
    ENG_BUF(int, leaf_c, kLeafB, M2 * sizeof(int));
    ENG_BUF(float, t_c, kTB, M2 * sizeof(float));
    ENG_BUF(int, ray_of_c, kRayOfB, M2 * sizeof(int));
    ENG_BUF(int, cnt, kSelCnt, psvo::kSelCountInts * sizeof(int));
    ENG_BUF(unsigned long long, desc, kSelDesc, (size_t)psvo::select_granules(r_hit) * sizeof(unsigned long long));
    if (e->sel_zero_gen != e->a.gen[kSelDesc]) {  // fresh memory: no stale granule may carry a future tag
        ENG_CALL(zero_async(desc, e->a.cap[kSelDesc], st, "map_step"));
        ENG_CALL(zero_async(cnt, psvo::kSelCountInts * sizeof(int), st, "map_step"));
        e->sel_zero_gen = e->a.gen[kSelDesc];
    }
    if (!e->host_flags) {
        if (hipHostMalloc(reinterpret_cast<void **>(&e->host_flags), sizeof(int),
                          hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess)
            return set_error(PSVO_E_LAUNCH, "map_step: pinned allocation failed");
        *e->host_flags = 0;
    }
    if (s.two_class()) {
        ENG_BUF(int, ob, kOffB2, (size_t)(r_hit + 1) * sizeof(int));
        s.offb = ob;
    }
    ENG_BUF(float, rgb_c, kRgbS, M2 * 3 * sizeof(float));
    int *src_c = nullptr;
    if (q.h2) {
        ENG_BUF(int, sc, kSrcC, M2 * sizeof(int));
        src_c = sc;
    }
    e->sel_tag = e->sel_tag == 0xffffffffu ? 1u : e->sel_tag + 1u;
    mark(e, st, PSVO_TIME_SELECT, 0);
    if (e->draw_gate_used && !e->draw_gate &&
        hipEventCreateWithFlags(&e->draw_gate, hipEventDisableSystemFence) != hipSuccess)
        return set_error(PSVO_E_LAUNCH, "map_step: event creation failed");
    {
        // the draw gate: bound to the selection's dispatch (a timed step: the
        // clock's stop event of the selection stands in for it, no marker)
        psvo::StopBind gate(e->draw_gate_used ? e->draw_gate : nullptr, true);
        const int sel_rc = psvo::select_samples(st, r_hit, q.s_max, d->truncation, d->max_depth, q.s.offsets, q.ray_ns,
                                                q.z_vals, q.z_stride, q.rank_ray, s.gt_depth, q.sdf_s, q.s.feat,
                                                q.s.leaf, q.s.tt, q.s.ray_of, M, s.two_class(), cx, offa, s.offb,
                                                feat_c, leaf_c, t_c, ray_of_c, rgb_c, src_c, cnt, desc, e->sel_tag,
                                                e->host_flags);
        if (gate.consumed() && gate.bound()) {  // (consumed: launched)
            e->draw_gate_ev = gate.bound();
            e->draw_gate_recorded = true;
        }
        ENG_CALL(sel_rc);
    }
    mark(e, st, PSVO_TIME_SELECT, 1);
    ENG_BUF(float, sdf_b, kSdfB, M * sizeof(float));
    ENG_BUF(float, act, kAct, (size_t)psvo_mlp_act_floats(M, d->width) * sizeof(float));
    ENG_BUF(uint64_t, masks, kMasks, (size_t)psvo_mlp_mask_words(M, d->width) * sizeof(uint64_t));
    const psvo::H2Rows h2r{nullptr, q.h2, src_c};
    // (src_c: x of kept sample j is row src_c[j] of the step's features)
    float *feat_k = src_c ? q.s.feat : feat_c;
    ENG_CALL(mlp_fwd_prepared(st, M, d->width, feat_k, q.images, sdf_b, rgb_c, act, masks, cnt,
                              src_c ? &h2r : nullptr));
    mark(e, st, PSVO_TIME_MLP_FWD, 1);  // opened by the render (device_forward / host_forward)
    s.k = Samples{offa, leaf_c, ray_of_c, t_c, feat_k, rgb_c, act, masks};
    s.h2_src = src_c;
    s.cidx = cx;
    s.sel_cnt = cnt;
    return PSVO_OK;
}

// The loss normalisers on `ax` (after the sampler, beside the decoder
// forward) unless the query counted them; st then waits for the
// coefficients.  Data parallel: the loss of the union batch (criterion.py:
// 70-101 normalise by batch-global counts and the padded [R_hit, S_max]
// size) — count sums and loss sums are all-reduced, the rank's gradients are
// its part of the union-batch gradient (the caller sums them over ranks).
int step_normalisers(MapStep &s) {
    psvo_engine *e = s.e;
    hipStream_t st = s.st, ax = s.ax;
    const psvo_map_desc *d = s.d;
    const Render &q = s.q;
    QuerySet *qset = s.qset;
    const EngineExchange &x = e->x;
    int rc = PSVO_OK;
    ENG_BUF(float, crit_ws, kCritWs, psvo_criterion_workspace_floats(q.r_hit) * sizeof(float));
    s.crit_ws = crit_ws;
    double *sums_c = x.xf64;
    s.sums = x.xf64 ? x.xf64 + 8 : nullptr;
    if (!s.dist) {
        ENG_BUF(double, sc, kSumsC, 8 * sizeof(double));
        ENG_BUF(double, sl, kSums, 8 * sizeof(double));
        sums_c = sc;
        s.sums = sl;
    }
    // the sampler counted the normalisers for exactly this GT (its tail wrote the coefficients)
    const bool coef_q = !s.dist && s.counts_gt && qset->counts_gt == s.counts_gt;
    // data parallel: the query gathered the union's counts — decided from the
    // gathered words (PSVO_FLAG_UNION_UNCOUNTED), the same on every rank, so
    // that all ranks issue the same collectives (psvo_map_query's counts_gt
    // must hold the step's GT depths: psvo.h)
    const bool sums_q = s.dist && s.counts_gt && qset->counts_gt != nullptr &&
                        !(qset->host_stats[PSVO_STAT_FLAGS] & psvo::PSVO_FLAG_UNION_UNCOUNTED);
    s.coef = coef_q ? static_cast<float *>(qset->a.p[kCoefQ]) : nullptr;
    if (!coef_q) {
        ENG_BUF(float, cbuf, kCoef, 4 * sizeof(float));
        s.coef = cbuf;
    }
    if (s.dist) {
        if (sums_q) {
            sums_c = static_cast<double *>(qset->a.p[kDistSums]);
            // (landed on the host before this launch; the wait orders it formally)
            ENG_CALL(st_wait(ax, qset->done2, "map_step"));
        } else {
            ENG_CALL(criterion_counts(ax, s.empty ? 0 : q.r_hit, q.s_max, d->truncation, d->max_depth, q.rank_ray,
                                      s.gt_depth, q.z_vals, q.z_stride, q.z_stride == q.s_max ? nullptr : q.ray_ns,
                                      crit_ws, sums_c));
            ENG_CALL(x.call(PSVO_XCH_SUM_F64, 0, 0, 8, ax, "loss normalisers"));
        }
        ENG_CALL(criterion_coef_from_sums(ax, sums_c, s.n_hit, q.s_max, d->truncation, d->w_rgb, d->w_depth, d->w_fs,
                                          d->w_sdf, kCritFlags, s.coef));
    } else if (!coef_q) {
        ENG_CALL(psvo::criterion_coef_z(ax, q.r_hit, q.s_max, d->truncation, d->max_depth, q.rank_ray, s.gt_depth,
                                        q.z_vals, q.z_stride, q.ray_ns, d->w_rgb, d->w_depth, d->w_fs, d->w_sdf,
                                        kCritFlags, crit_ws, sums_c, s.coef));
    }
    if (!coef_q) ENG_CALL(fork_join(ax, st, e->coef_ready));
    // after the normalisers: the fused loss pass waits for them, Adam for the marks
    // (width 128: the fused backward's embedding scatter flags the rows it touches instead — the mark
    // kernel beside the decoder forward slowed it by ≈ 17 µs)
    if (s.mark_into && !s.empty && !psvo::mlp_bwd_fuses_interp(d->width))
        ENG_CALL(psvo_adam_mark_rows(ax, q.m, q.s.leaf, d->vertex_idx, s.mark_into));
    return PSVO_OK;
}

// One fused per-ray pass on st: compositing, loss terms and the per-sample
// decoder gradients (d loss = 1).  Then the loss value (not on the gradient
// path), beside the decoder backward: data parallel on aux (its collective),
// single GPU on its own stream; e->loss_done marks it (step_backward /
// step_tail join it).  PSVO_STEP_NO_LOSS: the caller does not read the value
// (bundle_adjust_frames discards it, render_helpers.py:662-676): no
// reduction, no collective (every rank passes the same flags).
int step_loss(MapStep &s) {
    psvo_engine *e = s.e;
    hipStream_t st = s.st, lq = s.lq;
    const psvo_map_desc *d = s.d;
    const Render &q = s.q;
    int rc = PSVO_OK;
    ENG_BUF(float, color, kColor, (size_t)q.r_hit * 3 * sizeof(float));
    ENG_BUF(float, depth, kDepth, (size_t)q.r_hit * sizeof(float));
    ENG_BUF(float, g_sdf_s, kGSdfS, s.m_rows() * sizeof(float));
    ENG_BUF(float, g_rgb_s, kGRgbS, s.m_rows() * 3 * sizeof(float));
    s.g_sdf_s = g_sdf_s;
    s.g_rgb_s = g_rgb_s;
    if (!s.empty)
        ENG_CALL(psvo::composite_loss_z(st, q.r_hit, q.s_max, d->truncation, d->max_depth, q.s.offsets, q.ray_ns,
                                        q.z_vals, q.z_stride, q.rank_ray, s.gt_rgb, s.gt_depth, q.sdf_s, s.k.rgb_s,
                                        s.coef, s.crit_ws, color, depth, g_sdf_s, g_rgb_s, s.want_loss || s.dist,
                                        s.cidx));
    if (!s.want_loss) return PSVO_OK;
    ENG_CALL(fork_join(st, lq, e->grads_ready));
    if (!s.empty)
        ENG_CALL(psvo_criterion_reduce(lq, q.r_hit, s.crit_ws, s.sums));
    else
        ENG_CALL(zero_async(s.sums, 8 * sizeof(double), lq, "map_step"));
    if (s.dist) ENG_CALL(e->x.call(PSVO_XCH_SUM_F64, 8, 8, 8, lq, "loss sums"));
    ENG_CALL(psvo_criterion_finalize(lq, s.sums, s.n_hit, q.s_max, d->w_rgb, d->w_depth, d->w_fs, d->w_sdf,
                                     d->truncation, kCritFlags, s.loss_out));
    if (lq != s.ax) ENG_CALL(ev_record(e->loss_done, lq, "map_step"));
    return PSVO_OK;
}

// gradients: the caller's flat buffer (data-parallel all-reduce) or the
// arena, [embeddings | W1, b1, ..., W5, b5]; the rays' d_o / d_d
int step_grad_buffers(MapStep &s) {
    psvo_engine *e = s.e;
    hipStream_t st = s.st;
    int rc = PSVO_OK;
    s.grads = s.d->grad_flat;
    if (!s.grads) {
        ENG_BUF(float, gbuf, kDecGrad, psvo_map_grad_floats_w(s.d->n_emb, s.d->width) * sizeof(float));
        s.grads = gbuf;
    }
    int64_t sizes[10];
    dec_sizes(s.d->width, sizes);
    int64_t off = s.d->n_emb * 16;
    for (int i = 0; i < 10; ++i) {
        s.G[i] = s.grads + off;
        off += sizes[i];
    }
    ENG_BUF(float, grad_od, kGradOD, (size_t)s.R * 6 * sizeof(float));
    s.grad_od = grad_od;
    return PSVO_OK;
}

// the step clock: one marker per step, on `on`
int step_clock(psvo_engine *e, hipStream_t on) {
    if (e->clk.on && e->clk.n < (int)e->clk.ev.size()) ENG_CALL(ev_record(e->clk.ev[e->clk.n++], on, "map_step"));
    return PSVO_OK;
}

// data parallel, no samples on this rank: its part of the gradient is zero —
// it has joined the step's collectives; what remains is the optimiser step
int step_empty(MapStep &s, QueryGuard &guard) {
    psvo_engine *e = s.e;
    ENG_CALL(fork_join(s.ax, s.st, e->emb_done));
    ENG_CALL(zero_async(s.grads, (size_t)psvo_map_grad_floats_w(s.d->n_emb, s.d->width) * sizeof(float), s.st,
                        "map_step"));
    e->grads_clean = false;
    ENG_CALL(guard.release());
    if (!s.no_adam()) ENG_CALL(map_adam(s.st, s.d, s.grads, s.adam_step));
    return step_clock(e, s.st);
}

// Decoder backward on st, then the embedding backward on `eb` (after dfeat,
// beside the weight-gradient reduce) and the joins back into st.
// width 128: the interpolation backward runs inside the fused decoder
// backward (embedding scatter into grad_emb, dL/dx per sample), then only
// the per-ray d_o / d_d sums remain; otherwise k_interp_bwd after dfeat.
int step_backward(MapStep &s) {
    psvo_engine *e = s.e;
    hipStream_t st = s.st, ax = s.ax, eb = s.eb;
    const psvo_map_desc *d = s.d;
    const Render &q = s.q;
    const Samples &k = s.k;
    int rc = PSVO_OK;
    const int64_t M = q.m, R = s.R;
    const int n_split = 256;
    ENG_BUF(float, mlp_ws, kMlpWs, psvo_mlp_workspace_floats_w(M, d->width, n_split) * sizeof(float));
    ENG_BUF(float, dfeat, kDfeat, M * 16 * sizeof(float));
    const bool fuse_ib = psvo::mlp_bwd_fuses_interp(d->width);
    float *grad_emb = s.grads;
    const size_t emb_bytes = (size_t)d->n_emb * 16 * sizeof(float);
    const bool emb_dirty = !(e->grads_clean && e->clean_buf == grad_emb);
    if (fuse_ib && emb_dirty) ENG_CALL(zero_async(grad_emb, emb_bytes, st, "map_step"));
    float *gx = nullptr;
    if (fuse_ib) {
        ENG_BUF(float, gxb, kIbWs, (size_t)s.m_rows() * 3 * sizeof(float));
        gx = gxb;
    }
    const psvo::InterpFuse ipf{k.leaf,  k.ray_of,      q.rank_ray, d->vertex_idx, k.tt, s.rays_o, s.rays_d, d->centres,
                               d->emb,  d->voxel_size, grad_emb,   gx,            s.mark_into};
    mark(e, st, PSVO_TIME_MLP_BWD, 0);
    // the sparse decoder's class B: its rows at [M, 2 M) of the compact arrays
    const psvo::InterpFuse ipf_b{k.leaf + M, k.ray_of + M, q.rank_ray, d->vertex_idx, k.tt + M, s.rays_o, s.rays_d,
                                 d->centres, d->emb, d->voxel_size, grad_emb, gx ? gx + 3 * M : nullptr, s.mark_into};
    const psvo::TrunkBwd tbw{s.sel_cnt ? s.sel_cnt + 1 : nullptr, s.g_sdf_s + M, s.h2_src ? k.feat : k.feat + M * 16,
                             fuse_ib ? &ipf_b : nullptr, s.h2_src ? q.h2 : nullptr, s.h2_src ? s.h2_src + M : nullptr,
                             (e->paths & PSVO_PATH_BWD_TWO_LAUNCH) != 0};
    // (split: the weight-gradient slab sum on aux, step_tail)
    ENG_CALL(mlp_bwd(st, M, d->width, k.feat, q.images, k.rgb_s, k.act, k.masks, s.g_sdf_s, s.g_rgb_s, dfeat, s.G, 0,
                     n_split, mlp_ws, s.overlap ? e->dfeat_ready : nullptr, fuse_ib ? &ipf : nullptr,
                     s.split ? ax : nullptr, s.sel_cnt, s.two_class() ? &tbw : nullptr, s.h2_src));
    mark(e, st, PSVO_TIME_MLP_BWD, 1);
    if (s.overlap) e->bwd_recorded = true;  // mlp_bwd recorded dfeat_ready on st
    if (s.overlap && eb != st) ENG_CALL(st_wait(eb, e->dfeat_ready, "map_step"));
    if (!fuse_ib && emb_dirty) ENG_CALL(zero_async(grad_emb, emb_bytes, eb, "map_step"));
    e->grads_clean = false;
    e->clean_buf = grad_emb;
    mark(e, eb, PSVO_TIME_INTERP_BWD, 0);
    if (fuse_ib) {
        ENG_CALL(psvo::interp_rays_gx(eb, q.r_hit, k.offsets, q.rank_ray, k.tt, gx, s.grad_od, s.grad_od + R * 3,
                                      s.two_class() ? s.offb : nullptr, s.two_class() ? k.tt + M : nullptr,
                                      s.two_class() ? gx + 3 * M : nullptr));
    } else {
        ENG_BUF(float, ib_ws2, kIbWs, psvo_interp_bwd_workspace_floats(q.r_hit, q.s_max) * sizeof(float));
        ENG_CALL(psvo_interp_bwd_chunked(eb, q.r_hit, q.s_max, 16, d->voxel_size, k.offsets, q.rank_ray, k.leaf, k.tt,
                                         s.rays_o, s.rays_d, d->centres, d->vertex_idx, d->emb, dfeat, grad_emb,
                                         s.grad_od, s.grad_od + R * 3, ib_ws2));
    }
    mark(e, eb, PSVO_TIME_INTERP_BWD, 1);
    if (s.overlap && eb != st) {
        ENG_CALL(ev_record(e->emb_done, eb, "map_step"));
        ENG_CALL(st_wait(st, e->emb_done, "map_step"));
    }
    // the loss value's reads of crit_ws before the next step's writes: through
    // st, or (split) through aux's optimiser step, which the next render waits
    // for; split, st joins it too once the look-ahead is queued (step_tail)
    if (s.join_loss()) ENG_CALL(st_wait(s.split ? ax : st, e->loss_done, "map_step"));
    return PSVO_OK;
}

// The step's tail: the poses (with a look-ahead, also the next iteration's
// rays and query), the optimiser steps, the next decoder images, the step
// clock.  Look-ahead with the fused backward (s.split): st runs the per-ray
// sums, the pose step and the next query right after the decoder backward;
// aux sums the weight-gradient slabs, steps the optimiser and builds the next
// decoder images beside them (the next step's render waits for adam_done).
int step_tail(MapStep &s) {
    psvo_engine *e = s.e;
    hipStream_t st = s.st, ax = s.ax, eb = s.eb;
    const psvo_map_desc *d = s.d;
    int rc = PSVO_OK;
    PoseAdam pa;
    // look-ahead (psvo_map_frames.next_dirs_cam): the poses' gradient and
    // Adam step right after the embedding backward on its stream, then the
    // next iteration's rays + query there too — beside this step's weight
    // gradients and the map's Adam
    if (s.ahead) {
        if (s.wait_next) ENG_CALL(st_wait(eb, e->next_ready, "map_step"));
        // queued on the step's own stream (split tail): consumed there, no event
        ENG_CALL(frames_lookahead(e, eb, d, s.fr, s.R, s.q, s.grad_od, eb != st));
    } else if (s.fr) {
        ENG_CALL(frames_update(e, st, d, s.fr, s.q, s.grad_od, s.R, &pa));
    }
    // ---- optimiser steps, the poses' with the map's (the map's are skipped
    // when the caller all-reduces the gradients first)
    hipStream_t os = st;  // the stream of the optimiser step
    if (!s.no_adam()) {
        if (s.split) os = ax;
        ENG_CALL(map_adam(os, d, s.grads, s.adam_step, &pa, s.sparse_rows));
        e->grads_clean = true;
        if (s.ahead) {  // the next iteration's decoder images, while the look-ahead query runs
            ENG_BUF(float, images, kImages, psvo_mlp_image_floats_w(d->width) * sizeof(float));
            ENG_CALL(mlp_images(os, d->width, d->dec, images));
            e->images_next = true;
            e->images_w0 = d->dec[0];
        }
        if (s.split) {
            ENG_CALL(ev_record(e->adam_done, ax, "map_step"));
            e->adam_pending = true;
        }
    } else {
        ENG_CALL(pose_adam(st, d, pa));
    }
    // the step clock: after the optimiser step, on the stream that ran it (a
    // look-ahead step's: aux, where nothing waits behind the marker) — the
    // same point of every step (on st between two dependent kernels a marker
    // costs ≈ 5 µs, measured: not earlier)
    ENG_CALL(step_clock(e, os));
    // split tail: loss_out is written on the loss stream; the caller reads it
    // on st (the loss pass ends long before the look-ahead's pose step, so
    // this wait, queued behind the look-ahead, costs nothing).  The weights
    // stay pending on aux until the next engine call or psvo_map_join.
    if (s.split && s.join_loss()) ENG_CALL(st_wait(st, e->loss_done, "map_step"));
    return PSVO_OK;
}

// One mapping iteration: the schedule.  The two cross-stream waits it needs
// on st — the previous step's optimiser (before the interpolation reads the
// embeddings: the render) and the draw of the next pixels (before the
// look-ahead's pose step) — sit where their consumers are.  Queued in front
// of the render, both measured slower (round 4, config B: 0.941 vs
// 0.928-0.932 ms per iteration): the next draw co-runs with the persistent
// decoder kernels and ends late, so the render then waits for it.
int map_step_impl(psvo_engine *e, hipStream_t st, const psvo_map_desc *d, int64_t n_rays, const float *rays_o,
                  const float *rays_d, const float *gt_rgb, const float *gt_depth, const float *noise, uint64_t seed,
                  int64_t adam_step, int flags, float *loss_out, int *stats_out, const psvo_map_frames *fr) {
    PSVO_REQUIRE(e && d && rays_o && rays_d && gt_rgb && gt_depth && loss_out, "map_step: null argument");
    PSVO_REQUIRE(n_rays > 0 && adam_step >= 1, "map_step: bad sizes");
    PSVO_REQUIRE(d->width == 128 || d->width == 256, "map_step: decoder width %d unsupported (fused: 128, 256)",
                 d->width);
    MapStep s{e, st, d, fr, flags, n_rays, adam_step, rays_o, rays_d, gt_rgb, gt_depth, loss_out};
    // the normalisers from the query — single GPU the sampler's tail, data
    // parallel the query's second gather — only when the loss value is not
    // wanted (its reduction reads the counts k_crit_counts writes into the
    // loss partials)
    s.want_loss = !(flags & PSVO_STEP_NO_LOSS);
    s.counts_gt = !s.want_loss ? gt_depth : nullptr;
    ENG_CALL(take_query(e, st, d, s.R, rays_o, rays_d, seed, "map_step", &s.qset, noise, s.counts_gt));
    QueryGuard guard{e, st, s.qset};
    s.overlap = engine_overlap(e);
    if (s.overlap) ENG_CALL(ensure_aux(e));
    s.dist = e->x.on();
    s.ax = s.overlap ? e->aux : st;
    s.lq = (s.overlap && !s.dist) ? e->lossq : s.ax;
    s.ahead = fr && fr->next_dirs_cam;
    s.split = psvo::mlp_bwd_split_tail(d->width) && s.overlap && s.ahead && !s.no_adam();
    s.eb = s.split ? st : s.ax;
    // sparse-exact Adam (single GPU): the rows this step can touch, beside the
    // decoder — marked whenever the flags exist, also when the caller runs the
    // Adam step itself (PSVO_STEP_NO_ADAM, then psvo_map_adam): a later fused
    // step must still find these rows (their moments are non-zero from now on)
    const bool mark_rows = d->emb_row_flags && !s.dist;
    s.sparse_rows = mark_rows && !s.no_adam();
    // data parallel: this rank's rows into emb_row_local (the row-sparse
    // exchange lists them; the union flags come from what it exchanged)
    s.mark_into = mark_rows ? d->emb_row_flags : (s.dist ? d->emb_row_local : nullptr);
    // the look-ahead's inputs made on another stream: its position now, waited
    // for by the look-ahead's pose step only (psvo_map_frames.next_stream)
    s.wait_next = s.ahead && fr->next_stream && as_stream(fr->next_stream) != st;
    if (s.wait_next) {
        ENG_CALL(ensure_aux(e));
        ENG_CALL(ev_record(e->next_ready, as_stream(fr->next_stream), "map_step"));
    }
    // aux waits for z only to count the normalisers itself, or to mark the
    // rows the width-256 backward's scatter will touch
    const bool coef_known = s.counts_gt && s.qset->counts_gt == s.counts_gt;
    const bool need_z = !coef_known || s.dist || (d->emb_row_flags && !psvo::mlp_bwd_fuses_interp(d->width));
    const MapRender mr{e, st, d, *s.qset, rays_o, rays_d, "map_step", !(e->paths & PSVO_PATH_PADDED),
                       !(e->paths & PSVO_PATH_DENSE_DECODER), need_z};
    ENG_CALL(render_map(mr, stats_out, s.q));
    if (s.q.z_recorded) ENG_CALL(st_wait(s.ax, e->z_ready, "map_step"));
    s.empty = s.dist && (s.q.r_hit == 0 || s.q.m == 0);
    s.n_hit = s.dist ? s.qset->host_stats[PSVO_STAT_R_HIT] : s.q.r_hit;

    ENG_CALL(step_select(s));       // sparse: sample selection + the kept samples' decoder forward
    ENG_CALL(step_normalisers(s));  // ax: loss coefficients; st waits for them
    ENG_CALL(step_loss(s));         // st: fused loss pass; lq: the loss value
    ENG_CALL(step_grad_buffers(s));
    if (s.empty) return step_empty(s, guard);
    ENG_CALL(step_backward(s));     // st: decoder backward; eb: embedding backward
    e->tm.pending = e->tm.on;
    ENG_CALL(guard.release());
    return step_tail(s);            // poses / look-ahead, optimiser, next images, clock
}

}  // namespace

extern "C" int psvo_engine_grad_rays(psvo_engine *e, void *stream, int64_t n_rays, float *grad_o, float *grad_d) {
    PSVO_REQUIRE(e && grad_o && grad_d && n_rays > 0, "engine_grad_rays: bad arguments");
    const size_t bytes = (size_t)n_rays * 3 * sizeof(float);
    PSVO_REQUIRE(e->a.p[kGradOD] && e->a.cap[kGradOD] >= 2 * bytes, "engine_grad_rays: no step of %lld rays ran",
                 (long long)n_rays);
    const float *g = static_cast<const float *>(e->a.p[kGradOD]);
    hipStream_t st = as_stream(stream);
    if (hipMemcpyAsync(grad_o, g, bytes, hipMemcpyDeviceToDevice, st) != hipSuccess ||
        hipMemcpyAsync(grad_d, g + n_rays * 3, bytes, hipMemcpyDeviceToDevice, st) != hipSuccess)
        return set_error(PSVO_E_LAUNCH, "engine_grad_rays: copy failed");
    return PSVO_OK;
}

extern "C" int psvo_map_step(psvo_engine *e, void *stream, const psvo_map_desc *d, int64_t n_rays,
                             const float *rays_o, const float *rays_d, const float *gt_rgb, const float *gt_depth,
                             uint64_t seed, int64_t adam_step, int flags, float *loss_out, int *stats_out) {
    return map_step_impl(e, as_stream(stream), d, n_rays, rays_o, rays_d, gt_rgb, gt_depth, nullptr, seed, adam_step,
                         flags, loss_out, stats_out, nullptr);
}

extern "C" int psvo_map_step_frames(psvo_engine *e, void *stream, const psvo_map_desc *d, const psvo_map_frames *fr,
                                    const float *gt_rgb, const float *gt_depth, const float *noise, uint64_t seed,
                                    int64_t adam_step, int flags, float *loss_out, int *stats_out) {
    PSVO_REQUIRE(e && d && fr && fr->dirs_cam && fr->poses && fr->pose_step, "map_step_frames: null argument");
    PSVO_REQUIRE(fr->n_frames > 0 && fr->rays_per_frame > 0, "map_step_frames: bad sizes");
    PSVO_REQUIRE(fr->n_frames <= kXchMaxFrames, "map_step_frames: at most %d keyframes per call (rank)",
                 kXchMaxFrames);
    for (int f = 0; f < fr->n_frames; ++f)
        PSVO_REQUIRE(fr->pose_step[f] < 1 || (fr->pose_m && fr->pose_v), "map_step_frames: pose Adam needs m / v");
    PSVO_REQUIRE(!(fr->next_dirs_cam && noise), "map_step_frames: look-ahead needs drawn (not injected) noise");
    hipStream_t st = as_stream(stream);
    int rc = PSVO_OK;
    const int64_t R = (int64_t)fr->n_frames * fr->rays_per_frame;
    if (e->q_count > 0) {  // the previous call's look-ahead: rays and query made from the updated poses
        const QuerySet &q = e->qs[e->q_head];
        PSVO_REQUIRE(q.dirs != nullptr && q.dirs == fr->dirs_cam && q.R == R && q.seed == seed && !noise,
                     "map_step_frames: dirs_cam / seed differ from the previous call's next_dirs_cam / next_seed");
        return map_step_impl(e, st, d, R, q.ro, q.rd, gt_rgb, gt_depth, nullptr, seed, adam_step, flags, loss_out,
                             stats_out, fr);
    }
    ENG_BUF(float, rays_o, kRaysO, (size_t)R * 3 * sizeof(float));
    ENG_BUF(float, rays_d, kRaysD, (size_t)R * 3 * sizeof(float));
    ENG_CALL(psvo_pose_rays_frames(st, R, fr->rays_per_frame, fr->poses, fr->dirs_cam, rays_o, rays_d));
    return map_step_impl(e, st, d, R, rays_o, rays_d, gt_rgb, gt_depth, noise, seed, adam_step, flags, loss_out,
                         stats_out, fr);
}

extern "C" int psvo_track_step(psvo_engine *e, void *stream, const psvo_map_desc *d, int64_t n_rays,
                               const float *dirs_cam, const float *gt_rgb, const float *gt_depth, float *pose,
                               float *pose_m, float *pose_v, double lr, const float *noise, uint64_t seed,
                               int64_t adam_step, int flags, float *pose_grad, float *loss_out, int *stats_out) {
    PSVO_REQUIRE(e && d && dirs_cam && gt_rgb && gt_depth && pose && loss_out, "track_step: null argument");
    e->images_next = false;  // the weights may change before the next step
    PSVO_REQUIRE(n_rays > 0 && adam_step >= 1, "track_step: bad sizes");
    PSVO_REQUIRE(d->width == 128 || d->width == 256, "track_step: decoder width %d unsupported (fused: 128, 256)",
                 d->width);
    PSVO_REQUIRE((flags & PSVO_STEP_NO_ADAM) || (pose_m && pose_v), "track_step: Adam needs pose_m / pose_v");
    hipStream_t st = as_stream(stream);
    int rc = PSVO_OK;
    const int64_t R = n_rays;
    // ---- world rays from the pose (render_helpers.py:714-716)
    ENG_BUF(float, rays_o, kRaysO, (size_t)R * 3 * sizeof(float));
    ENG_BUF(float, rays_d, kRaysD, (size_t)R * 3 * sizeof(float));
    ENG_CALL(psvo_pose_rays(stream, R, pose, dirs_cam, rays_o, rays_d));
    Render q;
    PSVO_REQUIRE(e->q_count == 0, "track_step: the engine has queued mapping queries");
    PSVO_REQUIRE(!e->x.on(), "track_step: tracking runs on one GPU (SURVEY §8e: its median filter is global)");
    QuerySet *qset = nullptr;
    ENG_CALL(take_query(e, st, d, R, rays_o, rays_d, seed, "track_step", &qset, noise));
    QueryGuard guard{e, st, qset};
    ENG_CALL(render_track(e, st, d, *qset, rays_o, rays_d, stats_out, "track_step", q));
    // ---- loss (optionally with the median depth filter) and backward
    float *dtmp = nullptr, *dthr = nullptr;
    if (flags & PSVO_TRACK_DEPTH_FILTER) {
        ENG_BUF(float, tbuf, kDTmp, (size_t)q.r_hit * sizeof(float) + 64);
        dtmp = tbuf;
        dthr = tbuf + ((q.r_hit + 15) / 16) * 16;
        ENG_CALL(psvo_criterion_depth_filter(stream, q.r_hit, q.s_max, q.rank_ray, gt_depth, q.depth, q.weights,
                                             q.z_vals, dtmp, dthr));
    }
    float *g_sdf_s, *g_rgb_s;
    ENG_CALL(loss_backward(e, st, d, q, gt_rgb, gt_depth, dtmp, dthr, loss_out, &g_sdf_s, &g_rgb_s));
    // frozen map: decoder backward to the features only, interpolation
    // backward to the rays only (no embedding scatter)
    const int64_t M = q.m;
    ENG_BUF(float, dfeat, kDfeat, M * 16 * sizeof(float));
    const int n_split = 256;
    ENG_BUF(float, mlp_ws, kMlpWs, psvo_mlp_workspace_floats_w(M, d->width, n_split) * sizeof(float));
    mark(e, st, PSVO_TIME_MLP_BWD, 0);
    ENG_CALL(mlp_bwd(stream, M, d->width, q.s.feat, q.images, q.s.rgb_s, nullptr, q.s.masks, g_sdf_s, g_rgb_s, dfeat,
                     nullptr, 0, n_split, mlp_ws, nullptr));
    mark(e, st, PSVO_TIME_MLP_BWD, 1);
    ENG_BUF(float, grad_od, kGradOD, (size_t)R * 6 * sizeof(float));
    mark(e, st, PSVO_TIME_INTERP_BWD, 0);
    ENG_CALL(psvo_interp_bwd(stream, q.r_hit, 16, d->voxel_size, q.s.offsets, q.rank_ray, q.s.leaf, q.s.tt, rays_o,
                             rays_d, d->centres, d->vertex_idx, d->emb, dfeat, nullptr, grad_od, grad_od + R * 3));
    mark(e, st, PSVO_TIME_INTERP_BWD, 1);
    e->tm.pending = e->tm.on;
    ENG_CALL(guard.release());
    // ---- pose gradient through rotation() and the pose's Adam step
    if (!pose_grad) {
        ENG_BUF(float, gbuf, kPoseGrad, 8 * sizeof(float));
        pose_grad = gbuf;
    }
    ENG_CALL(psvo_pose_grad(stream, q.r_hit, q.rank_ray, dirs_cam, grad_od, grad_od + R * 3, pose, pose_grad));
    if (!(flags & PSVO_STEP_NO_ADAM)) {
        int64_t n6 = 6;
        int zero = 0;
        const float *g = pose_grad;
        ENG_CALL(adam_launch(st, 1, &pose, &g, &pose_m, &pose_v, &n6, &lr, d->beta1, d->beta2, d->eps, 0.0, adam_step,
                             &zero));
    }
    return PSVO_OK;
}
