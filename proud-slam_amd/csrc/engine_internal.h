// The native engine's state and the helpers its three translation units
// share: engine.cpp (lifecycle, setters, timing / clock, Adam entry points),
// engine_query.cpp (query sets: enqueue, second half, wait / take / release)
// and engine_step.cpp (render paths, mapping and tracking steps).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <time.h>

#include <vector>

#include "psvo_common.h"
#include "lookback.h"
#include "query.h"

namespace psvo {

// buffers of one query (intersection + sampling of a ray batch): a query set
enum QSlot { kStats, kHitIdx, kHitT0, kHitT1, kRayNv, kRayDsum, kRayRank, kRankRay, kSIdx, kSDepth, kSDist, kRayNs,
             kOffsets, kBlkOut, kRayCnt, kCoefQ, kLbDesc, kLeafQ, kTQ, kRayOfQ, kDistSums, kMDev, kNvRank, kCol0Rank,
             kQSlots };
// buffers of the rest of a step
enum Slot {
    kLeaf, kT, kRayOf, kZ, kMask, kFeat, kImages, kSdfS, kRgbS, kAct, kMasks, kSdf, kWeights, kColor,
    kDepth, kZmin, kCritWs, kSums, kGLoss, kGColor, kGDepth, kGSdf, kGSdfS, kGRgbS, kMlpWs, kDfeat, kDecGrad,
    kGradEmb, kGradOD, kRaysO, kRaysD, kDTmp, kPoseGrad, kSumsC, kCoef, kIbWs,
    // the sparse decoder (select_samples): compact index, ray offsets, the kept samples' rows, counts, look-back
    kCidx, kOffB, kFeatB, kLeafB, kTB, kRayOfB, kSdfB, kSelCnt, kSelDesc,
    // its class B (the trunk only): ray offsets, activations and masks
    kOffB2, kH2, kSrcC, kSlots
};

struct Arena {
    void *p[kSlots] = {};
    size_t cap[kSlots] = {};
    uint32_t gen[kSlots] = {};  // allocations made for the slot (a new buffer may reuse a freed base address)
};

// One ray batch's query: its buffers, the pinned statistics it reads back
// and the events that order it against the steps.  psvo_map_query runs a
// query on the engine's side stream one step ahead (the query depends only on
// the rays and the octree, not on the embeddings / decoder the running step
// updates), so the step that consumes it finds its sizes already on the host.
struct QuerySet {
    Arena a;                      // slots kStats..kOffsets
    // coherent pinned {seq, value} granules: PSVO_STAT_WORDS for the read-back
    // after the sampler, PSVO_STAT_WORDS more for a data-parallel query's second
    unsigned long long *host_raw = nullptr;
    int host_stats[PSVO_STAT_WORDS] = {};     // the values of the last statistics that landed
    int seq = 0;                  // the flag value the current statistics carry
    hipStream_t qstream = nullptr;  // the stream the query was queued on
    const int *stats_zeroed = nullptr;  // the device statistics buffer a completed read-back left zeroed
    uint32_t lb_zero_gen = 0;           // the look-back descriptor allocation (Arena::gen) last zeroed (tags ≠ 0)
    bool compacted = false;             // the sampler compacted the samples (slots kLeafQ / kTQ / kRayOfQ)
    hipEvent_t done = nullptr;    // statistics landed (after the sampler)
    bool done_recorded = false;   // a query consumed on its own stream skips it (one packet less there)
    hipEvent_t freed = nullptr;   // the consuming step finished with the buffers
    bool freed_recorded = false;
    hipStream_t freed_on = nullptr;  // the stream `freed` was recorded on (a wait on that stream is implied)
    bool freed_lazy = false;         // released on freed_on, event not recorded yet (a consumer on
                                     // another stream records it then: a later point of freed_on)
    bool pending = false;
    int64_t R = 0;
    const float *ro = nullptr, *rd = nullptr;
    const float *dirs = nullptr;  // a psvo_map_step_frames look-ahead: the camera directions it was made from
    // the GT depths the sampler counted the Criterion's normalisers with
    // (coefficients in slot kCoefQ), or null: the step computes them itself
    const float *counts_gt = nullptr;
    uint64_t seed = 0;
    int max_steps = 0;
    // data parallel: the query's second half — dist_counts → the all-gather of
    // [S_max, count words] → dist_smax → the second read-back — on the
    // engine's q2 stream, issued by the step once its interpolation and sdf
    // trunk are queued (query_phase2), so it runs beside them instead of on
    // the pose → traversal → sampler → interpolation chain
    hipEvent_t p1 = nullptr;     // the first read-back's kernel done (bound to its dispatch)
    hipEvent_t done2 = nullptr;  // the second read-back done
    bool p2_pending = false;     // queued first half, second half not issued yet
    const float *p2_gt = nullptr;
    float p2_tr = 0.f, p2_max_depth = 0.f;
};

}  // namespace psvo

// optional HIP-event timing of the roofline regions (PSVO_TIME_*)
struct EngineTimer {
    bool on = false;
    bool overlap = false;  // mode 2: events on the streams the regions run on, side streams kept
    bool pending = false;  // events of the last step not yet read
    bool markers = false;  // PSVO_TIMING_MARKERS=1: marker events around each region (the old timing)
    unsigned used = 0;     // regions the last step marked (a step may skip one: no compaction kernel)
    hipEvent_t ev[PSVO_TIME_REGIONS][2] = {};
    double ms[PSVO_TIME_REGIONS] = {};
    int64_t n[PSVO_TIME_REGIONS] = {};
    // kernel-bound timing (the default): the regions' kernels' own spans
    psvo::KernelClock kc;
    double kms[PSVO_TIME_REGIONS] = {};     // Σ kernel spans collected
    int64_t starts[PSVO_TIME_REGIONS] = {};  // region instances queued (a region's time = kms / starts)
};

// Data-parallel exchange (psvo_engine_set_exchange): the caller's collective
// callback and the device buffers it operates on.
struct EngineExchange {
    psvo_exchange_fn fn = nullptr;
    void *user = nullptr;
    int rank = 0, world = 1;
    int nch = 1;               // launch chunks the slot-0 table covers
    int cw = 8;                // words per rank of the query's first gather (dist_count_words(max_rays_rank))
    int64_t max_rays_rank = 0;
    int *xi32 = nullptr;       // psvo_engine_exchange_words(world, max_rays_global, max_rays_rank) int32
    double *xf64 = nullptr;    // 16 doubles: [0, 8) count sums, [8, 16) loss sums
    bool on() const { return fn != nullptr; }  // world 1 included: the one-rank protocol (tests)
    // int32 word offsets: [first gather: in | all ranks] [second gather: in | all ranks] [slot-0 count table]
    int64_t in_off() const { return 0; }
    int64_t all_off() const { return cw; }
    int64_t q2_in_off() const { return all_off() + (int64_t)world * cw; }
    int64_t q2_all_off() const { return q2_in_off() + psvo::kDistWordsPerRank; }
    int64_t table_off() const { return (q2_all_off() + (int64_t)world * psvo::kDistWordsPerRank + 63) / 64 * 64; }
    int64_t table_words() const { return (int64_t)psvo::kSamplerG * nch; }
    int call(int op, int64_t in, int64_t out, int64_t count, hipStream_t st, const char *what) const {
        const int rc = fn(user, op, in, out, count, st);
        if (rc != 0) return psvo::set_error(PSVO_E_LAUNCH, "exchange (%s) failed with %d", what, rc);
        return PSVO_OK;
    }
};

// psvo_engine_set_clock: an event on the caller's stream at the entry of
// every mapping step — the GPU reaches it when the previous step's work on
// that stream (through the look-ahead query) is done, so consecutive events
// are the iteration period as the GPU runs it
struct EngineClock {
    std::vector<hipEvent_t> ev;
    int n = 0;
    bool on = false;
};

struct psvo_engine {
    EngineExchange x;
    EngineClock clk;
    psvo::Arena a;
    psvo::QuerySet qs[2];           // FIFO of queries: head = the next step's
    int q_head = 0, q_count = 0;
    uint32_t lb_tag = 0;            // the last look-back descriptor tag handed out (lookback.h)
    hipStream_t side = nullptr;     // psvo_map_query's stream
    hipStream_t q2s = nullptr;      // data parallel: the queries' second halves (QuerySet::p2_pending)
    hipEvent_t in_ready = nullptr;  // the caller's stream position at psvo_map_query
    // the embedding backward runs on `aux` beside the decoder's weight
    // gradients where the decoder's backward does not run it itself (width
    // 256: k_interp_bwd's 8-KB workgroups fit next to k_dec256_dw's 104 KB)
    // (and the loss normalisers beside the decoder forward; data parallel,
    // also the loss value beside the decoder backward)
    hipStream_t aux = nullptr;
    // single GPU: the loss value (one-wave reduction, slow beside the
    // persistent decoder kernels) on its own stream, so it delays neither the
    // embedding backward on aux nor anything on the caller's stream
    hipStream_t lossq = nullptr;
    hipEvent_t dfeat_ready = nullptr, emb_done = nullptr, z_ready = nullptr, coef_ready = nullptr,
               grads_ready = nullptr, prep_fork = nullptr, prep_done = nullptr, loss_done = nullptr;
    // a look-ahead step's tail split (step_tail): the weight-gradient sum,
    // the optimiser step and the next decoder images on aux, while st runs the
    // pose step and the next query; every later reader of the weights on st
    // waits for adam_done first (the render paths, before the interpolation)
    hipEvent_t adam_done = nullptr;
    bool bwd_recorded = false;     // dfeat_ready holds a step's decoder backward end (psvo_map_side_wait)
    bool adam_pending = false;
    hipEvent_t next_ready = nullptr;  // psvo_map_frames.next_stream's position at the call
    hipEvent_t draw_gate = nullptr;   // the last step's sample selection done (psvo_engine_gate_stream)
    hipEvent_t draw_gate_ev = nullptr;  // the event that marks it: draw_gate, or a timed step's clock event
    bool draw_gate_recorded = false;
    bool draw_gate_used = false;      // a caller gates on it: bind it to the selections from now on
    EngineTimer tm;
    // the decoder images a look-ahead step built on st after its Adam step,
    // for the decoder whose W[0] it names; consumed by the next
    // psvo_map_step_frames, dropped by every other call
    bool images_next = false;
    const float *images_w0 = nullptr;
    int paths = 0;                  // PSVO_PATH_* (psvo_engine_set_paths)
    int64_t m_early = 0;            // the device-sized forward's capacity (device_forward): 1.25 × the largest M seen
    uint32_t sel_tag = 0;           // the sample selection's look-back descriptor tag
    uint32_t sel_zero_gen = 0;      // its descriptor allocation (Arena::gen) last zeroed
    int *host_flags = nullptr;      // coherent pinned: bit 3 = a sample selection gave up its look-back wait
    bool grads_clean = false;       // embedding-gradient buffer known to be zero (Adam zeroes it)
    const float *clean_buf = nullptr;  // ... and which buffer that is
    psvo::RenderWs *render = nullptr;  // psvo_render_frame's buffers (render.hip owns the type)
};

#define ENG_CALL(x)                     \
    do {                                \
        const int _rc = (x);            \
        if (_rc != PSVO_OK) return _rc; \
    } while (0)

// `T *name` = the engine's buffer of `slot` (query set q's for Q_BUF), at
// least `bytes`; needs `int rc` and the stream `st` in scope
#define ENG_BUF(T, name, slot, bytes)                                              \
    T *name = reinterpret_cast<T *>(arena_buf(e->a, st, slot, (bytes), &rc));     \
    if (!name) return rc;
#define Q_BUF(T, name, slot, bytes)                                              \
    T *name = reinterpret_cast<T *>(arena_buf(q.a, st, slot, (bytes), &rc));    \
    if (!name) return rc;

// shared between the engine's translation units only: not exported
#pragma GCC visibility push(hidden)
namespace psvo {
namespace eng {

// ---- stream ordering: one HIP call each, PSVO_OK or the error set.  Which
// stream waits for what is decided at the call sites; on the caller's stream
// a marker packet between two dependent kernels costs ≈ 5 µs, so no helper
// records or waits more than it is told to.
inline int ev_record(hipEvent_t ev, hipStream_t st, const char *who) {
    if (hipEventRecord(ev, st) == hipSuccess) return PSVO_OK;
    return set_error(PSVO_E_LAUNCH, "%s: event record failed", who);
}
inline int st_wait(hipStream_t st, hipEvent_t ev, const char *who) {
    if (hipStreamWaitEvent(st, ev, 0) == hipSuccess) return PSVO_OK;
    return set_error(PSVO_E_LAUNCH, "%s: stream wait failed", who);
}
inline int zero_async(void *p, size_t bytes, hipStream_t st, const char *who) {
    if (hipMemsetAsync(p, 0, bytes, st) == hipSuccess) return PSVO_OK;
    return set_error(PSVO_E_LAUNCH, "%s: memset failed", who);
}
// `st` waits for `ev` recorded on `from` now (no-op when from == st)
inline int fork_join(hipStream_t from, hipStream_t st, hipEvent_t ev) {
    if (from == st) return PSVO_OK;
    ENG_CALL(ev_record(ev, from, "engine"));
    return st_wait(st, ev, "engine");
}

inline double now_ns() {
    timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return t.tv_sec * 1e9 + t.tv_nsec;
}

// ---- engine.cpp (each described at its definition)
void *arena_buf(Arena &a, hipStream_t st, int slot, size_t bytes, int *rc);
void timer_collect(psvo_engine *e, bool block = false);
// open (end = 0) / close (end = 1) a timed region on `st`
void mark(psvo_engine *e, hipStream_t st, int region, int end);
int join_adam(psvo_engine *e, hipStream_t st, const char *who, double host_wait_us = 0.0);
// Work beside the main stream on `aux` (timed runs in mode 1: everything on
// the caller's stream, in dependency order).
inline bool engine_overlap(psvo_engine *e) { return !e->tm.on || e->tm.overlap; }
int ensure_aux(psvo_engine *e);
void dec_sizes(int W, int64_t (&n)[10]);
// the keyframe poses' Adam steps of a psvo_map_step_frames iteration, queued
// with the map's (one launch) or alone (data parallel: the map waits for the
// gradient all-reduce)
struct PoseAdam {
    int n = 0;
    float *p[kXchMaxFrames], *m[kXchMaxFrames], *v[kXchMaxFrames];
    const float *g[kXchMaxFrames];
    int64_t step[kXchMaxFrames];
    double lr = 0.0;
};
int map_adam(hipStream_t st, const psvo_map_desc *d, float *grads, int64_t adam_step, const PoseAdam *pa = nullptr,
             bool sparse_rows = false);
int pose_adam(hipStream_t st, const psvo_map_desc *d, const PoseAdam &pa);

// ---- engine_query.cpp (each described at its definition)
int query_set_init(QuerySet &s);
void query_set_free(QuerySet &s);
void host_wait_report();  // PSVO_HOST_WAIT_STATS=1: the host's time in the statistics waits, to stderr
int query_enqueue(psvo_engine *e, hipStream_t st, QuerySet &q, const psvo_map_desc *d, int64_t R,
                  const float *rays_o, const float *rays_d, uint64_t seed, const char *who,
                  const float *noise = nullptr, bool record_done = true, const float *counts_gt = nullptr);
int take_query(psvo_engine *e, hipStream_t st, const psvo_map_desc *d, int64_t R, const float *rays_o,
               const float *rays_d, uint64_t seed, const char *who, QuerySet **out, const float *noise = nullptr,
               const float *counts_gt = nullptr);
int freed_wait(QuerySet &q, hipStream_t s);
int release_query(psvo_engine *e, hipStream_t st, QuerySet *q);
// Drops the step's query set if the step fails after take_query: without it a
// failed batch (no hit ray, sampler overflow) would stay at the FIFO head and
// every later step would be refused as "rays differ from the queued batch".
struct QueryGuard {
    psvo_engine *e;
    hipStream_t st;
    QuerySet *q = nullptr;
    ~QueryGuard() {
        if (q) (void)release_query(e, st, q);
    }
    int release() {
        QuerySet *x = q;
        q = nullptr;
        return release_query(e, st, x);
    }
};
// What a step learns from its query's statistics once they are on the host.
struct Readback {
    int64_t r_hit = 0;     // hit rays (data parallel: this rank's, padded to the union's S_max)
    int64_t m = 0;         // valid samples
    int s_max = 0;         // (a deferred second half: the rank's own until query_readback_late)
    bool p2_late = false;  // data parallel: the second half is still to be issued (query_readback_late)
    bool empty = false;    // data parallel: a shard without samples — it still joins the collectives
};
// Waits for the statistics and decodes them: the flags become errors, the
// sizes go to `rb` (and, unless deferred, the words to stats_out if not null).
// Data parallel, the query's second half (the union S_max) is issued and
// waited for here — or, with defer_p2 and a shard that has samples, left to
// query_readback_late, so that the caller first queues what does not need it.
int query_readback(psvo_engine *e, QuerySet &q, bool defer_p2, int *stats_out, const char *who, Readback &rb);
int query_readback_late(psvo_engine *e, QuerySet &q, int *stats_out, const char *who, Readback &rb);

}  // namespace eng
}  // namespace psvo
#pragma GCC visibility pop
