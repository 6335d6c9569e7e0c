// The engine's query sets: a ray batch's intersection + sampling queued on a
// stream (query_enqueue), a data-parallel query's second half (query_phase2),
// the host's wait for the statistics and their decoding (query_readback), and
// the FIFO of queries made ahead of their steps (take / release / discard).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "engine_internal.h"

using namespace psvo;
using namespace psvo::eng;

namespace psvo {
namespace eng {

// The host spins on the statistics granules the device writes (each word
// tagged with the query's seq, relaxed system-scope stores: stat_to_host) —
// it sees them as soon as they land, without the event's completion-signal
// round trip and without a system-scope release on the device; the event
// recorded after that kernel (or, without one, the query's stream) is still
// queried now and then so a failed stream ends the wait with its error.
// PSVO_HOST_WAIT_STATS=1: the host's time in these waits, printed when the
// engine is freed (is the iteration host-bound? a host that never waits is)
struct HostWait {
    double ns = 0;
    long calls = 0, spun = 0;
};
static HostWait g_host_wait;
// every granule tagged `seq`: decode the values into out
static bool stats_landed(const unsigned long long *raw, int seq, int *out) {
    int v[PSVO_STAT_WORDS];
    for (int k = 0; k < PSVO_STAT_WORDS; ++k) {
        const unsigned long long g = __atomic_load_n(raw + k, __ATOMIC_ACQUIRE);
        if ((int)(g >> 32) != seq) return false;
        v[k] = (int)(unsigned)g;
    }
    memcpy(out, v, sizeof(v));
    return true;
}
static int spin_wait_impl(QuerySet &q, hipEvent_t ev, hipStream_t qs, const char *who, int part);
// part 0: the read-back after the sampler; 1: a data-parallel query's second
static int spin_wait(QuerySet &q, hipEvent_t ev, hipStream_t qs, const char *who, int part = 0) {
    int tmp[PSVO_STAT_WORDS];
    const bool ready = stats_landed(q.host_raw + part * PSVO_STAT_WORDS, q.seq, tmp);
    const double t0 = now_ns();
    const int rc = spin_wait_impl(q, ev, qs, who, part);
    g_host_wait.ns += now_ns() - t0;
    g_host_wait.calls += 1;
    g_host_wait.spun += ready ? 0 : 1;
    return rc;
}
static int spin_wait_impl(QuerySet &q, hipEvent_t ev, hipStream_t qs, const char *who, int part) {
    // the runtime query (error detection only) costs microseconds: at most one
    // per 0.5 ms of waiting, so the statistics are seen as soon as they land
    const unsigned long long *raw = q.host_raw + part * PSVO_STAT_WORDS;
    double next_query = now_ns() + 5e5;
    for (unsigned it = 1;; ++it) {
        if (stats_landed(raw, q.seq, q.host_stats)) return PSVO_OK;
        if ((it & 255) == 0 && now_ns() >= next_query) {
            next_query = now_ns() + 5e5;
            const hipError_t e = ev ? hipEventQuery(ev) : hipStreamQuery(qs);
            if (e == hipErrorNotReady) continue;
            if (e != hipSuccess) return set_error(PSVO_E_LAUNCH, "%s: stats read-back: %s", who, hipGetErrorString(e));
            // the event (no system-scope fence) may complete just before the
            // kernel's system-scope granule stores are visible: poll a while more
            for (unsigned k = 0; k < (1u << 22); ++k)
                if (stats_landed(raw, q.seq, q.host_stats)) return PSVO_OK;
            return set_error(PSVO_E_LAUNCH, "%s: stats read-back: event complete, granules not tagged %d", who,
                             q.seq);
        }
    }
}

int query_set_init(QuerySet &s) {
    if (s.host_raw) return PSVO_OK;
    if (hipHostMalloc(reinterpret_cast<void **>(&s.host_raw), 2 * PSVO_STAT_WORDS * sizeof(unsigned long long),
                      hipHostMallocCoherent | hipHostMallocMapped) !=
            hipSuccess ||
        // device-side ordering only: the statistics reach the host through the
        // scan kernel's own system-scope release (k_scan_samples / k_stats_to_host)
        hipEventCreateWithFlags(&s.done, hipEventDisableTiming | hipEventDisableSystemFence) != hipSuccess ||
        hipEventCreateWithFlags(&s.freed, hipEventDisableTiming | hipEventDisableSystemFence) != hipSuccess ||
        // (bound to a dispatch as its stop event: a timing event)
        hipEventCreateWithFlags(&s.p1, hipEventDisableSystemFence) != hipSuccess ||
        hipEventCreateWithFlags(&s.done2, hipEventDisableTiming | hipEventDisableSystemFence) != hipSuccess)
        return set_error(PSVO_E_LAUNCH, "engine: query set allocation failed");
    // tag 0: no statistics yet (seq from 1)
    memset(s.host_raw, 0, 2 * PSVO_STAT_WORDS * sizeof(unsigned long long));
    return PSVO_OK;
}

void query_set_free(QuerySet &s) {
    for (int k = 0; k < kQSlots; ++k)
        if (s.a.p[k]) (void)hipFree(s.a.p[k]);
    if (s.host_raw) (void)hipHostFree(s.host_raw);
    if (s.done) (void)hipEventDestroy(s.done);
    if (s.freed) (void)hipEventDestroy(s.freed);
    if (s.p1) (void)hipEventDestroy(s.p1);
    if (s.done2) (void)hipEventDestroy(s.done2);
}

void host_wait_report() {
    static const bool report = getenv("PSVO_HOST_WAIT_STATS") && *getenv("PSVO_HOST_WAIT_STATS") == '1';
    if (report && g_host_wait.calls > 0)
        fprintf(stderr, "psvo: host waited for the query statistics %ld times (%ld not yet landed), %.1f us each\n",
                g_host_wait.calls, g_host_wait.spun, g_host_wait.ns / 1e3 / g_host_wait.calls);
}

// A data-parallel query's second half (QuerySet::p2_pending) on the q2
// stream, forked at the first read-back: the rank's [S_max, count words]
// (dist_counts), their all-gather on the query communicator, the union S_max
// and normaliser sums (dist_smax), the second read-back.  Nothing on the
// step's stream waits for it: the host does (render, before the first launch
// sized by S_max), and aux before it reads the sums.
static int query_phase2(psvo_engine *e, QuerySet &q, const char *who) {
    if (!q.p2_pending) return PSVO_OK;
    q.p2_pending = false;
    const EngineExchange &x = e->x;
    if (!e->q2s && hipStreamCreateWithFlags(&e->q2s, hipStreamNonBlocking) != hipSuccess)
        return set_error(PSVO_E_LAUNCH, "%s: stream creation failed", who);
    hipStream_t s2 = e->q2s;
    int *stats = static_cast<int *>(q.a.p[kStats]);
    int *in = x.xi32 + x.q2_in_off();
    // (the count words start at zero, whatever a failed earlier half left)
    ENG_CALL(st_wait(s2, q.p1, who));
    ENG_CALL(zero_async(in + 1, (kDistWordsPerRank - 1) * sizeof(int), s2, who));
    ENG_CALL(dist_counts(s2, q.R, stats, static_cast<const int *>(q.a.p[kRankRay]), q.p2_gt,
                         static_cast<const float *>(q.a.p[kSDepth]), q.max_steps,
                         static_cast<const int *>(q.a.p[kRayNs]), q.p2_tr, q.p2_max_depth, in));
    ENG_CALL(x.call(PSVO_XCH_GATHER_I32 | PSVO_XCH_QUERY, x.q2_in_off(), x.q2_all_off(), kDistWordsPerRank, s2,
                    "S_max + counts"));
    ENG_CALL(dist_smax(s2, x.xi32 + x.q2_all_off(), x.world, stats, in,
                       q.p2_gt ? static_cast<double *>(q.a.p[kDistSums]) : nullptr));
    ENG_CALL(psvo::stats_to_host(s2, stats, q.host_raw + PSVO_STAT_WORDS, PSVO_STAT_WORDS, q.seq));
    q.stats_zeroed = stats;
    return ev_record(q.done2, s2, who);
}

// every queued second half, oldest query first; `st` then follows them
static int flush_phase2(psvo_engine *e, hipStream_t st, const char *who) {
    for (int k = 0; k < 2; ++k) {
        QuerySet &o = e->qs[e->q_head ^ k];
        if (!o.p2_pending) continue;
        ENG_CALL(query_phase2(e, o, who));
        ENG_CALL(st_wait(st, o.done2, who));
    }
    return PSVO_OK;
}

// The query half of render_rays (render_helpers.py:363-413): intersection,
// hit ranks and sampling of one ray batch into query set `q` on stream `st`,
// then the 32-byte statistics read-back (event q.done).  The sampler reads P,
// R_hit and max ⌈steps⌉ from `stats` on the device; its buffers are [R, cap]
// with cap ≥ max_steps = max ⌈Σ(t_out − t_in)/step⌉ + P, bounded by 50 leaf
// intervals of at most a voxel diagonal (rows are written only up to
// max_steps; an overflow is flagged and reported by the consumer).
// The traversal is queued by query_intersect; QueryLb is what it hands on.
struct QueryLb {
    // the statistics / rank pass and the sample scan inside the traversal and
    // sampler launches (decoupled look-back; the sampler's only on one GPU)
    unsigned long long *lb = nullptr;
    uint32_t tag = 0;
    // with the look-back: each rank's hit count and first voxel id by rank
    // (the sampler's only reads of other rows, one load each)
    int *nv_rank = nullptr, *col0_rank = nullptr;
};
static int query_intersect(psvo_engine *e, hipStream_t st, QuerySet &q, const psvo_map_desc *d, int64_t R,
                           const float *rays_o, const float *rays_d, const char *who, QueryLb &l) {
    int rc = PSVO_OK;
    // data parallel: an earlier query's second half first — every rank issues
    // the collectives in query order, and this query's kernels follow that
    // half's reads of the buffers they overwrite
    ENG_CALL(flush_phase2(e, st, who));
    Q_BUF(int, stats, kStats, PSVO_STAT_WORDS * sizeof(int));
    if (q.stats_zeroed != stats) ENG_CALL(zero_async(stats, PSVO_STAT_WORDS * sizeof(int), st, who));
    q.stats_zeroed = nullptr;  // until this query's read-back is queued
    Q_BUF(int, hit_idx, kHitIdx, R * kMaxHits * sizeof(int));
    Q_BUF(float, hit_t0, kHitT0, R * kMaxHits * sizeof(float));
    Q_BUF(float, hit_t1, kHitT1, R * kMaxHits * sizeof(float));
    Q_BUF(int, ray_nv, kRayNv, R * sizeof(int));
    Q_BUF(float, ray_dsum, kRayDsum, R * sizeof(float));
    Q_BUF(int, ray_rank, kRayRank, R * sizeof(int));
    Q_BUF(int, rank_ray, kRankRay, R * sizeof(int));
    mark(e, st, PSVO_TIME_INTERSECT, 0);
    Q_BUF(int, blk_out, kBlkOut, (size_t)(R + 3) / 4 * 2 * sizeof(int));  // per intersect block: tests, rounds
    if (psvo::query_lookback(R) && !(e->paths & PSVO_PATH_QUERY_SPLIT)) {
        Q_BUF(unsigned long long, lb, kLbDesc, (size_t)psvo::lookback_granules(R) * sizeof(unsigned long long));
        // fresh memory (or after a reported failure): no stale granule may
        // carry a future tag, and the ticket counters start at 0 (lookback.h)
        if (q.lb_zero_gen != q.a.gen[kLbDesc]) {
            ENG_CALL(zero_async(lb, q.a.cap[kLbDesc], st, who));
            q.lb_zero_gen = q.a.gen[kLbDesc];
        }
        e->lb_tag = e->lb_tag == 0xffffffffu ? 1u : e->lb_tag + 1u;
        Q_BUF(int, nv_rank, kNvRank, R * sizeof(int));
        Q_BUF(int, col0_rank, kCol0Rank, R * sizeof(int));
        l = QueryLb{lb, e->lb_tag, nv_rank, col0_rank};
    }
    ENG_CALL(psvo::intersect_ranked(st, R, rays_o, rays_d, d->centres, d->structure, d->voxel_size,
                                    d->max_distance, d->step_size, hit_idx, hit_t0, hit_t1, ray_nv, ray_dsum, stats,
                                    ray_rank, rank_ray, static_cast<const PackRec *>(d->packed), blk_out, l.lb, l.tag,
                                    l.nv_rank, l.col0_rank, d->n_nodes));
    return PSVO_OK;
}

int query_enqueue(psvo_engine *e, hipStream_t st, QuerySet &q, const psvo_map_desc *d, int64_t R,
                  const float *rays_o, const float *rays_d, uint64_t seed, const char *who, const float *noise,
                  bool record_done, const float *counts_gt) {
    int rc = PSVO_OK;
    const EngineExchange &x = e->x;
    QueryLb l;
    ENG_CALL(query_intersect(e, st, q, d, R, rays_o, rays_d, who, l));
    int *stats = static_cast<int *>(q.a.p[kStats]);
    const int *rank_ray = static_cast<const int *>(q.a.p[kRankRay]);
    const int *hit_idx = static_cast<const int *>(q.a.p[kHitIdx]), *ray_nv = static_cast<const int *>(q.a.p[kRayNv]);
    const float *hit_t0 = static_cast<const float *>(q.a.p[kHitT0]);
    const float *hit_t1 = static_cast<const float *>(q.a.p[kHitT1]);
    const float *ray_dsum = static_cast<const float *>(q.a.p[kRayDsum]);
    if (x.on() && noise) return set_error(PSVO_E_INVALID, "%s: injected sampler noise is single-GPU only", who);
    if (x.on()) {  // union-batch layout: ONE all-gather (8 words + the hit rows' counts), then local
        if (R > x.max_rays_rank)
            return set_error(PSVO_E_INVALID, "%s: %lld rays exceed the exchange's max_rays_rank %lld", who,
                             (long long)R, (long long)x.max_rays_rank);
        // (a query without GT depths: the step counts the normalisers itself —
        // on every rank, decided from the gathered flags)
        ENG_CALL(dist_pack(st, R, stats, rank_ray, hit_idx, ray_nv, x.xi32 + x.in_off(), l.nv_rank,
                           counts_gt ? 0 : psvo::PSVO_FLAG_UNION_UNCOUNTED));
        ENG_CALL(x.call(PSVO_XCH_GATHER_I32 | PSVO_XCH_QUERY, x.in_off(), x.all_off(), x.cw, st, "query layout"));
        ENG_CALL(dist_layout(st, x.xi32 + x.all_off(), x.world, x.rank, x.cw, x.nch, stats, x.xi32 + x.table_off(),
                             nullptr));
    }
    mark(e, st, PSVO_TIME_INTERSECT, 1);
    const int max_steps = (int)ceil(kMaxHits * 1.7321 * 1.001 * (double)d->voxel_size / (double)d->step_size) +
                          kMaxHits + 1;
    Q_BUF(int, s_idx, kSIdx, (size_t)R * max_steps * sizeof(int));
    Q_BUF(float, s_depth, kSDepth, (size_t)R * max_steps * sizeof(float));
    // the sampler's distance rows (render_helpers' sampled_dists) are not read
    // on this path: the sampler skips them (nullptr)
    float *const s_dist = nullptr;
    Q_BUF(int, ray_ns, kRayNs, (size_t)R * sizeof(int));
    Q_BUF(int, offsets, kOffsets, (size_t)(R + 1) * sizeof(int));
    mark(e, st, PSVO_TIME_SAMPLE, 0);
    if (x.on()) {
        ENG_CALL(dist_sample(st, R, max_steps, rank_ray, hit_idx, hit_t0, hit_t1, ray_dsum, d->step_size, seed, stats,
                             x.xi32 + x.table_off(), x.nch, s_idx, s_depth, s_dist, ray_ns, offsets, l.nv_rank,
                             l.col0_rank));
        // S_max of the union (every rank pads its [R_hit, S_max] blocks to it)
        // and, given the step's GT depths, the loss normalisers' counts: ONE
        // all-gather of 8 words, in the query's second half (query_phase2)
        if (counts_gt) {
            Q_BUF(double, qs_, kDistSums, 8 * sizeof(double));
            (void)qs_;
        }
        q.p2_gt = counts_gt;
        q.p2_tr = d->truncation;
        q.p2_max_depth = d->max_depth;
    }
    q.seq = q.seq == 0x7fffffff ? 1 : q.seq + 1;
    q.counts_gt = x.on() ? counts_gt : nullptr;  // data parallel: the union's count sums in kDistSums
    q.compacted = false;
    if (!x.on()) {  // the sampler's scan does the read-back (and, given the GT depths, the loss normalisers)
        psvo::SampleCounts sc{};
        // the per-ray counts pack into 12-bit fields (query_sample.hip pack_counts):
        // rows that may hold more than 4095 samples count in the step instead (k_crit_counts)
        const bool counts = counts_gt != nullptr && max_steps <= 4095;
        if (counts) {
            Q_BUF(int, ray_cnt, kRayCnt, (size_t)R * sizeof(int));
            Q_BUF(float, coefq, kCoefQ, 4 * sizeof(float));
            sc = psvo::SampleCounts{counts_gt, ray_cnt, coefq, d->truncation, d->max_depth, d->w_rgb, d->w_depth,
                                    d->w_fs, d->w_sdf,
                                    PSVO_CRIT_USE_COLOR | PSVO_CRIT_USE_DEPTH | PSVO_CRIT_USE_SDF};
            q.counts_gt = counts_gt;
        }
        // look-back sampler: the ray-major compaction in the same launch
        // (capacity R · max_steps: every row fits); otherwise k_compact_rays after the read-back
        int *leaf_q = nullptr, *ray_of_q = nullptr, *m_dev = nullptr;
        float *t_q = nullptr;
        if (l.lb) {
            const size_t cap = (size_t)R * max_steps;
            Q_BUF(int, lq_, kLeafQ, cap * sizeof(int));
            Q_BUF(float, tq_, kTQ, cap * sizeof(float));
            Q_BUF(int, rq_, kRayOfQ, cap * sizeof(int));
            Q_BUF(int, md_, kMDev, sizeof(int));
            leaf_q = lq_, t_q = tq_, ray_of_q = rq_, m_dev = md_;
        }
        ENG_CALL(psvo::sample_rays_to_host(st, R, max_steps, rank_ray, hit_idx, hit_t0, hit_t1, ray_dsum,
                                           d->step_size, noise, seed, stats, s_idx, s_depth, s_dist, ray_ns, offsets,
                                           q.host_raw, q.seq, counts ? &sc : nullptr, l.lb, l.tag, leaf_q, t_q,
                                           ray_of_q, m_dev, l.nv_rank, l.col0_rank));
        q.compacted = leaf_q != nullptr;
    }
    mark(e, st, PSVO_TIME_SAMPLE, 1);
    if (x.on()) {
        // the first read-back (the shard's sizes and the union's R_hit / P /
        // flags), the words kept for the second half, whose stream forks here
        // (q.p1: bound to the read-back's dispatch when possible, else recorded after it)
        psvo::StopBind p1(q.p1);
        ENG_CALL(psvo::stats_to_host(st, stats, q.host_raw, PSVO_STAT_WORDS, q.seq, false));
        if (!p1.consumed()) ENG_CALL(ev_record(q.p1, st, who));
        q.p2_pending = true;
    }
    q.stats_zeroed = x.on() ? nullptr : stats;  // (data parallel: the second read-back zeroes them)
    q.done_recorded = record_done;
    if (record_done) ENG_CALL(ev_record(q.done, st, who));
    q.qstream = st;
    q.R = R;
    q.ro = rays_o;
    q.rd = rays_d;
    q.dirs = nullptr;
    q.seed = seed;
    q.max_steps = max_steps;
    return PSVO_OK;
}

// A query set for a step on `st` over (R, rays, seed): the queued one
// psvo_map_query prepared for exactly this batch, or a fresh query enqueued
// on `st` itself.
int take_query(psvo_engine *e, hipStream_t st, const psvo_map_desc *d, int64_t R, const float *rays_o,
               const float *rays_d, uint64_t seed, const char *who, QuerySet **out, const float *noise,
               const float *counts_gt) {
    if (e->q_count > 0) {
        QuerySet &q = e->qs[e->q_head];
        if (q.R != R || q.ro != rays_o || q.rd != rays_d || q.seed != seed)
            return set_error(PSVO_E_INVALID, "%s: rays / seed differ from the batch queued by psvo_map_query", who);
        // the step's kernels read the query's outputs: order the streams
        if (q.qstream != st) {
            // a look-ahead queued without the event: its stream's position now (at or after the query)
            if (!q.done_recorded) ENG_CALL(ev_record(q.done, q.qstream, who));
            q.done_recorded = true;
            ENG_CALL(st_wait(st, q.done, who));
        }
        *out = &q;
        return PSVO_OK;
    }
    QuerySet &q = e->qs[e->q_head];
    ENG_CALL(query_enqueue(e, st, q, d, R, rays_o, rays_d, seed, who, noise, true, counts_gt));
    *out = &q;
    return PSVO_OK;
}

int freed_wait(QuerySet &q, hipStream_t s) {
    if (q.freed_lazy) {
        if (q.freed_on == s) return PSVO_OK;
        ENG_CALL(ev_record(q.freed, q.freed_on, "engine"));
        q.freed_lazy = false;
        q.freed_recorded = true;
    }
    if (q.freed_recorded && q.freed_on != s) ENG_CALL(st_wait(s, q.freed, "engine"));
    return PSVO_OK;
}

int release_query(psvo_engine *e, hipStream_t st, QuerySet *q) {
    // no marker packet on st now (between two kernels one costs ≈ 5 µs):
    // a consumer on another stream records it when it needs it (freed_wait)
    q->freed_lazy = true;
    q->freed_recorded = false;
    q->freed_on = st;
    if (e->q_count > 0 && q == &e->qs[e->q_head]) {
        q->pending = false;
        e->q_head ^= 1;
        e->q_count--;
    }
    return PSVO_OK;
}

// A sample selection (k_select_samples) that gave up its look-back wait set
// bit 3 of the pinned host word: its step's loss and gradients were formed
// without the abandoned workgroups' samples.  Reported at the engine's next
// host read-back (the following step's statistics, or select_stats) — the
// step itself queues everything without a host round trip — and cleared
// once reported; the descriptors are re-zeroed before the next selection.
static int select_failed(psvo_engine *e, const char *who) {
    if (!e->host_flags) return PSVO_OK;
    volatile int *f = e->host_flags;
    if (!(*f & psvo::kLbFlagTimeout)) return PSVO_OK;
    *f = 0;
    e->sel_zero_gen = 0;
    return set_error(PSVO_E_LAUNCH, "%s: the previous step's sample selection abandoned a look-back wait", who);
}


// data parallel: the query's second half now — issued, then waited for
static int phase2_now(psvo_engine *e, QuerySet &q, const char *who) {
    ENG_CALL(query_phase2(e, q, who));
    return spin_wait(q, q.done2, e->q2s, who, 1);
}

int query_readback(psvo_engine *e, QuerySet &q, bool defer_p2, int *stats_out, const char *who, Readback &rb) {
    ENG_CALL(spin_wait(q, q.done_recorded ? q.done : nullptr, q.qstream, who));
    timer_collect(e);  // the previous step's events completed before this read-back
    const bool dist = e->x.on();
    const int *hs = q.host_stats;
    const int flags = hs[PSVO_STAT_FLAGS];
    // the errors, in this order (a look-back give-up leaves every other word undefined)
    if (flags & kLbFlagTimeout) {
        q.lb_zero_gen = 0;  // the next query re-zeroes the descriptors and ticket counters
        return set_error(PSVO_E_LAUNCH, "%s: query look-back wait abandoned", who);
    }
    ENG_CALL(select_failed(e, who));
    if (flags & kStatFlagDfsOverflow) return set_error(PSVO_E_OVERFLOW, "%s: octree deeper than the DFS stack", who);
    if (flags & kStatFlagUnionOverflow)
        return set_error(PSVO_E_OVERFLOW, "%s: union batch exceeds max_rays_global", who);
    if (hs[PSVO_STAT_R_HIT] == 0)
        return set_error(PSVO_E_INVALID, "%s: no ray hits the octree (render_helpers.py:388)", who);
    if (flags & kStatFlagSamplerOverflow) return set_error(PSVO_E_OVERFLOW, "%s: sampler exceeded max_steps", who);
    // data-parallel: this rank's hit rays, padded to the union's S_max
    rb.r_hit = dist ? hs[PSVO_STAT_R_HIT_LOCAL] : hs[PSVO_STAT_R_HIT];
    rb.m = hs[PSVO_STAT_M];
    rb.empty = dist && (rb.r_hit == 0 || rb.m == 0);
    // data parallel: the union S_max comes with the query's second half
    // (query_phase2) — the mapping step waits for it only after queueing the
    // interpolation and the sdf trunk, which do not need it; the padded
    // paths (and an empty shard, which still joins the collectives) now
    rb.p2_late = dist && defer_p2 && !rb.empty;
    if (dist && !rb.p2_late) ENG_CALL(phase2_now(e, q, who));
    rb.s_max = hs[PSVO_STAT_S_MAX];
    if (stats_out && !rb.p2_late) memcpy(stats_out, hs, PSVO_STAT_WORDS * sizeof(int));
    if (rb.m == 0 && !rb.empty) return set_error(PSVO_E_INVALID, "%s: no valid samples", who);
    return PSVO_OK;
}

int query_readback_late(psvo_engine *e, QuerySet &q, int *stats_out, const char *who, Readback &rb) {
    if (!rb.p2_late) return PSVO_OK;
    ENG_CALL(phase2_now(e, q, who));
    rb.p2_late = false;
    rb.s_max = q.host_stats[PSVO_STAT_S_MAX];
    if (stats_out) memcpy(stats_out, q.host_stats, PSVO_STAT_WORDS * sizeof(int));
    return PSVO_OK;
}

}  // namespace eng
}  // namespace psvo

extern "C" int psvo_engine_queued(psvo_engine *e) { return e ? e->q_count : 0; }

// Drop every queued query (their buffers are reused only after their side-
// stream work completed: the next query waits on the stream).
extern "C" int psvo_map_discard(psvo_engine *e) {
    PSVO_REQUIRE(e, "map_discard: null engine");
    e->images_next = false;
    // no caller stream to order: the optimiser step of a split tail completes here
    if (e->adam_pending) {
        if (hipEventSynchronize(e->adam_done) != hipSuccess)
            return set_error(PSVO_E_LAUNCH, "map_discard: optimiser step failed");
        e->adam_pending = false;
    }
    while (e->q_count > 0) {
        QuerySet &q = e->qs[e->q_head];
        // the stream the query was queued on: psvo_map_query's side stream,
        // or aux for a psvo_map_step_frames look-ahead
        hipStream_t qs = q.qstream;
        if (qs) ENG_CALL(ev_record(q.freed, qs, "map_discard"));
        q.freed_recorded = qs != nullptr;
        q.freed_lazy = false;
        q.freed_on = qs;
        q.pending = false;
        e->q_head ^= 1;
        e->q_count--;
    }
    return PSVO_OK;
}

extern "C" int psvo_host_wait_stats(double *wait_us, long long *calls, long long *waited, int reset) {
    PSVO_REQUIRE(wait_us && calls && waited, "host_wait_stats: null argument");
    *wait_us = g_host_wait.ns / 1e3;
    *calls = g_host_wait.calls;
    *waited = g_host_wait.spun;
    if (reset) g_host_wait = HostWait();
    return PSVO_OK;
}

extern "C" int psvo_map_query(psvo_engine *e, void *stream, const psvo_map_desc *d, int64_t n_rays,
                              const float *rays_o, const float *rays_d, uint64_t seed) {
    PSVO_REQUIRE(e && d && rays_o && rays_d && n_rays > 0, "map_query: bad arguments");
    e->images_next = false;  // the weights may change before the next step
    PSVO_REQUIRE(e->q_count < 2, "map_query: two queries already queued (run psvo_map_step)");
    hipStream_t st = as_stream(stream);
    if (!e->side) {
        if (hipStreamCreateWithFlags(&e->side, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&e->in_ready, hipEventDisableTiming) != hipSuccess)
            return set_error(PSVO_E_LAUNCH, "map_query: side stream creation failed");
    }
    QuerySet &q = e->qs[(e->q_head + e->q_count) & 1];
    // the rays were produced on the caller's stream; the set's buffers may
    // still be read by the step that consumed it last
    ENG_CALL(ev_record(e->in_ready, st, "map_query"));
    ENG_CALL(st_wait(e->side, e->in_ready, "map_query"));
    ENG_CALL(freed_wait(q, e->side));
    // (a buffer that must grow syncs the side stream first, which includes that wait)
    ENG_CALL(query_enqueue(e, e->side, q, d, n_rays, rays_o, rays_d, seed, "map_query"));
    q.pending = true;
    e->q_count++;
    return PSVO_OK;
}
