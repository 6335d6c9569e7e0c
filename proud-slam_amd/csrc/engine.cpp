// Native mapping-iteration engine: one C call runs a whole render-and-optimise
// iteration of the mapping loop (render_helpers.py:609-672 — render_rays,
// Criterion, loss.backward(), Adam(embeddings).step(), Adam(decoder).step())
// on one HIP stream: 24 kernel launches, two 32-byte stats read-backs that
// size the sample buffers, no host allocation after warm-up.  It strings
// together the same C-ABI entry points the PyTorch autograd path calls, so
// the two paths compute the same numbers; what it removes is the Python /
// autograd / allocator time between launches, which otherwise leaves the GPU
// idle behind every read-back.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <utility>

#include "engine_internal.h"

// what render.hip needs of the engine (its struct is engine_internal.h's)
namespace psvo {
RenderWs *&engine_render_ws(psvo_engine *e) { return e->render; }
bool engine_data_parallel(const psvo_engine *e) { return e->x.on(); }
}  // namespace psvo

using namespace psvo;
using namespace psvo::eng;

namespace psvo {
thread_local KernelClock *g_kclock = nullptr;

namespace eng {

// device buffer of at least `bytes` for `slot`; growing synchronises the
// stream first (the old buffer may still be read by queued kernels)
void *arena_buf(Arena &a, hipStream_t st, int slot, size_t bytes, int *rc) {
    if (bytes == 0) bytes = 16;
    if (a.cap[slot] >= bytes) return a.p[slot];
    if (a.p[slot]) {
        (void)hipStreamSynchronize(st);
        (void)hipFree(a.p[slot]);
        a.p[slot] = nullptr;
        a.cap[slot] = 0;
    }
    const size_t cap = bytes + bytes / 4;  // headroom against per-step size jitter
    if (hipMalloc(&a.p[slot], cap) != hipSuccess) {
        *rc = set_error(PSVO_E_LAUNCH, "engine: hipMalloc(%zu) failed", cap);
        return nullptr;
    }
    a.cap[slot] = cap;
    a.gen[slot]++;
    return a.p[slot];
}

// block = false: only the pairs whose kernels have finished (a timed step's
// host must not wait for kernels it queued ahead); the rest move to the front
void timer_collect(psvo_engine *e, bool block) {
    EngineTimer &t = e->tm;
    if (!t.markers) {  // kernel-bound
        psvo::KernelClock &c = t.kc;
        auto ready = [&](hipEvent_t ev) {
            const hipError_t q = block ? hipEventSynchronize(ev) : hipEventQuery(ev);
            if (q == hipErrorNotReady && hipPeekAtLastError() == hipErrorNotReady) (void)hipGetLastError();  // not an error
            return q;
        };
        if (c.sum) {
            int w = 0;
            for (int i = 0; i < c.n; ++i) {
                const hipError_t q = ready(c.ev[i][1]);
                if (q == hipErrorNotReady) {
                    if (w != i) {
                        std::swap(c.ev[w][0], c.ev[i][0]);
                        std::swap(c.ev[w][1], c.ev[i][1]);
                        c.region[w] = c.region[i];
                    }
                    ++w;
                    continue;
                }
                float ms = 0.f;
                if (q == hipSuccess && hipEventElapsedTime(&ms, c.ev[i][0], c.ev[i][1]) == hipSuccess)
                    t.kms[c.region[i]] += ms;
                else
                    (void)hipGetLastError();  // not the next launch's error
            }
            c.n = w;
        } else {
            // closed instances in queue order; an unfinished one ends this pass
            // (its pairs and the later ones' stay until a later collection)
            int done = 0;
            for (; done < c.n_inst; ++done) {
                const psvo::KernelClock::Inst &I = c.inst[done];
                bool open = false;
                for (int d = 0; d < c.depth; ++d) open |= c.stack[d] == done;
                if (open) break;
                if (I.first < 0) continue;  // no kernel: the region's instance counts 0
                const hipError_t q = ready(c.ev[I.last][1]);
                if (q == hipErrorNotReady) break;
                float ms = 0.f;
                if (q == hipSuccess && hipEventElapsedTime(&ms, c.ev[I.first][0], c.ev[I.last][1]) == hipSuccess)
                    t.kms[I.region] += ms;
                else
                    (void)hipGetLastError();
            }
            if (done > 0) {  // drop the collected instances (the open ones keep their stack slots)
                for (int k = done; k < c.n_inst; ++k) c.inst[k - done] = c.inst[k];
                c.n_inst -= done;
                for (int d = 0; d < c.depth; ++d) c.stack[d] -= done;
            }
            if (c.n_inst == 0) c.n = 0;  // every pair read: the slots start over
        }
        t.pending = false;
        return;
    }
    if (!t.pending) return;
    for (int r = 0; r < PSVO_TIME_REGIONS; ++r) {
        if (!(t.used & (1u << r))) continue;  // never recorded: reading it would leave a sticky HIP error
        float ms = 0.f;
        if (hipEventSynchronize(t.ev[r][1]) == hipSuccess && hipEventElapsedTime(&ms, t.ev[r][0], t.ev[r][1]) == hipSuccess) {
            t.ms[r] += ms;
            t.n[r] += 1;
        } else {
            (void)hipGetLastError();  // not the next launch's error
        }
    }
    t.used = 0;
    t.pending = false;
}

void mark(psvo_engine *e, hipStream_t st, int region, int end) {
    EngineTimer &t = e->tm;
    if (!t.on) return;
    if (t.markers) {
        (void)hipEventRecord(t.ev[region][end], st);
        if (end) t.used |= 1u << region;
        return;
    }
    psvo::KernelClock &c = t.kc;
    if (!end) {
        if (c.n + 32 > psvo::KernelClock::kMax || c.n_inst + 2 > psvo::KernelClock::kMaxInst)
            timer_collect(e, true);  // room for the region's kernels
        t.starts[region] += 1;
        psvo::g_kclock = &c;
        c.streams[0] = st;  // the region's stream and the engine's side streams
        c.streams[1] = e->aux;
        c.streams[2] = e->lossq;
        c.streams[3] = e->side;
        if (c.depth >= 8) {
            c.overflow = true;
            return;
        }
        if (c.sum) {
            c.stack[c.depth++] = region;
        } else if (c.n_inst < psvo::KernelClock::kMaxInst) {
            c.inst[c.n_inst] = psvo::KernelClock::Inst{region, -1, -1};
            c.stack[c.depth++] = c.n_inst++;
        } else {
            c.overflow = true;
        }
    } else if (c.depth > 0) {
        c.depth--;
    }
}

// st waits for a split tail's optimiser step (step_tail) if one is pending.
// host_wait_us > 0: first poll the event from the host for up to that long
// (the device-sized forward is queued while the query still runs: a host
// that waits for the optimiser here keeps the cross-queue barrier — ≈ 20 µs
// of idle GPU between the sampler and the interpolation, measured — out of
// the stream)
int join_adam(psvo_engine *e, hipStream_t st, const char *who, double host_wait_us) {
    if (!e->adam_pending) return PSVO_OK;
    // already done (the usual case: the optimiser step ran beside the query):
    // no barrier packet in front of the interpolation — the command processor
    // resolves even a satisfied cross-queue wait with a few µs of latency
    hipError_t q = hipEventQuery(e->adam_done);
    if (q == hipErrorNotReady && host_wait_us > 0.0) {
        const double t_end = now_ns() + host_wait_us * 1e3;
        while (q == hipErrorNotReady && now_ns() < t_end) q = hipEventQuery(e->adam_done);
    }
    if (q == hipSuccess) {
        e->adam_pending = false;
        return PSVO_OK;
    }
    if (q == hipErrorNotReady && hipPeekAtLastError() == hipErrorNotReady) (void)hipGetLastError();  // not an error
    ENG_CALL(st_wait(st, e->adam_done, who));
    e->adam_pending = false;
    return PSVO_OK;
}

int ensure_aux(psvo_engine *e) {
    if (e->aux) return PSVO_OK;
    hipEvent_t *evs[] = {&e->dfeat_ready, &e->emb_done, &e->z_ready, &e->coef_ready, &e->grads_ready,
                         &e->prep_fork, &e->prep_done, &e->loss_done, &e->adam_done, &e->next_ready};
    if (hipStreamCreateWithFlags(&e->aux, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&e->lossq, hipStreamNonBlocking) != hipSuccess)
        return set_error(PSVO_E_LAUNCH, "engine: aux stream creation failed");
    // stream-ordering events on one device: no system-scope fence (its L2
    // write-back, ≈ dirty bytes ÷ 6 TB/s, would sit between the kernels)
    for (hipEvent_t *ev : evs)  // (dfeat_ready may be bound to a dispatch as its stop event, like q.p1)
        if (hipEventCreateWithFlags(ev, (ev == &e->dfeat_ready ? 0 : hipEventDisableTiming) |
                                            hipEventDisableSystemFence) != hipSuccess)
            return set_error(PSVO_E_LAUNCH, "engine: event creation failed");
    return PSVO_OK;
}

// decoder parameter sizes (nrgbd.py:98-108, depth 2, in 16, sdf_dim 128) for width W
void dec_sizes(int W, int64_t (&n)[10]) {
    const int64_t w = W;
    const int64_t v[10] = {w * 16, w, w * w, w, 129 * w, 129, w * 144, w, 3 * w, 3};
    for (int i = 0; i < 10; ++i) n[i] = v[i];
}

// grads: [embeddings (n_emb x 16) | W1, b1, ..., W5, b5]
// one launch for both optimisers (lr per tensor); the embedding gradient is
// zeroed as it is consumed — the next iteration's atomics accumulate into it
int map_adam(hipStream_t st, const psvo_map_desc *d, float *grads, int64_t adam_step, const PoseAdam *pa,
             bool sparse_rows) {
    constexpr int kMax = 11 + kXchMaxFrames;
    float *p[kMax];
    const float *g[kMax];
    float *m[kMax], *v[kMax];
    int64_t n[kMax], steps[kMax];
    double lr[kMax];
    int zero[kMax];
    const uint8_t *rows[kMax] = {};
    if (sparse_rows) rows[0] = d->emb_row_flags;  // the embedding table: flagged rows only
    p[0] = d->emb;
    g[0] = grads;
    m[0] = d->emb_m;
    v[0] = d->emb_v;
    n[0] = d->n_emb * 16;
    lr[0] = d->lr_emb;
    zero[0] = 1;
    int64_t off = d->n_emb * 16;
    int64_t kDecSizes[10];
    dec_sizes(d->width, kDecSizes);
    for (int i = 0; i < 10; ++i) {
        p[1 + i] = d->dec[i];
        g[1 + i] = grads + off;
        m[1 + i] = d->dec_m[i];
        v[1 + i] = d->dec_v[i];
        n[1 + i] = kDecSizes[i];
        lr[1 + i] = d->lr_dec;
        zero[1 + i] = 0;  // overwritten by the decoder backward
        off += kDecSizes[i];
    }
    int cnt = 11;
    for (int i = 0; i < cnt; ++i) steps[i] = adam_step;
    for (int f = 0; pa && f < pa->n; ++f, ++cnt) {
        p[cnt] = pa->p[f];
        g[cnt] = pa->g[f];
        m[cnt] = pa->m[f];
        v[cnt] = pa->v[f];
        n[cnt] = 6;
        lr[cnt] = pa->lr;
        zero[cnt] = 0;
        steps[cnt] = pa->step[f];
    }
    return adam_launch(st, cnt, p, g, m, v, n, lr, d->beta1, d->beta2, d->eps, 0.0, adam_step, zero, steps, rows);
}

// the poses' Adam steps on their own (one launch, each pose at its own step)
int pose_adam(hipStream_t st, const psvo_map_desc *d, const PoseAdam &pa) {
    if (pa.n == 0) return PSVO_OK;
    int64_t n6[kXchMaxFrames];
    double lr[kXchMaxFrames];
    int zero[kXchMaxFrames];
    for (int k = 0; k < pa.n; ++k) {
        n6[k] = 6;
        lr[k] = pa.lr;
        zero[k] = 0;
    }
    return adam_launch(st, pa.n, pa.p, pa.g, pa.m, pa.v, n6, lr, d->beta1, d->beta2, d->eps, 0.0, 1, zero,
                       const_cast<int64_t *>(pa.step));
}

}  // namespace eng
}  // namespace psvo

extern "C" psvo_engine *psvo_engine_new(void) {
    psvo_engine *e = new psvo_engine();
    // PSVO_INTERP_PASS=1: engines start with the separate interpolation pass
    // (psvo_engine_set_paths replaces the whole mask)
    const char *ipass = getenv("PSVO_INTERP_PASS");
    if (ipass && ipass[0] == '1') e->paths |= PSVO_PATH_INTERP_PASS;
    // PSVO_BWD_TWO_LAUNCH=1: likewise the two-launch decoder backward
    const char *two = getenv("PSVO_BWD_TWO_LAUNCH");
    if (two && two[0] == '1') e->paths |= PSVO_PATH_BWD_TWO_LAUNCH;
    for (auto &q : e->qs)
        if (query_set_init(q) != PSVO_OK) {
            psvo_engine_free(e);
            return nullptr;
        }
    return e;
}

static EngineExchange exchange_layout(int world, int64_t max_rays_global, int64_t max_rays_rank) {
    EngineExchange x;
    x.world = world;
    x.nch = dist_slot0_rows(max_rays_global) / kSamplerG;
    x.max_rays_rank = max_rays_rank > 0 ? max_rays_rank : max_rays_global;
    x.cw = dist_count_words((int)x.max_rays_rank);
    return x;
}

extern "C" int64_t psvo_engine_exchange_words(int world, int64_t max_rays_global, int64_t max_rays_rank) {
    if (world < 1 || max_rays_global < 1 || max_rays_rank < 0 || max_rays_rank > max_rays_global) return -1;
    const EngineExchange x = exchange_layout(world, max_rays_global, max_rays_rank);
    return x.table_off() + x.table_words();
}

extern "C" int psvo_engine_set_exchange(psvo_engine *e, int rank, int world, int64_t max_rays_global,
                                        int64_t max_rays_rank, psvo_exchange_fn fn, void *user, int *xi32,
                                        double *xf64) {
    PSVO_REQUIRE(e, "engine_set_exchange: null engine");
    PSVO_REQUIRE(world >= 1 && rank >= 0 && rank < world && max_rays_global >= 1 && max_rays_rank >= 0 &&
                     max_rays_rank <= max_rays_global,
                 "engine_set_exchange: bad rank %d / world %d / max_rays_global %lld / max_rays_rank %lld", rank,
                 world, (long long)max_rays_global, (long long)max_rays_rank);
    PSVO_REQUIRE(e->q_count == 0, "engine_set_exchange: queries are queued");
    PSVO_REQUIRE(!fn || (xi32 && xf64), "engine_set_exchange: exchange buffers required");
    e->x = exchange_layout(world, max_rays_global, max_rays_rank);
    e->x.fn = fn;
    e->x.user = user;
    e->x.rank = rank;
    e->x.xi32 = xi32;
    e->x.xf64 = xf64;
    return PSVO_OK;
}

extern "C" int psvo_engine_set_paths(psvo_engine *e, int paths) {
    PSVO_REQUIRE(e && (paths & ~(PSVO_PATH_QUERY_SPLIT | PSVO_PATH_PADDED | PSVO_PATH_DENSE_DECODER |
                               PSVO_PATH_INTERP_PASS | PSVO_PATH_BWD_TWO_LAUNCH)) == 0,
                 "engine_set_paths: bad arguments");
    PSVO_REQUIRE(e->q_count == 0, "engine_set_paths: queries are queued");
    e->paths = paths;
    return PSVO_OK;
}

extern "C" int psvo_engine_gate_stream(psvo_engine *e, void *stream) {
    PSVO_REQUIRE(e, "engine_gate_stream: null engine");
    e->draw_gate_used = true;  // (binding the event costs the selection's stream ≈ 5 µs: only for a gating caller)
    if (!e->draw_gate_recorded) return PSVO_OK;
    return st_wait(as_stream(stream), e->draw_gate_ev, "engine_gate_stream");
}

extern "C" int psvo_engine_select_stats(psvo_engine *e, void *stream, int64_t *out, int reset) {
    PSVO_REQUIRE(e && out, "engine_select_stats: null argument");
    for (int i = 0; i < 5; ++i) out[i] = 0;
    if (!e->a.p[kSelCnt]) return PSVO_OK;  // no sparse step yet
    hipStream_t st = as_stream(stream);
    int c[psvo::kSelCountInts];
    if (hipMemcpyAsync(c, e->a.p[kSelCnt], sizeof(c), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return set_error(PSVO_E_LAUNCH, "engine_select_stats: copy failed");
    unsigned long long u[3];
    memcpy(u, c + 4, sizeof(u));
    out[0] = (int64_t)c[0] + c[1];  // kept: class A + class B
    out[1] = c[3];                  // composited
    out[2] = (int64_t)u[0];
    out[3] = (int64_t)u[1];
    out[4] = (int64_t)u[2];
    if (c[2] & psvo::kLbFlagTimeout) {  // reported once: the bit and the host word cleared
        ENG_CALL(zero_async(static_cast<int *>(e->a.p[kSelCnt]) + 2, sizeof(int), st, "engine_select_stats"));
        if (e->host_flags) *(volatile int *)e->host_flags = 0;
        e->sel_zero_gen = 0;
        return set_error(PSVO_E_LAUNCH, "engine_select_stats: a sample selection's look-back wait was abandoned");
    }
    if (reset)
        ENG_CALL(zero_async(static_cast<int *>(e->a.p[kSelCnt]) + 4, 6 * sizeof(int), st, "engine_select_stats"));
    return PSVO_OK;
}

extern "C" int psvo_engine_set_timing(psvo_engine *e, int on) {
    PSVO_REQUIRE(e, "engine_set_timing: null engine");
    EngineTimer &t = e->tm;
    const char *mk = getenv("PSVO_TIMING_MARKERS");
    if (on && !t.ev[0][0])
        for (int r = 0; r < PSVO_TIME_REGIONS; ++r)
            for (int k = 0; k < 2; ++k)
                // a device-scope release: a marker with the default system-scope one
                // writes the L2 back between the kernels it brackets (measured in the time)
                if (hipEventCreateWithFlags(&t.ev[r][k], hipEventReleaseToDevice) != hipSuccess)
                    return set_error(PSVO_E_LAUNCH, "engine_set_timing: hipEventCreate failed");
    // the kernel-bound pairs: device-scope release too — the stop event is
    // the kernel's own completion signal, and a system-scope release there
    // adds an L2 write-back to the span that the untimed kernel does not pay
    const unsigned kc_flags = hipEventReleaseToDevice;
    if (on && !t.kc.ev[0][0])
        for (int i = 0; i < psvo::KernelClock::kMax; ++i)
            for (int k = 0; k < 2; ++k)
                if (hipEventCreateWithFlags(&t.kc.ev[i][k], kc_flags) != hipSuccess)
                    return set_error(PSVO_E_LAUNCH, "engine_set_timing: hipEventCreate failed");
    timer_collect(e, true);
    if (psvo::g_kclock == &t.kc) psvo::g_kclock = nullptr;
    t.kc.depth = 0;
    t.kc.overflow = false;
    t.on = on != 0;
    t.overlap = on == 2;
    t.markers = mk && *mk == '1';
    const char *ks = getenv("PSVO_TIMING_SPAN");
    t.kc.sum = !(ks && *ks == '1');
    t.kc.n = 0;
    t.kc.n_inst = 0;
    for (int r = 0; r < PSVO_TIME_REGIONS; ++r) {
        t.ms[r] = 0.0;
        t.n[r] = 0;
        t.kms[r] = 0.0;
        t.starts[r] = 0;
    }
    return PSVO_OK;
}

extern "C" int psvo_engine_timing(psvo_engine *e, double *mean_ms) {
    PSVO_REQUIRE(e && mean_ms, "engine_timing: null argument");
    EngineTimer &t = e->tm;
    timer_collect(e, true);
    for (int r = 0; r < PSVO_TIME_REGIONS; ++r) {
        if (t.markers)
            mean_ms[r] = t.n[r] ? t.ms[r] / (double)t.n[r] : -1.0;
        else  // a region whose instances launched no kernel reads 0 (e.g. no separate compaction)
            mean_ms[r] = t.starts[r] ? t.kms[r] / (double)t.starts[r] : -1.0;
    }
    PSVO_REQUIRE(t.markers || !t.kc.overflow, "engine_timing: more kernels per step than timing slots");
    return PSVO_OK;
}

extern "C" int psvo_engine_set_clock(psvo_engine *e, int max_steps) {
    PSVO_REQUIRE(e && max_steps >= 0, "engine_set_clock: bad arguments");
    while ((int)e->clk.ev.size() < max_steps) {
        hipEvent_t ev;
        // device-scope release: the clock's marker sits between the query's scan
        // and the compaction on the critical stream (a system-scope one costs
        // an L2 write-back there)
        if (hipEventCreateWithFlags(&ev, hipEventReleaseToDevice) != hipSuccess)
            return set_error(PSVO_E_LAUNCH, "engine_set_clock: event failed");
        e->clk.ev.push_back(ev);
    }
    e->clk.n = 0;
    e->clk.on = max_steps > 0;
    return PSVO_OK;
}

extern "C" int psvo_engine_clock(psvo_engine *e, double *period_ms, int *n_steps) {
    PSVO_REQUIRE(e && period_ms && n_steps, "engine_clock: null argument");
    *period_ms = -1.0;
    *n_steps = e->clk.n;
    if (e->clk.n >= 2) {
        float ms = 0.f;
        hipEvent_t a = e->clk.ev[0], b = e->clk.ev[e->clk.n - 1];
        if (hipEventSynchronize(b) != hipSuccess || hipEventElapsedTime(&ms, a, b) != hipSuccess)
            return set_error(PSVO_E_LAUNCH, "engine_clock: event read failed");
        *period_ms = ms / (double)(e->clk.n - 1);
    }
    return PSVO_OK;
}

extern "C" void psvo_engine_free(psvo_engine *e) {
    if (!e) return;
    for (hipEvent_t ev : e->clk.ev) (void)hipEventDestroy(ev);
    host_wait_report();
    (void)hipDeviceSynchronize();
    for (int r = 0; r < PSVO_TIME_REGIONS; ++r)
        for (int k = 0; k < 2; ++k)
            if (e->tm.ev[r][k]) (void)hipEventDestroy(e->tm.ev[r][k]);
    if (psvo::g_kclock == &e->tm.kc) psvo::g_kclock = nullptr;
    for (int i = 0; i < psvo::KernelClock::kMax; ++i)
        for (int k = 0; k < 2; ++k)
            if (e->tm.kc.ev[i][k]) (void)hipEventDestroy(e->tm.kc.ev[i][k]);
    for (int s = 0; s < kSlots; ++s)
        if (e->a.p[s]) (void)hipFree(e->a.p[s]);
    for (auto &q : e->qs) query_set_free(q);
    if (e->side) (void)hipStreamDestroy(e->side);
    if (e->q2s) (void)hipStreamDestroy(e->q2s);
    if (e->aux) {
        (void)hipStreamSynchronize(e->aux);  // a pending tail split's optimiser step
        (void)hipStreamDestroy(e->aux);
    }
    if (e->lossq) (void)hipStreamDestroy(e->lossq);
    if (e->loss_done) (void)hipEventDestroy(e->loss_done);
    if (e->dfeat_ready) (void)hipEventDestroy(e->dfeat_ready);
    if (e->emb_done) (void)hipEventDestroy(e->emb_done);
    if (e->z_ready) (void)hipEventDestroy(e->z_ready);
    if (e->coef_ready) (void)hipEventDestroy(e->coef_ready);
    if (e->grads_ready) (void)hipEventDestroy(e->grads_ready);
    if (e->prep_fork) (void)hipEventDestroy(e->prep_fork);
    if (e->prep_done) (void)hipEventDestroy(e->prep_done);
    if (e->adam_done) (void)hipEventDestroy(e->adam_done);
    if (e->next_ready) (void)hipEventDestroy(e->next_ready);
    if (e->in_ready) (void)hipEventDestroy(e->in_ready);
    if (e->draw_gate) (void)hipEventDestroy(e->draw_gate);
    if (e->host_flags) (void)hipHostFree(e->host_flags);
    psvo::render_ws_free(e->render);
    delete e;
}

static int64_t dec_total(int W) {
    int64_t n[10], t = 0;
    dec_sizes(W, n);
    for (int i = 0; i < 10; ++i) t += n[i];
    return t;
}

extern "C" int64_t psvo_map_grad_floats(int64_t n_emb) { return n_emb * 16 + dec_total(128); }
extern "C" int64_t psvo_map_grad_floats_w(int64_t n_emb, int width) { return n_emb * 16 + dec_total(width); }

extern "C" int psvo_map_adam_ex(psvo_engine *e, void *stream, const psvo_map_desc *d, int64_t adam_step,
                                int flags) {
    PSVO_REQUIRE(e && d && d->grad_flat && adam_step >= 1, "map_adam: needs desc->grad_flat and adam_step >= 1");
    e->images_next = false;  // the weights may change before the next step
    hipStream_t st = as_stream(stream);
    ENG_CALL(join_adam(e, st, "map_adam"));
    // sparse-exact when the row flags hold every row with a gradient: a
    // single-GPU step marked its rows itself (also under PSVO_STEP_NO_ADAM);
    // data parallel, only the gradient exchange knows the union of all ranks'
    // rows, so the caller says it marked them (PSVO_ADAM_ROWS_EXCHANGED)
    const bool flags_complete = !e->x.on() || (flags & PSVO_ADAM_ROWS_EXCHANGED);
    const bool sparse = d->emb_row_flags != nullptr && flags_complete;
    ENG_CALL(map_adam(st, d, d->grad_flat, adam_step, nullptr, sparse));
    if (d->emb_row_flags && !sparse) {
        // dense step under the exchange without a union mark (one unforced
        // rank, a caller's own all-reduce): keep the flags sticky-complete —
        // every row whose moments are now non-zero — so a later sparse step
        // still steps them; this rank's marks are spent
        ENG_CALL(psvo_adam_flags_from_state(st, d->n_emb, d->emb_m, d->emb_v, d->emb_row_flags));
        if (d->emb_row_local) ENG_CALL(zero_async(d->emb_row_local, (size_t)d->n_emb, st, "map_adam"));
    }
    e->grads_clean = true;
    return PSVO_OK;
}

extern "C" int psvo_map_adam(psvo_engine *e, void *stream, const psvo_map_desc *d, int64_t adam_step) {
    return psvo_map_adam_ex(e, stream, d, adam_step, 0);
}

extern "C" int psvo_map_side_wait(psvo_engine *e, void *stream) {
    PSVO_REQUIRE(e, "map_side_wait: null engine");
    if (!e->dfeat_ready || !e->bwd_recorded) return PSVO_OK;
    return st_wait(as_stream(stream), e->dfeat_ready, "map_side_wait");
}

extern "C" int psvo_map_join(psvo_engine *e, void *stream) {
    PSVO_REQUIRE(e, "map_join: null engine");
    return join_adam(e, as_stream(stream), "map_join");
}
