// The ray-query stage as its callers see it (query_trace.hip: traversal and
// statistics / rank pass; query_sample.hip: sampler, scan and compaction;
// query_dist.hip: the data-parallel union layout): the engine, the renderer,
// the Criterion's count kernels and the debug entry points.
#pragma once

#include "psvo_common.h"
#include "lookback.h"

namespace psvo {

// The bits of a query's PSVO_STAT_FLAGS word (the engine turns the first
// four into errors at the read-back):
constexpr int kStatFlagDfsOverflow = 1;      // the octree is deeper than the traversal's DFS stack
constexpr int kStatFlagSamplerOverflow = 2;  // a ray needs more than the sampler rows' max_steps
constexpr int kStatFlagUnionOverflow = 4;    // data parallel: the union batch exceeds max_rays_global
constexpr int kLbFlagTimeout = 8;            // a look-back wait was abandoned (lookback.h's bug trap)
// set by k_dist_smax when some rank did not count: every rank then counts in
// its step (one decision for all ranks, so all issue the same collectives)
constexpr int PSVO_FLAG_UNION_UNCOUNTED = 16;

// the query's statistics words → coherent pinned host memory as {seq, value}
// granules (stat_to_host; zeroing them on the device): the engine's host
// thread polls the tags instead of waiting for an event (query_trace.hip)
// zero: clear the words read (the query set's next use needs no memset);
// false for a first read-back that later kernels of the query still extend
int stats_to_host(hipStream_t st, int *stats, unsigned long long *host, int words, int seq, bool zero = true);
// The Criterion's normalisers (criterion.py:70-101: the valid-depth rays and
// the front / sdf samples over the padded [R_hit, S_max] layout) depend only
// on the samples' depths and the rays' GT depth, so the sampler counts them
// per ray as it emits samples (ray_cnt i32[R]) and its last workgroup turns
// the sums into the backward coefficients coef f32[4] (crit_coef_from_counts:
// k_crit_coef's bits).  gt_depth null: not counted.
struct SampleCounts {
    const float *gt_depth;
    int *ray_cnt;
    float *coef;
    float tr, max_depth, w_rgb, w_depth, w_fs, w_sdf;
    int crit_flags;
};
// psvo_sample_rays (single GPU, whole batch) whose scan also does
// stats_to_host's read-back (query_sample.hip); with counts also the
// normalisers.  lb_desc (query_lookback): the scan runs inside the sampler
// launch by look-back (lookback.h) over the descriptors after the
// traversal's (lookback_granules(r_hit_cap) granules, tag ≠ 0 fresh per
// query), the rows hold only their valid prefix, and with leaf / t / ray_of
// (capacity r_hit_cap · max_steps_cap) the launch also does k_compact_rays'
// compaction
int sample_rays_to_host(hipStream_t st, int64_t r_hit_cap, int max_steps_cap, const int *rank_ray, const int *hit_idx,
                        const float *hit_t0, const float *hit_t1, const float *ray_dsum, float step_size,
                        const float *noise, uint64_t seed, int *stats, int *s_idx, float *s_depth, float *s_dist,
                        int *ray_ns, int *offsets, unsigned long long *host, int seq,
                        const SampleCounts *counts = nullptr, unsigned long long *lb_desc = nullptr,
                        uint32_t lb_tag = 0, int *leaf = nullptr, float *t = nullptr, int *ray_of = nullptr,
                        int *m_out = nullptr,  // with the compaction: M on the device
                        const int *nv_rank = nullptr, const int *col0_rank = nullptr);  // intersect_ranked's copies
// whether a query of r rays runs its statistics / rank pass and its sample
// scan by look-back (up to kLbMaxRays rays), and its descriptor granules
constexpr int kIsWaves = 8;   // k_intersect_sorted: waves (rays) per workgroup
constexpr int kSmpWaves = 8;  // k_sample_fused: waves (rays) per workgroup
constexpr int64_t kLbMaxRays = 16384;  // 8 rays per workgroup: 2,048 workgroups, within lookback.h's 64 · 64
constexpr int kLbIsGranules = 5, kLbSmpGranules = 8;
// statistics words [kStatQuery, +3): the traversal's P / R_hit / max ⌈steps⌉
// again, for the look-back sampler — never zeroed by a read-back, so a
// sampler workgroup that starts after the launch's last one zeroed words
// [0, kStatQuery) still reads this batch's values (lookback.h helping)
constexpr int kStatQuery = 13;
static_assert(kStatQuery + 3 <= PSVO_STAT_WORDS, "statistics words");
// The statistics / rank pass and the sample scan: by default inside the
// traversal and sampler launches by decoupled look-back (lookback.h; up to
// kLbMaxRays rays: the packed pf / psm count granule); beyond that, and on
// the data-parallel sampler, as kernels of their own (k_ray_stats_rank,
// k_scan_samples).  The
// round-3 in-launch variant — the launch's last-arriving workgroup re-reading
// every ray — measured slower than the split kernels (one workgroup's
// dependent sc1 round trips) and is gone.
inline bool query_lookback(int64_t r) { return r > 0 && r <= kLbMaxRays; }
// (the sampler's descriptors lie after the traversal's: sample_rays_to_host)
inline int64_t lookback_granules(int64_t r) {
    return lb_granules<kLbIsGranules>(div_up(r, kIsWaves)) + lb_granules<kLbSmpGranules>(div_up(r, kSmpWaves));
}

// psvo_ray_intersect_sorted + psvo_hit_rank with the two single-block
// reductions fused into one launch (query_trace.hip)
int intersect_ranked(hipStream_t st, int64_t n_rays, const float *rays_o, const float *rays_d, const float *centres,
                     const int *structure, float voxel_size, float max_distance, float step_size, int *hit_idx,
                     float *hit_t0, float *hit_t1, int *ray_nv, float *ray_dsum, int *stats, int *ray_rank,
                     int *rank_ray, const PackRec *packed = nullptr, int *blk_out = nullptr,
                     unsigned long long *lb_desc = nullptr, uint32_t lb_tag = 0,
                     int *nv_rank = nullptr, int *col0_rank = nullptr, int64_t n_nodes = 0);  // look-back: by-rank hit count, first id

// look-back blocks helped (lookback.h) by the traversal and by the sampler:
// one counter per translation unit (psvo_debug_lb_helps)
int lb_helps_trace(int64_t *out1, bool reset);
int lb_helps_sample(int64_t *out1, bool reset);

// data-parallel query (query_dist.hip): rows of the slot-0 count table for a
// union batch of at most max_rays_global rays; the words one rank
// contributes to the query's first all-gather (8 words + a hit-count byte per
// hit row, for at most max_rays_rank rays); pack them; union statistics +
// slot-0 count table from the gathered words; the sampler over the rank's
// rows (query_sample.hip); after the second all-gather ([S_max, 7 count
// words] per rank) the union S_max and normaliser sums.
// One number by design: the first gather's header words per rank (R_hit, P,
// max ceil, first voxel id of its first hit row, flags; the rest 0) and the
// second gather's words per rank
constexpr int kDistWordsPerRank = 8;
// word 0 of a rank's second-gather words: its S_max, with this bit set when
// it did not count its rows (no GT depths given to its query)
constexpr int kDistNotCounted = 1 << 30;
int dist_slot0_rows(int64_t max_rays_global);
int dist_count_words(int max_rays_rank);
int dist_pack(hipStream_t st, int64_t R, const int *stats, const int *rank_ray, const int *hit_idx,
              const int *ray_nv, int *out, const int *nv_rank = nullptr, int flags_or = 0);
// (q2_in: this rank's words of the second gather, whose count words it
// zeroes, or null: the caller zeroes them on the stream of dist_counts)
int dist_layout(hipStream_t st, const int *all, int world, int rank, int stride, int nch, int *stats, int *table,
                int *q2_in);
int dist_sample(hipStream_t st, int64_t r_hit_cap, int max_steps_cap, const int *rank_ray, const int *hit_idx,
                const float *hit_t0, const float *hit_t1, const float *ray_dsum, float step_size, uint64_t seed,
                int *stats, const int *table, int nch, int *s_idx, float *s_depth, float *s_dist, int *ray_ns,
                int *offsets, const int *nv_rank = nullptr, const int *col0_rank = nullptr);
int dist_smax(hipStream_t st, const int *all, int world, int *stats, int *in, double *sums);
// this rank's words of the second gather: in[0] = S_max of its rows; given
// the GT depths, in[1..7] += n_valid, Σ front / Σ sdf-band over the valid
// samples, and per padding class (front, band: sample_terms of the MAX_DEPTH
// fill) the rays and their Σ ns — in[1..7] zeroed before (criterion.hip)
int dist_counts(hipStream_t st, int64_t R, const int *stats, const int *rank_ray, const float *gt_depth,
                const float *z_rows, int z_stride, const int *ray_ns, float truncation, float max_depth, int *in);

// sample compaction alone, one wave per hit ray (query_sample.hip k_compact_rays):
// the valid prefix of each sampler row → leaf / t / ray_of_sample at offsets[r] + s
int compact_rays(hipStream_t st, int64_t r_hit, int cap, const int *s_idx, const float *s_depth, const int *offsets,
                 int *leaf, float *t, int *ray_of_sample);

}  // namespace psvo
