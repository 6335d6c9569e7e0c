// Ray / sparse-voxel-octree query on gfx950, second half: inverse-CDF
// sampling of the hit rays, the scan of their sample counts and the sample
// compaction.  (query_trace.hip: the traversal whose hit rows these read.)
//
// Reference behaviour restated (DARYL-GWZ/Proud-SLAM):
//   voxel_helpers.py:288-374  sampler host wrapper: G = 200 blocks × K' slots, 800-slot chunks
//   sample_gpu.cu:133-239     inverse-CDF kernel incl. its layout-dependent trailing segment
//   voxel_helpers.py:637-663  probs / steps, clamp + MAX_DEPTH fill
//   render_helpers.py:390-460 ray and sample compaction
//
// MI355X design: one wave per ray in the fused sampler (lane b owns bin b);
// the per-launch statistics (S_max, M) and the Criterion's normalisers are
// reduced inside the launch, so the host reads them back once instead of
// the reference's sequence of host syncs.
//
// Arithmetic: the sampler is compiled with FP contraction off and IEEE
// division so sample depths reproduce the CPU oracle bit for bit (the
// reference CUDA uses __fdividef and nvcc's default FMA contraction; see
// DESIGN.md "parity").
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include "query.h"
#include "query_common.h"

namespace psvo {
namespace {

// ---------------------------------------------------------------------------
// Sampler core shared by the drop-in launch and the fused path.  `Rows`
// abstracts where row elements come from: the drop-in kernel indexes a
// contiguous chunk exactly like the reference; the fused kernel maps the
// reference's logical [200, K', P] layout onto the compacted hit rays.
struct RawRows {
    const int *pts_idx;
    const float *min_depth, *max_depth, *probs;
    int H;
    __device__ int idx_at(int elem_from_H) const { return pts_idx[H + elem_from_H]; }
    __device__ int idx_slot0(int col) const { return pts_idx[col]; }
    __device__ float lo_at(int e) const { return min_depth[H + e]; }
    __device__ float hi_at(int e) const { return max_depth[H + e]; }
    __device__ float prob_at(int e) const { return probs[H + e]; }
    // bins of the ray's own row (e < max_hits)
    __device__ int own_idx(int e) const { return idx_at(e); }
    __device__ float own_lo(int e) const { return lo_at(e); }
    __device__ float own_hi(int e) const { return hi_at(e); }
    __device__ float own_prob(int e) const { return prob_at(e); }
};

struct FusedRows {
    const int *rank_ray;
    const int *hit_idx;
    const float *hit_t0, *hit_t1, *dsum;
    int P, r_hit;
    int own_row;   // logical row of this ray
    int base_row;  // logical row of slot 0 of this chunk of this block
    int jj;        // slot within the launch chunk
    __device__ int real(int lrow) const { return lrow < r_hit ? lrow : 0; }
    __device__ int64_t at(int elem_from_H) const {
        const int e = jj * P + elem_from_H;
        const int lrow = base_row + e / P;
        const int col = e % P;
        return (int64_t)rank_ray[real(lrow) - row_begin] * kMaxHits + col;
    }
    __device__ int idx_at(int e) const {
        if (fast) return e < P ? hit_idx[own_base + e] : next_c0;  // beyond the own row only (row + 1, col 0) is read
        if (slot0) {
            const int lrow = base_row + (jj * P + e) / P;
            if (lrow < row_begin || lrow >= row_end) return next_col0;  // only (own row + 1, col 0) is read
        }
        return hit_idx[at(e)];
    }
    __device__ int idx_slot0(int col) const {
        // the slot-0 row's valid hits are its prefix [0, nv): only "== -1" is asked
        if (fast) return col < slot0_nv ? 0 : -1;
        if (slot0) return col < slot0[slot0_row] ? 0 : -1;
        return hit_idx[(int64_t)rank_ray[real(base_row)] * kMaxHits + col];
    }
    __device__ float lo_at(int e) const { return hit_t0[at(e)]; }
    __device__ float hi_at(int e) const { return hit_t1[at(e)]; }
    __device__ float prob_at(int e) const {
        const int64_t a = at(e);
        const float dd = hit_idx[a] != -1 ? hit_t1[a] - hit_t0[a] : 0.0f;
        return __fdiv_rn(dd, dsum[rank_ray[real(own_row)]]);
    }
    // bins of the ray's own row (e < P): logical row own_row = i < r_hit, no division
    int64_t own_base;  // rank_ray[own_row] * kMaxHits
    float own_dsum;
    __device__ int own_idx(int e) const { return hit_idx[own_base + e]; }
    __device__ float own_lo(int e) const { return hit_t0[own_base + e]; }
    __device__ float own_hi(int e) const { return hit_t1[own_base + e]; }
    __device__ float own_prob(int e) const {
        const int64_t a = own_base + e;
        const float dd = hit_idx[a] != -1 ? hit_t1[a] - hit_t0[a] : 0.0f;
        return __fdiv_rn(dd, own_dsum);
    }
    // data-parallel engine: this rank holds only the logical rows
    // [row_begin, row_end) (rank_ray / hit_* are local); the sampler reads
    // other rows only as slot 0's hit counts (the slot-0 table, built from
    // the exchanged counts) and as the first voxel id of the row after its
    // own (next_col0)
    const int *slot0 = nullptr;  // [200 · nch] valid hits of each launch chunk's slot-0 row
    int slot0_row = 0;           // table row of (block, chunk)
    int row_begin = 0, row_end = 0, next_col0 = -1;
    // the engine's launches (the by-rank copies of the traversal: hit count
    // and first id per rank): the two reads of other rows preloaded with the
    // ray's own row — no rank → ray → row chain
    bool fast = false;
    int slot0_nv = 0, next_c0 = -1;
};

__device__ __forceinline__ uint32_t mix32(uint64_t x) {
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return (uint32_t)x;
}

// inverse-CDF sampling of one ray; writes ≤ max_steps samples, returns count s.
template <typename Rows, typename Noise, typename Emit>
__device__ int sample_one(const Rows &rows, float steps_j, float fixed_step_size, int max_hits, int num_rays,
                          int H, int max_steps, Noise noise, Emit emit) {
    int bin = 0, s = 0;
    float lo_depth = rows.lo_at(0);
    float hi_depth = rows.hi_at(0);
    float lo_cdf = 0.0f;
    float hi_cdf = rows.prob_at(0);
    float step = (float)(1.0 / (double)steps_j);
    float z_low = lo_depth;
    const int total_steps = (int)ceilf(steps_j);
    bool done = false;
    if (fixed_step_size > 0.0f) step = fixed_step_size;
    for (int cs = 0; cs < total_steps; ++cs) {
        const float cdf = ((float)cs + noise(cs)) * step;
        while (cdf > hi_cdf) {
            if (s < max_steps) emit(s, rows.idx_at(bin), (hi_depth + z_low) * 0.5f, hi_depth - z_low);
            ++bin;
            ++s;
            if (bin >= max_hits || rows.idx_at(bin) == -1) {
                done = true;
                break;
            }
            lo_depth = rows.lo_at(bin);
            hi_depth = rows.hi_at(bin);
            lo_cdf = hi_cdf;
            hi_cdf = hi_cdf + rows.prob_at(bin);
            z_low = lo_depth;
        }
        if (done) break;
        const float u = __fdiv_rn(cdf - lo_cdf, hi_cdf - lo_cdf);
        const float z = lo_depth + u * (hi_depth - lo_depth);
        if (s < max_steps) emit(s, rows.idx_at(bin), (z + z_low) * 0.5f, z - z_low);
        z_low = z;
        ++s;
    }
    // sample_gpu.cu:224-237 verbatim semantics (see svo_oracle.c)
    while ((z_low < hi_depth) && (num_rays > (H + bin))) {
        if (s < max_steps) emit(s, rows.idx_at(bin), (hi_depth + z_low) * 0.5f, hi_depth - z_low);
        ++bin;
        ++s;
        if (bin >= max_hits || rows.idx_slot0(bin) == -1) break;
        lo_depth = rows.lo_at(bin);
        hi_depth = rows.hi_at(bin);
        z_low = lo_depth;
    }
    return s;
}

__global__ __launch_bounds__(64) void k_sample_raw(int b, int num_rays, int max_hits, int max_steps,
                                                   float fixed_step_size, const int *__restrict__ pts_idx,
                                                   const float *__restrict__ min_depth,
                                                   const float *__restrict__ max_depth,
                                                   const float *__restrict__ noise, const float *__restrict__ probs,
                                                   const float *__restrict__ steps, int *__restrict__ s_idx,
                                                   float *__restrict__ s_depth, float *__restrict__ s_dist) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (int64_t)b * num_rays) return;
    const int bi = (int)(gid / num_rays);
    const int j = (int)(gid % num_rays);
    const int64_t blk_h = (int64_t)bi * num_rays * max_hits;
    const int64_t blk_s = (int64_t)bi * num_rays * max_steps;
    RawRows rows{pts_idx + blk_h, min_depth + blk_h, max_depth + blk_h, probs + blk_h, j * max_hits};
    const int K = j * max_steps;
    const float *nz = noise + blk_s + K;
    int *oi = s_idx + blk_s + K;
    float *od = s_depth + blk_s + K;
    float *os = s_dist + blk_s + K;
    sample_one(
        rows, steps[(int64_t)bi * num_rays + j], fixed_step_size, max_hits, num_rays, j * max_hits, max_steps,
        [&](int cs) { return nz[cs]; },
        [&](int s, int v, float dep, float dis) {
            oi[s] = v;
            od[s] = dep;
            os[s] = dis;
        });
}

}  // namespace
}  // namespace psvo

using namespace psvo;

extern "C" int psvo_inverse_cdf_sampling(void *stream, int b, int num_rays, int max_hits, int max_steps,
                                         float fixed_step_size, const int *pts_idx, const float *min_depth,
                                         const float *max_depth, const float *uniform_noise, const float *probs,
                                         const float *steps, int *sampled_idx, float *sampled_depth,
                                         float *sampled_dists) {
    PSVO_REQUIRE(b >= 0 && num_rays >= 0 && max_hits > 0 && max_steps > 0,
                 "inverse_cdf_sampling: bad sizes b=%d num_rays=%d max_hits=%d max_steps=%d", b, num_rays, max_hits,
                 max_steps);
    const int64_t total = (int64_t)b * num_rays;
    if (total == 0) return PSVO_OK;
    psvo::launch(k_sample_raw, dim3(div_up(total, kWave)), dim3(kWave), 0, as_stream(stream), b, num_rays,
                       max_hits, max_steps, fixed_step_size, pts_idx, min_depth, max_depth, uniform_noise, probs,
                       steps, sampled_idx, sampled_depth, sampled_dists);
    return check_launch("inverse_cdf_sampling");
}

// ---------------------------------------------------------------------------
// The fused sampler (the engine's and psvo_sample_rays' path).
namespace psvo {
namespace {

// look-back blocks this unit's launches helped (lookback.h: a predecessor
// that had not started) — diagnostic, read by lb_helps_sample
__device__ unsigned long long psvo_g_lb_helps;
#ifdef PSVO_IS_STAMPS  // the diagnostic build's per-workgroup times (query_common.h SMP_T*)
__device__ unsigned long long psvo_g_smp_stamps[4096][8];
#endif

// Wave-parallel restatement of sample_one for one ray (one wave), valid when
// the cdf sequence ((cs + noise) * step) is non-decreasing — noise in [0, 1)
// and probs >= 0, which the fused path guarantees (probs are interval
// lengths / their sum; noise is clamped to [0.001, 0.999] or caller-given in
// [0, 1)).  The serial loop's output is a merge of two sorted streams:
//   interior sample cs in bin b(cs)   at position cs + b(cs)
//   end of bin b (bins it passed)     at position C_b + b
// with C_b = #{cs : !(cdf_cs > hcdf_b)} (first cs beyond bin b) and
// b(cs) = #{b : C_b <= cs}.  The trailing segment (sample_gpu.cu:224-237) is a
// run of consecutive bins whose first failing predicate a ballot finds.
// Every value is computed with the same float expressions as sample_one, so
// outputs are bit-identical to it.  Lane b owns bin b (max_hits <= 64).
struct WaveBins {  // per-wave LDS: bin b written by lane b, read by any lane
    float hc[kWave], lo[kWave], hi[kWave];
    int idx[kWave], c[kWave];
};

template <typename Rows, typename Noise, typename Emit>
__device__ int sample_wave(const Rows &rows, float steps_j, int max_hits, int num_rays, int H, Noise noise, Emit emit,
                           int lane, WaveBins &W) {
    const bool own = lane < max_hits;
    const int idx_b = own ? rows.own_idx(lane) : -1;
    const float lo_b = own ? rows.own_lo(lane) : 0.0f;
    const float hi_b = own ? rows.own_hi(lane) : 0.0f;
    const float prob_b = own ? rows.own_prob(lane) : 0.0f;
    // valid bins [0, nb): the serial loop stops at the first bin >= 1 with idx -1
    const uint64_t inval = __ballot(own && lane >= 1 && idx_b == -1);
    const int nb = inval ? min(__ffsll((unsigned long long)inval) - 1, max_hits) : max_hits;
    // hcdf_b: the serial running sum, same order of float additions
    SMP_T0(5);
    float acc = 0.0f, hcdf_b = 0.0f;
    for (int k = 0; k < nb; ++k) {
        const float pk = __shfl(prob_b, k, kWave);
        acc = (k == 0) ? pk : acc + pk;
        if (k == lane) hcdf_b = acc;
    }
    const float step = (float)(1.0 / (double)steps_j);
    const int total_steps = (int)ceilf(steps_j);
    auto cdf_at = [&](int cs) { return ((float)cs + noise(cs)) * step; };
    // C_b = first cs in [0, total_steps) with cdf_cs > hcdf_b (total_steps if none)
    int c_b = 0x7fffffff;  // bins past nb never end by cdf
    if (lane < nb) {
        int lo = 0, hi = total_steps;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cdf_at(mid) > hcdf_b) hi = mid; else lo = mid + 1;
        }
        c_b = lo;
    }
    W.hc[lane] = hcdf_b;
    W.lo[lane] = lo_b;
    W.hi[lane] = hi_b;
    W.idx[lane] = idx_b;
    W.c[lane] = c_b;
    wave_lds_sync();
    SMP_T0(6);
    const int cs_end = W.c[nb - 1];  // first cs past the last valid bin
    const bool done = cs_end < total_steps;
    const int cs_lim = done ? cs_end : total_steps;
    // b(cs) = #{b < nb : C_b <= cs}; C_b is non-decreasing in b
    auto bin_of = [&](int cs) {
        int lo = 0, hi = nb;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (W.c[mid] <= cs) lo = mid + 1; else hi = mid;
        }
        return lo;
    };
    auto c_before = [&](int b) { return b == 0 ? 0 : W.c[b - 1]; };
    // z of interior sample c lying in bin b (sample_one: u, z)
    auto z_at = [&](int c, int b) {
        const float hc = W.hc[b];
        const float lc = b == 0 ? 0.0f : W.hc[b - 1];
        const float lo = W.lo[b], hi = W.hi[b];
        const float u = __fdiv_rn(cdf_at(c) - lc, hc - lc);
        return lo + u * (hi - lo);
    };
    // interior samples; z(cs - 1) comes from the neighbouring lane (the loop
    // bound is wave-uniform, so every lane takes part in the shuffles)
    float carry = 0.0f;
    for (int base = 0; base < cs_lim; base += kWave) {
        const int cs = base + lane;
        const bool act = cs < cs_lim;
        const int b = act ? bin_of(cs) : 0;
        const float z = act ? z_at(cs, b) : 0.0f;
        float zp = __shfl(z, lane > 0 ? lane - 1 : 0, kWave);
        if (lane == 0) zp = carry;
        carry = __shfl(z, kWave - 1, kWave);
        if (act) {
            const float z_low = cs == c_before(b) ? W.lo[b] : zp;
            emit(cs + b, W.idx[b], (z + z_low) * 0.5f, z - z_low);
        }
    }
    SMP_T0(7);
    // ends of the bins the main loop passed
    const int b_last = total_steps > 0 && !done ? bin_of(total_steps - 1) : 0;
    const int n_ends = done ? nb : b_last;
    // z_low at the end of bin b: its last interior sample, or lo_b if it has none
    auto end_z_low = [&](int b) { return W.c[b] > c_before(b) ? z_at(W.c[b] - 1, b) : W.lo[b]; };
    if (lane < n_ends) emit(c_b + lane, idx_b, (hi_b + end_z_low(lane)) * 0.5f, hi_b - end_z_low(lane));
    int s = cs_lim + n_ends;
    // trailing segment
    int bin0;
    float zl, hi_d;
    if (done) {
        bin0 = nb;
        zl = end_z_low(nb - 1);
        hi_d = W.hi[nb - 1];
    } else if (total_steps == 0) {
        bin0 = 0;
        zl = W.lo[0];
        hi_d = W.hi[0];
    } else {
        bin0 = b_last;
        zl = z_at(total_steps - 1, b_last);
        hi_d = W.hi[b_last];
    }
    if (zl < hi_d && num_rays > H + bin0) {
        const int v0 = bin0 < max_hits ? W.idx[bin0] : rows.idx_at(bin0);
        if (lane == 0) emit(s, v0, (hi_d + zl) * 0.5f, hi_d - zl);
        // bins k > bin0 continue while idx_slot0(k) != -1 && lo < hi && num_rays > H + k
        const bool cont = own && lane > bin0 && rows.idx_slot0(lane) != -1 && lo_b < hi_b && num_rays > H + lane;
        const uint64_t fail = ~__ballot(cont) & (~0ull << (bin0 + 1 < 64 ? bin0 + 1 : 63));
        const int k_end = bin0 + 1 >= 64 ? bin0 + 1 : (fail ? __ffsll((unsigned long long)fail) - 1 : 64);
        if (lane > bin0 && lane < k_end) emit(s + (lane - bin0), idx_b, (hi_b + lo_b) * 0.5f, hi_b - lo_b);
        s += k_end - bin0;
    }
    return s;
}

// Rows [row_begin, row_begin + n_rows) of the logical hit-ray order (n_rows <
// 0: through R_hit); ray i's outputs go to row i - row_begin.  A data-
// parallel rank samples its own rays inside the GLOBAL [200, K', P] layout
// this way: rank_ray / hit_* / dsum / stats then describe
// the all-gathered batch, and the noise key is the global logical index.
// the scan of the ray sample counts, the normaliser sums and the statistics
// read-back inside the sampler launch by decoupled look-back (single GPU;
// desc == nullptr: k_scan_samples runs after the launch instead)
struct SampleTail {
    int *offsets;              // [R_hit + 1] exclusive scan of ray_ns
    unsigned long long *host;  // PSVO_STAT_WORDS granules (stat_to_host)
    int seq;
    SampleCounts c;            // the Criterion's normalisers (c.gt_depth null: not counted)
    unsigned long long *desc;  // look-back descriptors (lookback.h), or null
    uint32_t tag;              // this launch's descriptor tag
    // with desc: the ray-major compacted samples (k_compact_rays' output:
    // leaf / t / ray_of_sample at offsets[r] + s, capacity R · max_steps_cap),
    // or null.  With desc the rows hold only their valid prefix (no padding:
    // every reader implies (-1, MAX_DEPTH) past the ray's count)
    int *leaf;
    float *t;
    int *ray_of;
    int *m_out;  // or null: the batch's sample count M, on the device (the step's device-sized forward)
    LbCtl ctl;   // lookback.h (tests: psvo_debug_set_lookback)
};
constexpr int kSmpStage = 256;  // a row's first samples staged in LDS for the in-launch compaction
// ray_cnt word: valid front / sdf samples (12 bits each), then whether a
// padded sample (z = MAX_DEPTH) is front / sdf, whether the ray's depth is valid
__device__ __forceinline__ int pack_counts(int nf, int nsm, bool pf, bool psm, bool valid) {
    return nf | (nsm << 12) | ((int)pf << 24) | ((int)psm << 25) | ((int)valid << 26);
}

// the sampler's look-back state (wave 0): the own block's aggregate {M,
// S_max, nf, nsm, Σ_pf ns, Σ_psm ns, pf | psm << 16, valid}, its lanes'
// in-block offsets, its exclusive prefix and the wait's state
struct SmpLb {  // in LDS: nothing of it stays in registers across the help passes
    uint32_t agg[kLbSmpGranules], ex[kLbSmpGranules];
    int before[kSmpWaves], rc, spins;
};

// one ray of k_sample_fused; returns its valid-sample count, or -1 when the
// wave has no ray (the launch covers r_hit_cap rows)
template <bool HELP = false>
__device__ __forceinline__ int sample_fused_ray(int64_t row_begin, int64_t n_rows, int64_t r_hit_cap,
                                                int max_steps_cap, const int *__restrict__ rank_ray,
                                                const int *__restrict__ hit_idx, const float *__restrict__ hit_t0,
                                                const float *__restrict__ hit_t1, const float *__restrict__ ray_dsum,
                                                float step_size, const float *__restrict__ noise, uint64_t seed,
                                                int *__restrict__ stats, int *__restrict__ s_idx,
                                                float *__restrict__ s_depth, float *__restrict__ s_dist,
                                                const int *__restrict__ slot0, int slot0_nch,
                                                const int *__restrict__ nv_rank, const int *__restrict__ col0_rank,
                                                int &il_out, WaveBins &W, const SampleTail &tl, int &cnt_word,
                                                int *stage_i, float *stage_z, int blk, int wrow = -1) {
    // look-back mode: P / R_hit / max ⌈steps⌉ from the traversal's copy, which
    // no workgroup of this launch re-zeroes (a workgroup may start after the
    // last one zeroed the statistics: lookback.h helping)
    const int *qp = tl.desc ? stats + kStatQuery : stats;
    const int P = qp[PSVO_STAT_P];
    const int r_hit = qp[PSVO_STAT_R_HIT];
    const int max_steps = qp[PSVO_STAT_MAX_CEIL] + P;
    // the engine's launches (row_begin 0, or a data-parallel rank's own rows
    // indexed locally): the ray's rank → ray read beside the statistics words
    // the block's row of this wave (HELP: of this lane, wrow)
    if (wrow < 0) wrow = threadIdx.x / kWave;
    const int il_s = blk * (blockDim.x / kWave) + wrow;
    const int orig_s = (nv_rank && il_s < r_hit_cap) ? rank_ray[il_s] : 0;
    if (slot0) {  // data-parallel engine: the rank's rows, local rank_ray / hit arrays
        row_begin = stats[PSVO_STAT_ROW_BEGIN];
        n_rows = stats[PSVO_STAT_R_HIT_LOCAL];
    }
    const int lane = threadIdx.x & (kWave - 1);
    const int il = blk * (blockDim.x / kWave) + wrow;  // one ray per wave (HELP: per lane)
    const int i = (int)row_begin + il;                                        // logical row
    il_out = il;
    const int64_t n_own = n_rows < 0 ? (int64_t)r_hit - row_begin : n_rows;
    if (i >= r_hit || il >= n_own || il >= r_hit_cap || P <= 0) return -1;
    // (look-back mode: the last workgroup derives this flag; no atomics on `stats`)
    if (!tl.desc && max_steps > max_steps_cap && lane == 0 && il == 0)
        atomicOr(stats + PSVO_STAT_FLAGS, kStatFlagSamplerOverflow);
    const int kp = (r_hit + kSamplerG - 1) / kSamplerG;
    const int b = i / kp;
    const int j = i - b * kp;
    const int c = j / kSamplerChunk;
    const int jj = j - c * kSamplerChunk;
    const int nr = min(kSamplerChunk, kp - c * kSamplerChunk);
    const int orig = nv_rank ? orig_s : slot0 ? rank_ray[il] : rank_ray[i];
    // look-back mode (r_hit_cap = the batch's rays): a rank outside it only
    // after an abandoned look-back wait (flagged) — no row
    if (tl.desc && (orig < 0 || orig >= r_hit_cap)) return -1;
    const float dsum = ray_dsum[orig];
    FusedRows rows{rank_ray, hit_idx, hit_t0, hit_t1, ray_dsum, P, r_hit, i, b * kp + c * kSamplerChunk, jj,
                   (int64_t)orig * kMaxHits, dsum};
    if (slot0) {
        if (c >= slot0_nch) {  // the exchanged table covers slot0_nch launch chunks
            if (lane == 0) atomicOr(stats + PSVO_STAT_FLAGS, kStatFlagUnionOverflow);
            return -1;
        }
        rows.slot0 = slot0;
        rows.slot0_row = b * slot0_nch + c;
        rows.row_begin = (int)row_begin;
        rows.row_end = (int)(row_begin + n_rows);
        rows.next_col0 = stats[PSVO_STAT_NEXT_COL0];
    }
    if (nv_rank) {  // the two reads of other rows, beside the own row's loads
        rows.fast = true;
        if (slot0) {
            rows.slot0_nv = slot0[rows.slot0_row];
            rows.next_c0 = il + 1 < n_rows ? col0_rank[il + 1] : rows.next_col0;
        } else {
            rows.slot0_nv = nv_rank[rows.base_row];  // base_row <= i < R_hit
            rows.next_c0 = col0_rank[i + 1 < r_hit ? i + 1 : 0];
        }
    }
    const float steps_j = __fdiv_rn(dsum, step_size);
    const int cap = max_steps < max_steps_cap ? max_steps : max_steps_cap;
    const bool nopad = tl.desc != nullptr;  // look-back mode: rows end at their valid prefix
    int *oi = s_idx + (int64_t)il * max_steps_cap;
    float *od = s_depth + (int64_t)il * max_steps_cap;
    float *os = s_dist ? s_dist + (int64_t)il * max_steps_cap : nullptr;  // the engine reads no distances
    const float *nz = noise ? noise + ((int64_t)b * kp + j) * max_steps : nullptr;
    const uint64_t key = seed * 0x9E3779B97F4A7C15ull + ((uint64_t)(b * kp + j) << 20);
    int count = 0;
    // the normalisers' per-sample terms (criterion.hip sample_terms) on the stored depths
    const bool counting = tl.c.gt_depth != nullptr;
    const float gd = counting ? tl.c.gt_depth[orig] : 0.f;
    const float lo_t = gd - tl.c.tr, hi_t = gd + tl.c.tr;
    const bool dm = gd > 0.0f && gd < tl.c.max_depth;
    int nf = 0, nsm = 0;
    auto noise_at = [&](int cs) {
        if (nz) return nz[cs];
        const float u = (float)(mix32(key + (uint64_t)cs) >> 8) * (1.0f / 16777216.0f);
        return fminf(fmaxf(u, 0.001f), 0.999f);
    };
    if constexpr (HELP) {
        // a helped row (lookback.h), one per lane: its count and count word
        // only, by the serial loop the wave sampler restates bit for bit
        // (sample_one) — small code; the row's owner writes it when it runs
        sample_one(rows, steps_j, 0.0f, P, nr, jj * P, cap, noise_at, [&](int s, int v, float dep, float) {
            if (s >= cap || v == -1) return;
            ++count;
            if (counting) {
                const bool f = dep < lo_t;
                nf += f;
                nsm += !f && !(dep > hi_t) && dm;
            }
        });
        if (counting) {
            const bool pf = kMaxDepthFill < lo_t;
            const bool psm = !pf && !(kMaxDepthFill > hi_t) && dm;
            cnt_word = pack_counts(nf, nsm, pf, psm, gd > 0.01f && gd < tl.c.max_depth);
        }
        return count;
    }
    const int s_end = sample_wave(
        rows, steps_j, P, nr, jj * P, noise_at,
        [&](int s, int v, float dep, float dis) {
            if (s >= cap) return;
            if (nopad && v == -1) return;  // the implied padding
            // voxel_helpers.py:654-656: clamp dists, MAX_DEPTH / 0 where idx == -1
            oi[s] = v;
            od[s] = v == -1 ? kMaxDepthFill : dep;
            if (os) os[s] = v == -1 ? 0.0f : fmaxf(dis, 0.0f);
            if (stage_i && s < kSmpStage) {  // v != -1 here (nopad)
                stage_i[s] = v;
                stage_z[s] = dep;
            }
            count += (v != -1);
            if (counting && v != -1) {
                const bool f = dep < lo_t;
                nf += f;
                nsm += !f && !(dep > hi_t) && dm;
            }
        },
        lane, W);
    const int s_written = nopad ? cap : s_end < cap ? s_end : cap;
    for (int s = s_written + lane; s < cap; s += kWave) {  // up to max_steps: readers stop at S_max <= max_steps
        oi[s] = -1;
        od[s] = kMaxDepthFill;
        if (os) os[s] = 0.0f;
    }
    if (counting) {
        const bool pf = kMaxDepthFill < lo_t;  // a padded sample: z = MAX_DEPTH
        const bool psm = !pf && !(kMaxDepthFill > hi_t) && dm;
        cnt_word = pack_counts(wave_sum(nf), wave_sum(nsm), pf, psm, gd > 0.01f && gd < tl.c.max_depth);
    }
    return wave_sum(count);
}

// k_scan_samples' work for one sampler workgroup (its 8 rows), wave 0 only,
// in two parts.  smp_lb_pass: the aggregate of block `cur`'s rows {M, S_max,
// and with the normalisers nf, nsm, Σ_pf ns, Σ_psm ns, pf | psm << 16,
// valid} — the own block's kept in `lb`, a helped block's published — then
// the own block's look-back (lookback.h lb_scan_help: returns the next block
// to help, or done / failed).  smp_lb_finish: its rows' offsets; the
// workgroup holding row n − 1 (block 0 when there is no row) writes
// offsets[n], the loss coefficients and the statistics read-back (granules,
// no system-scope release), and zeroes the device statistics for the next
// query.  Integer sums: exact, the same totals as k_scan_samples.
__device__ int smp_lb_pass(bool own, int cur, int blk, int nb, const int *s_ns, const int *s_cw, const SampleTail &tl,
                           SmpLb &lb) {
    constexpr int NG = kLbSmpGranules;
    const int lane = threadIdx.x & (kWave - 1);
    uint32_t agg[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) agg[g] = 0;
    int before = 0;  // samples of this workgroup's rows in front of lane's row
    const bool counting = tl.c.gt_depth != nullptr;
#pragma unroll
    for (int k = 0; k < kSmpWaves; ++k) {
        const int c = max(s_ns[k], 0);
        before += k < lane ? c : 0;
        agg[0] += (uint32_t)c;
        agg[1] = max(agg[1], (uint32_t)c);
        if (counting) {
            const int cw = s_ns[k] >= 0 ? s_cw[k] : 0;
            const int pf = (cw >> 24) & 1, psm = (cw >> 25) & 1;
            agg[2] += (uint32_t)(cw & 0xFFF);
            agg[3] += (uint32_t)((cw >> 12) & 0xFFF);
            agg[4] += pf ? (uint32_t)c : 0u;
            agg[5] += psm ? (uint32_t)c : 0u;
            agg[6] += (uint32_t)(pf | (psm << 16));
            agg[7] += (uint32_t)((cw >> 26) & 1);
        }
    }
    int spins = 0;
    if (own) {
#pragma unroll
        for (int g = 0; g < NG; ++g)
            if (lane == g) lb.agg[g] = agg[g];
        if (lane < kSmpWaves) lb.before[lane] = before;
    } else {
        lb_publish<NG>(tl.desc, cur, lane, agg, tl.tag);
        if (lane == 0) atomicAdd(&psvo_g_lb_helps, 1ull);
#pragma unroll
        for (int g = 0; g < NG; ++g) agg[g] = lb.agg[g];  // the own aggregate again
        spins = lb.spins;
    }
    uint32_t ex[NG];
    const int rc = lb_scan_help<NG, 0b10u>(tl.desc, blk, nb, tl.tag, lane, agg, ex, spins, tl.ctl.spin_max);
    if (lane == 0) {
        lb.rc = rc;
        lb.spins = spins;
    }
    if (rc == kLbDone) {
#pragma unroll
        for (int g = 0; g < NG; ++g)
            if (lane == g) lb.ex[g] = ex[g];
    }
    return rc;
}

__device__ void smp_lb_finish(int n, const SmpLb &lb, int *__restrict__ stats, const SampleTail &tl, int *s_off,
                              int st_word, int max_steps_cap, int blk) {
    const int lane = threadIdx.x & (kWave - 1);
    const bool ok = lb.rc == kLbDone;
    uint32_t ex[kLbSmpGranules], agg[kLbSmpGranules];
#pragma unroll
    for (int g = 0; g < kLbSmpGranules; ++g) {
        ex[g] = lb.ex[g];
        agg[g] = lb.agg[g];
    }
    const int last = n > 0 ? (n - 1) / kSmpWaves : 0;  // the workgroups past it returned without a descriptor
    const int il = blk * kSmpWaves + lane;
    const int before = lane < kSmpWaves ? lb.before[lane] : 0;
    // an abandoned wait (!ok: `ex` undefined) stores offset 0 (an in-bounds
    // range for any reader; the batch is reported failed) and the compaction
    // skips its rows
    if (lane < kSmpWaves) s_off[lane] = ok ? (int)ex[0] + before : -1;  // the in-launch compaction's
    if (lane < kSmpWaves && il < n) tl.offsets[il] = ok ? (int)ex[0] + before : 0;
    if (blk != last) return;
    const int tot = ok ? (int)(ex[0] + agg[0]) : 0;
    const int smax = ok ? (int)max(ex[1], agg[1]) : 0;
    if (lane == 0) {
        tl.offsets[n] = tot;
        if (tl.m_out) *tl.m_out = tot;  // an abandoned wait: no samples (the flag reports it)
    }
    if (tl.c.gt_depth && lane == 0) {  // the count sums over the padded [R_hit, S_max] layout (criterion.py:70-101)
        const uint32_t pp = ex[6] + agg[6];
        const long long t_nf = ex[2] + agg[2], t_nsm = ex[3] + agg[3], t_nspf = ex[4] + agg[4],
                        t_nspsm = ex[5] + agg[5], t_pf = pp & 0xFFFF, t_psm = pp >> 16, t_valid = ex[7] + agg[7];
        const long long n_f = t_nf + (long long)smax * t_pf - t_nspf;
        const long long n_s = t_nsm + (long long)smax * t_psm - t_nspsm;
        crit_coef_from_counts((double)t_valid, (double)n_f, (double)n_s, (double)n, (double)smax, tl.c.w_rgb,
                              tl.c.w_depth, tl.c.w_fs, tl.c.w_sdf, tl.c.tr, tl.c.crit_flags, tl.c.coef);
    }
    // the sampler's own flag (sample_fused_ray: max_steps beyond the rows' capacity)
    // (st_word: the last workgroup's load at its start — only it re-zeroes
    // the statistics, so its words are the traversal's; no dependent load here)
    const int max_steps = __shfl(st_word, PSVO_STAT_MAX_CEIL, kWave) + __shfl(st_word, PSVO_STAT_P, kWave);
    if (lane < PSVO_STAT_WORDS) {
        int v = lane == PSVO_STAT_S_MAX ? smax : lane == PSVO_STAT_M ? tot : st_word;
        if (lane == PSVO_STAT_FLAGS && n > 0 && max_steps > max_steps_cap) v |= kStatFlagSamplerOverflow;
        if (lane == PSVO_STAT_FLAGS && !ok) v |= kLbFlagTimeout;
        if (lane < kStatQuery) stats[lane] = 0;  // ready for the query set's next use (no memset launch)
        if (tl.host) stat_to_host(tl.host, lane, v, tl.seq);
    }
}

__global__ __launch_bounds__(64 * kSmpWaves) void k_sample_fused(int64_t row_begin, int64_t n_rows, int64_t r_hit_cap,
                                                      int max_steps_cap,
                                                      const int *__restrict__ rank_ray,
                                                      const int *__restrict__ hit_idx,
                                                      const float *__restrict__ hit_t0,
                                                      const float *__restrict__ hit_t1,
                                                      const float *__restrict__ ray_dsum, float step_size,
                                                      const float *__restrict__ noise, uint64_t seed,
                                                      int *__restrict__ stats, int *__restrict__ s_idx,
                                                      float *__restrict__ s_depth, float *__restrict__ s_dist,
                                                      int *__restrict__ ray_ns, const int *__restrict__ slot0,
                                                      int slot0_nch, SampleTail tl, const int *__restrict__ nv_rank,
                                                      const int *__restrict__ col0_rank) {
    __shared__ WaveBins bins_all[kSmpWaves];
    // look-back mode (the engine's single-GPU query: row_begin 0, all rows):
    // the rows of this batch from the traversal's copy of its statistics
    // (kStatQuery: never re-zeroed inside this launch)
    const int blk = (int)blockIdx.x;
    const int *qp = stats + kStatQuery;
    const int n_lb = tl.desc && qp[PSVO_STAT_P] > 0 ? (int)min((int64_t)qp[PSVO_STAT_R_HIT], r_hit_cap) : 0;
    const int last_lb = n_lb > 0 ? (n_lb - 1) / kSmpWaves : 0;  // the workgroup holding the last row
    if (tl.desc && blk > last_lb) return;
    if (tl.desc) {
        lb_debug_delay(tl.ctl, blk);
        if (threadIdx.x == 0) lb_mark_started<kLbSmpGranules>(tl.desc, blk, last_lb + 1, tl.tag);
    }
    __shared__ int stage_i[kSmpWaves][kSmpStage];
    __shared__ float stage_z[kSmpWaves][kSmpStage];
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    SMP_T(0);
    const bool compact = tl.desc && tl.leaf;
    // the statistics words for the read-back, loaded now (the traversal's
    // are final; the one flag this launch adds is derived, not re-read):
    // no dependent round trip after the look-back in the last workgroup
    const int st_word = tl.desc && w == 0 && lane < PSVO_STAT_WORDS ? stats[lane] : 0;
    int il = 0, cnt_word = 0;
    int count = sample_fused_ray(row_begin, n_rows, r_hit_cap, max_steps_cap, rank_ray, hit_idx, hit_t0, hit_t1,
                                 ray_dsum, step_size, noise, seed, stats, s_idx, s_depth, s_dist, slot0, slot0_nch,
                                 nv_rank, col0_rank, il, bins_all[w], tl, cnt_word,
                                 compact ? stage_i[w] : nullptr, compact ? stage_z[w] : nullptr, blk);
    SMP_T(1);
    if (!tl.desc) {  // k_scan_samples reads them after the launch
        if (count >= 0 && lane == 0) {
            ray_ns[il] = count;
            if (tl.c.gt_depth) tl.c.ray_cnt[il] = cnt_word;
        }
        return;
    }
    __shared__ int s_ns[kSmpWaves], s_cw[kSmpWaves], s_off[kSmpWaves];
    if (lane == 0) {
        if (count >= 0) ray_ns[il] = count;
        s_ns[w] = count;  // -1: no row
        s_cw[w] = cnt_word;
    }
    // the counts publish before the rows' stores drain: a workgroup's
    // successors wait for its aggregate, not for its stores (measured: the
    // drain in front of the look-back cost up to 7 µs at the launch's tail)
    __syncthreads();
    SMP_T(2);
    __shared__ SmpLb lb;  // wave 0: the own block's aggregate / prefix
    if (w == 0) {
        // a predecessor that has not started: wave 0 counts its rows (one
        // per lane, the serial sampler) and publishes their aggregate, then
        // resumes its own look-back (lookback.h)
        __shared__ int s_hns[kSmpWaves], s_hcw[kSmpWaves];
        int rc = smp_lb_pass(true, blk, blk, last_lb + 1, s_ns, s_cw, tl, lb);
        while (rc >= 0) {
            if (lane < kSmpWaves) {
                int hil = 0, hcw = 0;
                const int hc = sample_fused_ray<true>(row_begin, n_rows, r_hit_cap, max_steps_cap, rank_ray, hit_idx,
                                                      hit_t0, hit_t1, ray_dsum, step_size, noise, seed, stats, s_idx,
                                                      s_depth, s_dist, slot0, slot0_nch, nv_rank, col0_rank, hil,
                                                      bins_all[0], tl, hcw, nullptr, nullptr, rc, lane);
                s_hns[lane] = hc;
                s_hcw[lane] = hcw;
            }
            rc = smp_lb_pass(false, rc, blk, last_lb + 1, s_hns, s_hcw, tl, lb);
        }
    }
    const int own_count = count, own_il = il;
    if (w == 0) smp_lb_finish(n_lb, lb, stats, tl, s_off, st_word, max_steps_cap, blk);
    SMP_T(3);
    if (!compact) return;
    // a row longer than the LDS stage is re-read below: this wave's own stores first
    if (own_count > kSmpStage) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // k_compact_rays' work: the row's valid prefix to its compacted place —
    // the first kSmpStage samples from LDS, the rest (rows longer than that)
    // read back from the row with sc1 loads (this wave's own stores, past L1)
    const int off = s_off[w];
    if (own_count <= 0 || off < 0) return;
    const int *oi = s_idx + (int64_t)own_il * max_steps_cap;
    const float *od = s_depth + (int64_t)own_il * max_steps_cap;
    for (int s = lane; s < own_count; s += kWave) {
        const bool st = s < kSmpStage;
        tl.leaf[off + s] = st ? stage_i[w][s] : ld_wt(oi + s);
        tl.t[off + s] = st ? stage_z[w][s] : ld_wt(od + s);
        tl.ray_of[off + s] = own_il;
    }
    SMP_T(4);
}

// offsets[0..R_hit] = exclusive scan of ray_ns; S_max and M into stats.  With
// `host` the statistics go to the host and `stats` is zeroed for the next
// query.
__global__ __launch_bounds__(1024) void k_scan_samples(int64_t row_begin, int64_t n_rows, int64_t r_hit_cap,
                                                       const int *__restrict__ ray_ns, int *__restrict__ offsets,
                                                       int *__restrict__ stats, int dist, unsigned long long *host,
                                                       int seq, SampleCounts cnt) {
    __shared__ int total;
    __shared__ int smax[16];
    __shared__ long long s_c[7][16];
    const int64_t n_own = dist ? (int64_t)stats[PSVO_STAT_R_HIT_LOCAL]
                               : n_rows < 0 ? (int64_t)stats[PSVO_STAT_R_HIT] - row_begin : n_rows;
    const int64_t n = max((int64_t)0, min(n_own, r_hit_cap));
    const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid / kWave, nw = blockDim.x / kWave;
    if ((n + blockDim.x - 1) / blockDim.x <= kRegRun) {
        // ≤ 8 rays per thread (R_hit ≤ 8,192): one round of independent loads —
        // the ray's sample count and its normaliser count word side by side —,
        // run sums / maxima / count sums in registers (32-bit: ≤ 8,192 rays of
        // ≤ 4,095 counts), one barrier, then the wave totals combined in
        // registers (every thread reads the ≤ 16 wave words it needs)
        __shared__ int s_wave[16], s_red[8][16];
        const int per = (int)((n + blockDim.x - 1) / blockDim.x);
        const int64_t beg = (int64_t)tid * per;
        int vals[kRegRun], cw[kRegRun];
#pragma unroll
        for (int k = 0; k < kRegRun; ++k) {
            const bool in = k < per && beg + k < n;
            vals[k] = in ? ray_ns[beg + k] : 0;
            cw[k] = in && cnt.gt_depth ? cnt.ray_cnt[beg + k] : 0;
        }
        int local = 0, mx = 0, c[7] = {0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < kRegRun; ++k) {
            local += vals[k];
            mx = max(mx, vals[k]);
            const int pf = (cw[k] >> 24) & 1, psm = (cw[k] >> 25) & 1;
            c[0] += cw[k] & 0xFFF;
            c[1] += (cw[k] >> 12) & 0xFFF;
            c[2] += pf;
            c[3] += psm;
            c[4] += (cw[k] >> 26) & 1;
            c[5] += pf ? vals[k] : 0;
            c[6] += psm ? vals[k] : 0;
        }
        int incl = local;
#pragma unroll
        for (int sh = 1; sh < kWave; sh <<= 1) {
            const int t = __shfl_up(incl, sh, kWave);
            if (lane >= sh) incl += t;
        }
        mx = wave_max(mx);
        if (cnt.gt_depth) {
#pragma unroll
            for (int k = 0; k < 7; ++k) c[k] = wave_sum(c[k]);
        }
        if (lane == kWave - 1) s_wave[w] = incl;
        if (lane == 0) {
            s_red[7][w] = mx;
#pragma unroll
            for (int k = 0; k < 7; ++k) s_red[k][w] = c[k];
        }
        __syncthreads();
        int before = 0, tot = 0;
        for (int k = 0; k < nw; ++k) {
            const int v = s_wave[k];
            before += k < w ? v : 0;
            tot += v;
        }
        int run = before + incl - local;
#pragma unroll
        for (int k = 0; k < kRegRun; ++k)
            if (k < per && beg + k < n) {
                offsets[beg + k] = run;
                run += vals[k];
            }
        if (w != 0) return;
        // wave 0: the block's maximum and count sums over the ≤ 16 wave words
        const bool wl = lane < nw;
        int bm = wl ? s_red[7][lane] : 0;
#pragma unroll
        for (int sh = 8; sh > 0; sh >>= 1) bm = max(bm, __shfl_xor(bm, sh, kWave));
        bm = __shfl(bm, 0, kWave);
        if (lane == 0) offsets[n] = tot;
        if (cnt.gt_depth) {
            int t[7];
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                int v = wl ? s_red[k][lane] : 0;
#pragma unroll
                for (int sh = 8; sh > 0; sh >>= 1) v += __shfl_xor(v, sh, kWave);
                t[k] = v;
            }
            if (lane == 0) {  // the count sums over the padded [R_hit, S_max] layout → coefficients
                const long long n_f = (long long)t[0] + (long long)bm * t[2] - t[5];
                const long long n_s = (long long)t[1] + (long long)bm * t[3] - t[6];
                crit_coef_from_counts((double)t[4], (double)n_f, (double)n_s, (double)n, (double)bm, cnt.w_rgb,
                                      cnt.w_depth, cnt.w_fs, cnt.w_sdf, cnt.tr, cnt.crit_flags, cnt.coef);
            }
        }
        if (host) {  // the engine's read-back (every reader of stats is past the barrier)
            if (lane < PSVO_STAT_WORDS) {
                const int v = lane == PSVO_STAT_S_MAX ? bm : lane == PSVO_STAT_M ? tot : stats[lane];
                stats[lane] = 0;
                stat_to_host(host, lane, v, seq);
            }
        } else if (lane == 0) {
            stats[PSVO_STAT_S_MAX] = bm;
            stats[PSVO_STAT_M] = tot;
        }
        return;
    }
    int mx = 0;
    block_scan_runs(n, [&](int64_t i) { return ray_ns[i]; }, offsets, &total, &mx);
    mx = wave_max(mx);
    if (lane == 0) smax[w] = mx;
    if (cnt.gt_depth) {  // the loss normalisers' per-ray counts (k_sample_fused), exact integer sums
        long long c[7] = {};
        for (int64_t i0 = tid; i0 < n; i0 += (int64_t)blockDim.x * 8) {
            int cw[8], ns[8];  // one round of independent loads, then the sums
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int64_t i = i0 + (int64_t)k * blockDim.x;
                cw[k] = i < n ? cnt.ray_cnt[i] : 0;
                ns[k] = i < n ? ray_ns[i] : 0;
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int pf = (cw[k] >> 24) & 1, psm = (cw[k] >> 25) & 1;
                c[0] += cw[k] & 0xFFF;
                c[1] += (cw[k] >> 12) & 0xFFF;
                c[2] += pf;
                c[3] += psm;
                c[4] += (cw[k] >> 26) & 1;
                c[5] += pf ? ns[k] : 0;
                c[6] += psm ? ns[k] : 0;
            }
        }
#pragma unroll
        for (int k = 0; k < 7; ++k) {
#pragma unroll
            for (int sh = 32; sh > 0; sh >>= 1) c[k] += __shfl_xor(c[k], sh, kWave);
            if (lane == 0) s_c[k][w] = c[k];
        }
    }
    __syncthreads();
    if (tid < kWave) {  // wave 0; with `host` one statistics word per lane (no serial copy loop)
        for (int k = 1; k < nw; ++k) mx = max(mx, smax[k]);
        const int tot = total;
        if (lane == 0) offsets[n] = tot;
        if (cnt.gt_depth && lane == 0) {  // the count sums over the padded [R_hit, S_max] layout → coefficients
            long long t[7];
            for (int k = 0; k < 7; ++k) {
                t[k] = 0;
                for (int q = 0; q < nw; ++q) t[k] += s_c[k][q];
            }
            const long long n_f = t[0] + (long long)mx * t[2] - t[5];
            const long long n_s = t[1] + (long long)mx * t[3] - t[6];
            crit_coef_from_counts((double)t[4], (double)n_f, (double)n_s, (double)n, (double)mx, cnt.w_rgb,
                                  cnt.w_depth, cnt.w_fs, cnt.w_sdf, cnt.tr, cnt.crit_flags, cnt.coef);
        }
        if (host) {  // the engine's read-back, as k_stats_to_host (every reader of stats is past the barrier)
            if (lane < PSVO_STAT_WORDS) {
                const int v = lane == PSVO_STAT_S_MAX ? mx : lane == PSVO_STAT_M ? tot : stats[lane];
                stats[lane] = 0;
                stat_to_host(host, lane, v, seq);
            }
        } else if (lane == 0) {
            stats[PSVO_STAT_S_MAX] = mx;
            stats[PSVO_STAT_M] = tot;
        }
    }
}

}  // namespace
}  // namespace psvo

extern "C" int psvo_sample_rays_range(void *stream, int64_t row_begin, int64_t n_rows, int64_t r_hit_cap,
                                      int max_steps_cap, const int *rank_ray, const int *hit_idx,
                                      const float *hit_t0, const float *hit_t1, const float *ray_dsum,
                                      float step_size, const float *noise, uint64_t seed, int *stats, int *s_idx,
                                      float *s_depth, float *s_dist, int *ray_ns, int *offsets) {
    PSVO_REQUIRE(r_hit_cap >= 0 && max_steps_cap > 0, "sample_rays: bad caps");
    PSVO_REQUIRE(row_begin >= 0, "sample_rays: row_begin < 0");
    PSVO_REQUIRE(offsets != nullptr && ray_ns != nullptr, "sample_rays: ray_ns / offsets required");
    if (r_hit_cap == 0) return PSVO_OK;
    hipStream_t st = as_stream(stream);
    psvo::launch(k_sample_fused, dim3(div_up(r_hit_cap, kSmpWaves)), dim3(64 * kSmpWaves), 0, st, row_begin, n_rows, r_hit_cap,
                       max_steps_cap, rank_ray, hit_idx, hit_t0, hit_t1, ray_dsum, step_size, noise, seed, stats,
                       s_idx, s_depth, s_dist, ray_ns, nullptr, 0, SampleTail{}, static_cast<const int *>(nullptr),
                       static_cast<const int *>(nullptr));
    psvo::launch(k_scan_samples, dim3(1), dim3(1024), 0, st, row_begin, n_rows, r_hit_cap, ray_ns, offsets,
                       stats, 0, nullptr, 0, SampleCounts{});
    return check_launch("sample_rays");
}

extern "C" int psvo_sample_rays(void *stream, int64_t r_hit_cap, int max_steps_cap, const int *rank_ray,
                                const int *hit_idx, const float *hit_t0, const float *hit_t1, const float *ray_dsum,
                                float step_size, const float *noise, uint64_t seed, int *stats, int *s_idx,
                                float *s_depth, float *s_dist, int *ray_ns, int *offsets) {
    return psvo_sample_rays_range(stream, 0, -1, r_hit_cap, max_steps_cap, rank_ray, hit_idx, hit_t0, hit_t1,
                                  ray_dsum, step_size, noise, seed, stats, s_idx, s_depth, s_dist, ray_ns, offsets);
}

namespace psvo {
// the single-GPU sampler with the statistics read-back fused into its scan
// (one launch less before the host can size the rest of the step)
int sample_rays_to_host(hipStream_t st, int64_t r_hit_cap, int max_steps_cap, const int *rank_ray, const int *hit_idx,
                        const float *hit_t0, const float *hit_t1, const float *ray_dsum, float step_size,
                        const float *noise, uint64_t seed, int *stats, int *s_idx, float *s_depth, float *s_dist,
                        int *ray_ns, int *offsets, unsigned long long *host, int seq, const SampleCounts *counts, unsigned long long *lb_desc, uint32_t lb_tag, int *leaf,
                        float *t, int *ray_of, int *m_out, const int *nv_rank, const int *col0_rank) {
    PSVO_REQUIRE(r_hit_cap > 0 && max_steps_cap > 0 && offsets && ray_ns && host,
                 "sample_rays_to_host: bad arguments");
    PSVO_REQUIRE(!lb_desc || (r_hit_cap <= kLbMaxRays && lb_tag != 0), "sample_rays_to_host: look-back arguments");
    SampleTail tl{};
    if (counts) tl.c = *counts;
    tl.host = host;
    tl.seq = seq;
    if (lb_desc) {  // after the traversal's descriptors (lookback_granules)
        tl.offsets = offsets;
        tl.desc = lb_desc + lb_granules<kLbIsGranules>(div_up(r_hit_cap, kIsWaves));
        tl.tag = lb_tag;
        tl.ctl = lb_ctl(2);
        if (leaf && t && ray_of) {
            tl.leaf = leaf;
            tl.t = t;
            tl.ray_of = ray_of;
            tl.m_out = m_out;
        }
    }
    psvo::launch(k_sample_fused, dim3(div_up(r_hit_cap, kSmpWaves)), dim3(64 * kSmpWaves), 0, st, 0, -1, r_hit_cap, max_steps_cap,
                       rank_ray, hit_idx, hit_t0, hit_t1, ray_dsum, step_size, noise, seed, stats, s_idx, s_depth,
                       s_dist, ray_ns, nullptr, 0, tl, nv_rank, col0_rank);
    if (!lb_desc)
        psvo::launch(k_scan_samples, dim3(1), dim3(1024), 0, st, 0, -1, r_hit_cap, ray_ns, offsets, stats, 0,
                           host, seq, tl.c);
    return check_launch("sample_rays_to_host");
}
// the fused sampler + scan over this rank's rows (stats from dist_layout)
int dist_sample(hipStream_t st, int64_t r_hit_cap, int max_steps_cap, const int *rank_ray, const int *hit_idx,
                const float *hit_t0, const float *hit_t1, const float *ray_dsum, float step_size, uint64_t seed,
                int *stats, const int *table, int nch, int *s_idx, float *s_depth, float *s_dist, int *ray_ns,
                int *offsets, const int *nv_rank, const int *col0_rank) {
    if (r_hit_cap == 0) return PSVO_OK;
    psvo::launch(k_sample_fused, dim3(div_up(r_hit_cap, kSmpWaves)), dim3(64 * kSmpWaves), 0, st, 0, 0, r_hit_cap, max_steps_cap,
                       rank_ray, hit_idx, hit_t0, hit_t1, ray_dsum, step_size, nullptr, seed, stats, s_idx, s_depth,
                       s_dist, ray_ns, table, nch, SampleTail{}, nv_rank, col0_rank);
    psvo::launch(k_scan_samples, dim3(1), dim3(1024), 0, st, 0, 0, r_hit_cap, ray_ns, offsets, stats, 1,
                       nullptr, 0, SampleCounts{});
    return check_launch("dist_sample");
}
// the sampler's helped-block counter (psvo_debug_lb_helps)
int lb_helps_sample(int64_t *out1, bool reset) {
    unsigned long long h = 0;
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpyFromSymbol(&h, HIP_SYMBOL(psvo_g_lb_helps), sizeof(h)) != hipSuccess)
        return set_error(PSVO_E_LAUNCH, "debug_lb_helps: copy failed");
    *out1 = (int64_t)h;
    const unsigned long long z = 0;
    if (reset && hipMemcpyToSymbol(HIP_SYMBOL(psvo_g_lb_helps), &z, sizeof(z)) != hipSuccess)
        return set_error(PSVO_E_LAUNCH, "debug_lb_helps: reset failed");
    return PSVO_OK;
}
}  // namespace psvo

#ifdef PSVO_IS_STAMPS
extern "C" int psvo_debug_smp_stamps(void *dst, int64_t bytes) {
    if (bytes < (int64_t)sizeof(psvo::psvo_g_smp_stamps)) return -1;
    return hipMemcpyFromSymbol(dst, HIP_SYMBOL(psvo::psvo_g_smp_stamps), sizeof(psvo::psvo_g_smp_stamps)) ==
                   hipSuccess
               ? 0
               : -2;
}
#endif

// ---------------------------------------------------------------------------
// The single-workgroup scan of a count array on its own.
namespace psvo {
namespace {

__global__ __launch_bounds__(1024) void k_scan_counts(int64_t n, const int *__restrict__ counts,
                                                      int *__restrict__ offsets) {
    __shared__ int total;
    block_scan_runs(n, [&](int64_t i) { return counts[i]; }, offsets, &total);
    __syncthreads();
    if (threadIdx.x == 0) offsets[n] = total;
}

}  // namespace
}  // namespace psvo

extern "C" int psvo_scan_counts(void *stream, int64_t n, const int *counts, int *offsets) {
    PSVO_REQUIRE(n >= 0, "scan_counts: n < 0");
    psvo::launch(k_scan_counts, dim3(1), dim3(1024), 0, as_stream(stream), n, counts, offsets);
    return check_launch("scan_counts");
}

namespace psvo {
namespace {

// ---------------------------------------------------------------------------
// z_vals / mask [R_hit, S_max] and ray-major compacted samples.
__global__ void k_sample_points(int64_t r_hit, int s_max, int cap, const int *__restrict__ s_idx,
                                const float *__restrict__ s_depth, const int *__restrict__ ray_ns,
                                const int *__restrict__ offsets, int *__restrict__ leaf, float *__restrict__ t,
                                int *__restrict__ ray_of_sample, float *__restrict__ z_vals,
                                uint8_t *__restrict__ mask) {
    // grid rows stride over the hit rays (no 64-bit division per element)
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= s_max) return;
    for (int64_t r = blockIdx.y; r < r_hit; r += gridDim.y) {
        const int64_t e = r * s_max + s;
        // valid samples form a prefix of each row; past it the padding
        // (-1, MAX_DEPTH) is implied — the look-back sampler does not write it
        const bool in = s < offsets[r + 1] - offsets[r];
        const int v = in ? s_idx[r * cap + s] : -1;
        const float z = in ? s_depth[r * cap + s] : kMaxDepthFill;
        z_vals[e] = z;
        mask[e] = v != -1;
        if (v != -1) {
            const int64_t o = offsets[r] + s;
            leaf[o] = v;
            t[o] = z;
            ray_of_sample[o] = (int)r;
        }
    }
}

// Ray-major sample compaction only (the engine's mapping path: the loss
// kernels read z from the sampler's rows, so no padded [R_hit, S_max] copy):
// one wave per hit ray copies the valid prefix of its sampler row to the
// compact arrays — ns ≈ 64 entries, not the S_max-wide row k_sample_points
// walks.
__global__ __launch_bounds__(256) void k_compact_rays(int64_t r_hit, int cap, const int *__restrict__ s_idx,
                                                      const float *__restrict__ s_depth,
                                                      const int *__restrict__ offsets, int *__restrict__ leaf,
                                                      float *__restrict__ t, int *__restrict__ ray_of_sample) {
    const int64_t r = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= r_hit) return;
    const int lane = threadIdx.x & (kWave - 1);
    const int beg = offsets[r], ns = offsets[r + 1] - beg;
    for (int s = lane; s < ns; s += kWave) {
        leaf[beg + s] = s_idx[r * cap + s];
        t[beg + s] = s_depth[r * cap + s];
        ray_of_sample[beg + s] = (int)r;
    }
}

}  // namespace
}  // namespace psvo

extern "C" int psvo_sample_points(void *stream, int64_t r_hit, int s_max, int max_steps_cap, const int *s_idx,
                                  const float *s_depth, const int *ray_ns, const int *offsets, int *leaf, float *t,
                                  int *ray_of_sample, float *z_vals, uint8_t *mask) {
    PSVO_REQUIRE(r_hit >= 0 && s_max >= 0 && s_max <= max_steps_cap, "sample_points: bad sizes");
    const int64_t total = r_hit * (int64_t)s_max;
    if (total == 0) return PSVO_OK;
    (void)ray_ns;
    const int bx = s_max <= 64 ? 64 : s_max <= 128 ? 128 : 256;
    const unsigned gy = (unsigned)(r_hit < 65535 ? r_hit : 65535);
    psvo::launch(k_sample_points, dim3(div_up(s_max, bx), gy), dim3(bx), 0, as_stream(stream), r_hit,
                       s_max, max_steps_cap, s_idx, s_depth, ray_ns, offsets, leaf, t, ray_of_sample, z_vals, mask);
    return check_launch("sample_points");
}

namespace psvo {
int compact_rays(hipStream_t st, int64_t r_hit, int cap, const int *s_idx, const float *s_depth, const int *offsets,
                 int *leaf, float *t, int *ray_of_sample) {
    PSVO_REQUIRE(r_hit >= 0 && cap > 0, "compact_rays: bad sizes");
    if (r_hit == 0) return PSVO_OK;
    psvo::launch(k_compact_rays, dim3(div_up(r_hit, 4)), dim3(256), 0, st, r_hit, cap, s_idx, s_depth, offsets,
                       leaf, t, ray_of_sample);
    return check_launch("compact_rays");
}

}  // namespace psvo
