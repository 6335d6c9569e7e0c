// Ray query on gfx950, data parallel: the three small kernels that build the
// union batch's layout on every rank from two all-gathers.
//
// Reference behaviour restated (DARYL-GWZ/Proud-SLAM):
//   voxel_helpers.py:288-374  sampler host wrapper: G = 200 blocks × K' slots, 800-slot chunks
//   sample_gpu.cu:224-237     the sampler's trailing segment: its two reads of other rows
//
// Integers only; compiled like the other query units (FP contraction off).
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include "query.h"

namespace psvo {
namespace {

// Data-parallel query (engine_query.cpp): each rank samples
// its own hit rays inside the [200, K', P] layout of the union batch (ranks
// in order).  Besides P / R_hit / max ceil(steps) of the union, the sampler
// reads other ranks' rows in two places only (sample_gpu.cu:224-237): whether
// column k of each launch chunk's slot-0 row is a hit (idx_slot0(k) == -1 —
// a row's hits are its prefix, so that is k < the row's hit count) and the
// first voxel id of the row after a ray's own (a ray with exactly P bins).
// So ONE all-gather carries everything: per rank 8 words and the hit count
// of each of its hit rows (a byte each, rank order) — every rank then builds
// the union layout and the [200 · nch] slot-0 count table itself
// (kDistWordsPerRank: query.h).

// this rank's words: thread t packs the hit counts of its hit rows 4t..4t+3
__global__ __launch_bounds__(256) void k_dist_pack(const int *__restrict__ stats, const int *__restrict__ rank_ray,
                                                   const int *__restrict__ hit_idx, const int *__restrict__ ray_nv,
                                                   int *__restrict__ out, const int *__restrict__ nv_rank,
                                                   int flags_or) {
    const int r_hit = stats[PSVO_STAT_R_HIT];
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t == 0) {
        out[0] = r_hit;
        out[1] = stats[PSVO_STAT_P];
        out[2] = stats[PSVO_STAT_MAX_CEIL];
        out[3] = r_hit > 0 ? hit_idx[(int64_t)rank_ray[0] * kMaxHits] : -1;
        // e.g. a DFS-stack overflow on one rank: every rank fails together; and
        // PSVO_FLAG_UNION_UNCOUNTED from a rank whose query had no GT depths
        out[4] = stats[PSVO_STAT_FLAGS] | flags_or;
        for (int k = 5; k < kDistWordsPerRank; ++k) out[k] = 0;
    }
    const int j0 = 4 * t;
    if (j0 >= r_hit) return;
    uint32_t w = 0;
    for (int k = 0; k < 4 && j0 + k < r_hit; ++k)  // nv <= 50
        w |= (uint32_t)(nv_rank ? nv_rank[j0 + k] : ray_nv[rank_ray[j0 + k]]) << (8 * k);
    out[kDistWordsPerRank + t] = (int)w;
}

// union-batch statistics and the slot-0 count table from the gathered words
// (world x stride): table[b · nch + c] = hit count of logical row b·K' + c·800
// (row 0 past the union's end)
__global__ __launch_bounds__(256) void k_dist_layout(const int *__restrict__ all, int world, int rank, int stride,
                                                     int nch, int *__restrict__ stats, int *__restrict__ table,
                                                     int *__restrict__ q2_in) {
    int r_hit = 0;
    for (int r = 0; r < world; ++r) r_hit += all[r * stride];
    // this query's count words start at zero (k_dist_counts adds into them),
    // whatever an earlier query that failed before k_dist_smax left there
    if (q2_in && threadIdx.x >= 1 && threadIdx.x < kDistWordsPerRank) q2_in[threadIdx.x] = 0;
    if (threadIdx.x == 0) {
        int p = 0, mc = 0, begin = 0, flags = 0;
        for (int r = 0; r < world; ++r) {
            const int *w = all + r * stride;
            if (r < rank) begin += w[0];
            p = max(p, w[1]);
            mc = max(mc, w[2]);
            flags |= w[4];
        }
        // the logical row after this rank's last: the next rank holding hit rows,
        // or (past the union's last row) row 0, as the reference's row-0 padding
        int next = -1;
        for (int r = rank + 1; r < world && next < 0; ++r)
            if (all[r * stride] > 0) next = r;
        for (int r = 0; r < world && next < 0; ++r)
            if (all[r * stride] > 0) next = r;
        stats[PSVO_STAT_R_HIT_LOCAL] = all[rank * stride];
        stats[PSVO_STAT_ROW_BEGIN] = begin;
        stats[PSVO_STAT_NEXT_COL0] = next >= 0 ? all[next * stride + 3] : -1;
        stats[PSVO_STAT_P] = p;
        stats[PSVO_STAT_R_HIT] = r_hit;
        stats[PSVO_STAT_MAX_CEIL] = mc;
        stats[PSVO_STAT_FLAGS] |= flags;
    }
    const int kp = (r_hit + kSamplerG - 1) / kSamplerG;
    for (int row = threadIdx.x; row < kSamplerG * nch; row += blockDim.x) {
        const int b = row / nch, c = row - b * nch;
        int lrow = b * kp + c * kSamplerChunk;
        if (lrow >= r_hit) lrow = 0;
        int nv = 0;
        if (r_hit > 0) {
            int o = 0, beg = 0;
            while (lrow >= beg + all[o * stride]) beg += all[o++ * stride];  // the owner: lrow < r_hit
            const int j = lrow - beg;
            nv = (int)(((uint32_t)all[o * stride + kDistWordsPerRank + (j >> 2)] >> (8 * (j & 3))) & 0xffu);
        }
        table[row] = nv;
    }
}

// after the gather of [S_max, count words] (world x 8): the union S_max and,
// given the rank's counts (dist_counts), the union's normaliser sums —
// integers, so any summation order gives the single-GPU doubles; zeroes the
// rank's count words for the next query's atomics
__global__ void k_dist_smax(const int *__restrict__ all, int world, int *__restrict__ stats, int *__restrict__ in,
                            double *__restrict__ sums) {
    if (threadIdx.x != 0) return;
    int mx = 0;
    bool counted = true;  // every rank counted its rows against GT depths (k_dist_counts)
    for (int r = 0; r < world; ++r) {
        const int w0 = all[r * kDistWordsPerRank];
        mx = max(mx, w0 & ~kDistNotCounted);
        counted = counted && !(w0 & kDistNotCounted);
    }
    stats[PSVO_STAT_S_MAX_LOCAL] = stats[PSVO_STAT_S_MAX];
    stats[PSVO_STAT_S_MAX] = mx;
    // the same on every rank: whether the step may take the union's count
    // sums from here or must count (and all-reduce) them itself
    if (!counted) stats[PSVO_STAT_FLAGS] |= PSVO_FLAG_UNION_UNCOUNTED;
    if (sums && counted) {
        long long c[7] = {0, 0, 0, 0, 0, 0, 0};
        for (int r = 0; r < world; ++r)
            for (int k = 0; k < 7; ++k) c[k] += all[r * kDistWordsPerRank + 1 + k];
        // words: n_valid, Σ front, Σ sdf band (valid samples), rays whose padding is front,
        // Σ their ns, rays whose padding is in the band, Σ their ns (dist_counts)
        for (int k = 0; k < 8; ++k) sums[k] = 0.0;
        sums[2] = (double)c[0];                       // kNValid
        sums[3] = (double)(c[1] + mx * c[3] - c[4]);  // kNFront: + (S_max − ns) per padded-front ray
        sums[4] = (double)(c[2] + mx * c[5] - c[6]);  // kNSdf
    }
    for (int k = 1; k < kDistWordsPerRank; ++k) in[k] = 0;
}

}  // namespace

int dist_slot0_rows(int64_t max_rays_global) {
    const int64_t kp = (max_rays_global + kSamplerG - 1) / kSamplerG;
    return kSamplerG * (int)((kp + kSamplerChunk - 1) / kSamplerChunk);
}
int dist_count_words(int max_rays_rank) { return kDistWordsPerRank + (max_rays_rank + 3) / 4; }
int dist_pack(hipStream_t st, int64_t R, const int *stats, const int *rank_ray, const int *hit_idx,
              const int *ray_nv, int *out, const int *nv_rank, int flags_or) {
    psvo::launch(k_dist_pack, dim3((int)div_up(div_up(R, 4), 256) + (R == 0)), dim3(256), 0, st, stats, rank_ray,
                 hit_idx, ray_nv, out, nv_rank, flags_or);
    return check_launch("dist_pack");
}
int dist_layout(hipStream_t st, const int *all, int world, int rank, int stride, int nch, int *stats, int *table,
                int *q2_in) {
    psvo::launch(k_dist_layout, dim3(1), dim3(256), 0, st, all, world, rank, stride, nch, stats, table, q2_in);
    return check_launch("dist_layout");
}
int dist_smax(hipStream_t st, const int *all, int world, int *stats, int *in, double *sums) {
    psvo::launch(k_dist_smax, dim3(1), dim3(64), 0, st, all, world, stats, in, sums);
    return check_launch("dist_smax");
}

}  // namespace psvo
