// Ray / sparse-voxel-octree query on gfx950, first half: DFS intersection,
// stable depth sort and hit-ray ranking with the batch's statistics.
// (query_sample.hip: the sampler; query_dist.hip: the data-parallel layout.)
//
// Reference behaviour restated (DARYL-GWZ/Proud-SLAM):
//   intersect_gpu.cu:75-140   slab AABB test
//   intersect_gpu.cu:191-270  DFS from node 0, children popped 7→0, ≤ n_max leaf hits
//   voxel_helpers.py:557-595  sort by t_in, max_distance trim, P = max valid hits
//
// MI355X design: one lane per ray (rays are independent and divergent); the
// DFS keeps a per-level (node, remaining-children bitmask) stack and the
// ≤50-entry hit list in LDS, laid out [slot][lane] so the 64 lanes of a wave
// hit 64 distinct banks.  Per-launch statistics (P, R_hit, max steps) are
// wave-reduced and published with one atomic per wave, so the host reads
// them back once instead of the reference's sequence of host syncs.
//
// Arithmetic: the traversal is compiled with FP contraction off and IEEE
// division so hit indices reproduce the CPU oracle bit for bit (the
// reference CUDA uses __fdividef and nvcc's default FMA contraction; see
// DESIGN.md "parity").
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include "query.h"
#include "query_common.h"

namespace psvo {
namespace {

__device__ __forceinline__ int child_mask(const int *__restrict__ children, int node) {
    const int *row = children + (int64_t)node * 9;
    int m = 0;
#pragma unroll
    for (int u = 0; u < 8; ++u) m |= (row[u] > -1) ? (1 << u) : 0;
    return m;
}

// DFS of one ray over the flattened octree, emitting ≤ n_max leaf hits in
// the reference order into the LDS-resident list (stride kWave).
// Returns the number of AABB tests; *cnt the number of hits; *overflow if
// the level stack would exceed kLevels.
template <int STRIDE = kWave>
__device__ int dfs_ray(const float o[3], const float d[3], const float *__restrict__ points,
                       const int *__restrict__ children, float half_voxel, int n_max, int *l_node, int *l_mask,
                       int *h_idx, float *h_t0, float *h_t1, int *cnt_out, bool *overflow) {
    float inv[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) inv[a] = __fdiv_rn(1.0f, d[a]);
    int cnt = 0, visits = 0;
    int lvl = -1;
    {
        float t0, t1;
        const int side = children[8];
        ++visits;
        if (ray_aabb(o, inv, points[0], points[1], points[2], half_voxel * (float)side, t0, t1)) {
            if (side == 1) {
                h_idx[0] = 0;
                h_t0[0] = t0;
                h_t1[0] = t1;
                cnt = 1;
            } else {
                lvl = 0;
                l_node[0] = 0;
                l_mask[0] = child_mask(children, 0);
            }
        }
    }
    while (lvl >= 0 && cnt < n_max) {
        int m = l_mask[lvl * STRIDE];
        if (m == 0) {
            --lvl;
            continue;
        }
        const int u = 31 - __clz(m);
        l_mask[lvl * STRIDE] = m & ~(1 << u);
        const int k = children[(int64_t)l_node[lvl * STRIDE] * 9 + u];
        const float *pc = points + (int64_t)k * 3;
        const int side = children[(int64_t)k * 9 + 8];
        float t0, t1;
        ++visits;
        if (!ray_aabb(o, inv, pc[0], pc[1], pc[2], half_voxel * (float)side, t0, t1)) continue;
        if (side == 1) {
            h_idx[cnt * STRIDE] = k;
            h_t0[cnt * STRIDE] = t0;
            h_t1[cnt * STRIDE] = t1;
            ++cnt;
            continue;
        }
        if (lvl + 1 >= kLevels) {
            *overflow = true;
            break;
        }
        ++lvl;
        l_node[lvl * STRIDE] = k;
        l_mask[lvl * STRIDE] = child_mask(children, k);
    }
    *cnt_out = cnt;
    return visits;
}

// ---------------------------------------------------------------------------
// drop-in grid.svo_intersect: [b, m] rays against [b, n] trees.
__global__ __launch_bounds__(64) void k_svo_intersect_raw(int b, int n, int m, float voxelsize, int n_max,
                                                          const float *__restrict__ ray_start,
                                                          const float *__restrict__ ray_dir,
                                                          const float *__restrict__ points,
                                                          const int *__restrict__ children, int *__restrict__ idx,
                                                          float *__restrict__ min_depth,
                                                          float *__restrict__ max_depth) {
    __shared__ int l_node[kLevels * kWave];
    __shared__ int l_mask[kLevels * kWave];
    __shared__ int h_idx[kMaxHits * kWave];
    __shared__ float h_t0[kMaxHits * kWave];
    __shared__ float h_t1[kMaxHits * kWave];
    const int lane = threadIdx.x;
    const int64_t gid = (int64_t)blockIdx.x * kWave + lane;
    if (gid >= (int64_t)b * m) return;
    const int bi = (int)(gid / m);
    const float o[3] = {ray_start[gid * 3 + 0], ray_start[gid * 3 + 1], ray_start[gid * 3 + 2]};
    const float d[3] = {ray_dir[gid * 3 + 0], ray_dir[gid * 3 + 1], ray_dir[gid * 3 + 2]};
    int cnt = 0;
    bool overflow = false;
    const int nm = n_max < kMaxHits ? n_max : kMaxHits;
    dfs_ray(o, d, points + (int64_t)bi * n * 3, children + (int64_t)bi * n * 9, voxelsize * 0.5f, nm,
            l_node + lane, l_mask + lane, h_idx + lane, h_t0 + lane, h_t1 + lane, &cnt, &overflow);
    int *oi = idx + gid * n_max;
    float *omin = min_depth + gid * n_max;
    float *omax = max_depth + gid * n_max;
    for (int l = 0; l < n_max; ++l) {
        const bool v = l < cnt;
        oi[l] = v ? h_idx[l * kWave + lane] : -1;
        omin[l] = v ? h_t0[l * kWave + lane] : 0.0f;
        omax[l] = v ? h_t1[l * kWave + lane] : 0.0f;
    }
}

}  // namespace
}  // namespace psvo

using namespace psvo;

extern "C" int psvo_svo_intersect(void *stream, int b, int n, int m, float voxelsize, int n_max,
                                  const float *ray_start, const float *ray_dir, const float *points,
                                  const int *children, int *idx, float *min_depth, float *max_depth) {
    PSVO_REQUIRE(b >= 0 && n > 0 && m >= 0 && n_max > 0, "svo_intersect: bad sizes b=%d n=%d m=%d n_max=%d", b, n, m,
                 n_max);
    PSVO_REQUIRE(n_max <= kMaxHits, "svo_intersect: n_max=%d exceeds %d", n_max, kMaxHits);
    const int64_t total = (int64_t)b * m;
    if (total == 0) return PSVO_OK;
    psvo::launch(k_svo_intersect_raw, dim3(div_up(total, kWave)), dim3(kWave), 0, as_stream(stream), b, n, m,
                       voxelsize, n_max, ray_start, ray_dir, points, children, idx, min_depth, max_depth);
    return check_launch("svo_intersect");
}

// ---------------------------------------------------------------------------
// The statistics / hit-rank pass as kernels of their own (beyond kLbMaxRays
// rays and on the drop-in path; the engine's traversal below does the same
// work inside its launch) and the statistics' read-back.
namespace psvo {
namespace {

// one wave, one word per lane (words <= 64)
__global__ void k_stats_to_host(int *__restrict__ stats, unsigned long long *host, int words, int seq, int zero) {
    const int i = threadIdx.x;
    if (i < words) {
        const int v = stats[i];
        if (zero) stats[i] = 0;  // ready for the query set's next use (no memset launch)
        stat_to_host(host, i, v, seq);
    }
}

// P (max valid hits), R_hit and max ceil(Σ/step) over the rays — one block.
__device__ void ray_stats_body(int64_t n, const int *__restrict__ ray_nv, const float *__restrict__ ray_dsum,
                               float step_size, int *__restrict__ stats) {
    int p = 0, hits = 0, mc = 0;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
        const int nv = ray_nv[i];
        p = max(p, nv);
        hits += nv > 0;
        if (nv > 0) mc = max(mc, (int)ceilf(__fdiv_rn(ray_dsum[i], step_size)));
    }
    p = wave_max(p);
    hits = wave_sum(hits);
    mc = wave_max(mc);
    __shared__ int sp[16], sh[16], sm[16];
    const int w = threadIdx.x / kWave;
    if ((threadIdx.x & (kWave - 1)) == 0) {
        sp[w] = p;
        sh[w] = hits;
        sm[w] = mc;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < (int)(blockDim.x / kWave); ++k) {
            p = max(p, sp[k]);
            hits += sh[k];
            mc = max(mc, sm[k]);
        }
        stats[PSVO_STAT_P] = p;
        stats[PSVO_STAT_R_HIT] = hits;
        stats[PSVO_STAT_MAX_CEIL] = mc;
    }
}

__global__ __launch_bounds__(1024) void k_ray_stats(int64_t n, const int *__restrict__ ray_nv,
                                                    const float *__restrict__ ray_dsum, float step_size,
                                                    int *__restrict__ stats) {
    ray_stats_body(n, ray_nv, ray_dsum, step_size, stats);
}

__device__ void hit_rank_body(int64_t n, const int *__restrict__ ray_nv, int *__restrict__ ray_rank,
                              int *__restrict__ rank_ray) {
    __shared__ int total;
    block_scan_runs(n, [&](int64_t i) { return ray_nv[i] > 0 ? 1 : 0; }, ray_rank, &total);
    __syncthreads();
    const int tid = threadIdx.x;
    for (int64_t i = tid; i < n; i += blockDim.x) {
        if (ray_nv[i] > 0) {
            rank_ray[ray_rank[i]] = (int)i;
        } else {
            ray_rank[i] = -1;
        }
    }
}

__global__ __launch_bounds__(1024) void k_hit_rank(int64_t n, const int *__restrict__ ray_nv,
                                                   int *__restrict__ ray_rank, int *__restrict__ rank_ray) {
    hit_rank_body(n, ray_nv, ray_rank, rank_ray);
}

// k_ray_stats + k_hit_rank in one launch (the engine's path).  Up to
// kRankPasses·1024 rays every input is read once, in one round of
// independent loads, and held in registers: ray i = k·1024 + t is thread t's
// pass k, its rank among the hit rays = the hit rays of the earlier passes +
// of the earlier waves of this pass (ballot counts in LDS, one scan) + the
// lower lanes (mbcnt).  The serial version (more rays) read ray_nv three
// times behind three barriers — dependent memory round trips on the
// critical path between the traversal and the sampler.
constexpr int kRankPasses = 8;

__global__ __launch_bounds__(1024) void k_ray_stats_rank(int64_t n, const int *__restrict__ ray_nv,
                                                         const float *__restrict__ ray_dsum, float step_size,
                                                         int *__restrict__ stats, int *__restrict__ ray_rank,
                                                         int *__restrict__ rank_ray, const int *__restrict__ blk_out,
                                                         int n_blk) {
    const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid / kWave;
    if (n <= (int64_t)kRankPasses * 1024 && n_blk <= 2048) {
        __shared__ int s_cnt[kRankPasses * 16];
        __shared__ int s_red[5][16];
        int nv[kRankPasses];
        float ds[kRankPasses];
        int v_blk = 0, r_blk = 0;
        if (blk_out) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int b = j * 1024 + tid;
                if (b < n_blk) {
                    v_blk += blk_out[2 * b];
                    r_blk += blk_out[2 * b + 1];
                }
            }
        }
#pragma unroll
        for (int k = 0; k < kRankPasses; ++k) {
            const int64_t i = (int64_t)k * 1024 + tid;
            nv[k] = i < n ? ray_nv[i] : 0;
            ds[k] = i < n ? ray_dsum[i] : 0.f;
        }
        int p = 0, mc = 0;
#pragma unroll
        for (int k = 0; k < kRankPasses; ++k) {
            p = max(p, nv[k]);
            if (nv[k] > 0) mc = max(mc, (int)ceilf(__fdiv_rn(ds[k], step_size)));
            const uint64_t m = __ballot(nv[k] > 0);
            if (lane == 0) s_cnt[k * 16 + w] = __popcll(m);
        }
        p = wave_max(p);
        mc = wave_max(mc);
        const int vs = wave_sum(v_blk), rs = wave_sum(r_blk);
        if (lane == 0) {
            s_red[0][w] = p;
            s_red[1][w] = mc;
            s_red[2][w] = vs;
            s_red[3][w] = rs;
        }
        __syncthreads();
        const int nw = blockDim.x / kWave;
        if (w == 0) {  // exclusive scan of the (pass, wave) hit counts, two per lane
            const int a0 = (lane * 2) / 16 < kRankPasses && (lane * 2) % 16 < nw ? s_cnt[lane * 2] : 0;
            const int a1 = (lane * 2 + 1) / 16 < kRankPasses && (lane * 2 + 1) % 16 < nw ? s_cnt[lane * 2 + 1] : 0;
            int incl = a0 + a1;
#pragma unroll
            for (int sh = 1; sh < kWave; sh <<= 1) {
                const int t = __shfl_up(incl, sh, kWave);
                if (lane >= sh) incl += t;
            }
            if (lane * 2 < kRankPasses * 16) {
                s_cnt[lane * 2] = incl - a0 - a1;
                s_cnt[lane * 2 + 1] = incl - a1;
            }
            if (lane == kWave - 1) s_red[4][0] = incl;  // hit rays
        }
        __syncthreads();
        if (tid == 0) {
            int pp = 0, mm = 0, vv = 0, rr = 0;
            for (int k = 0; k < nw; ++k) {
                pp = max(pp, s_red[0][k]);
                mm = max(mm, s_red[1][k]);
                vv += s_red[2][k];
                rr += s_red[3][k];
            }
            stats[PSVO_STAT_P] = pp;
            stats[PSVO_STAT_R_HIT] = s_red[4][0];
            stats[PSVO_STAT_MAX_CEIL] = mm;
            if (blk_out) {
                atomicAdd(stats + PSVO_STAT_VISITS, vv);
                atomicAdd(stats + PSVO_STAT_ROUNDS, rr);
            }
        }
#pragma unroll
        for (int k = 0; k < kRankPasses; ++k) {
            const int64_t i = (int64_t)k * 1024 + tid;
            const uint64_t m = __ballot(nv[k] > 0);
            if (i < n) {
                const int rk = s_cnt[k * 16 + w] +
                               (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                                              __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                ray_rank[i] = nv[k] > 0 ? rk : -1;
                if (nv[k] > 0) rank_ray[rk] = (int)i;
            }
        }
        return;
    }
    if (blk_out) {  // the intersect blocks' AABB tests / traversal rounds
        int v = 0, rd = 0;
        for (int i = threadIdx.x; i < n_blk; i += blockDim.x) {
            v += blk_out[2 * i];
            rd += blk_out[2 * i + 1];
        }
        v = wave_sum(v);
        rd = wave_sum(rd);
        if ((threadIdx.x & (kWave - 1)) == 0) {
            atomicAdd(stats + PSVO_STAT_VISITS, v);  // 16 waves: 16 atomics
            atomicAdd(stats + PSVO_STAT_ROUNDS, rd);
        }
    }
    ray_stats_body(n, ray_nv, ray_dsum, step_size, stats);
    __syncthreads();
    hit_rank_body(n, ray_nv, ray_rank, rank_ray);
}

}  // namespace

int stats_to_host(hipStream_t st, int *stats, unsigned long long *host, int words, int seq, bool zero) {
    psvo::launch(k_stats_to_host, dim3(1), dim3(64), 0, st, stats, host, words, seq, zero ? 1 : 0);
    return check_launch("stats_to_host");
}
}  // namespace psvo

extern "C" int psvo_ray_stats(void *stream, int64_t n_rays, const int *ray_nv, const float *ray_dsum,
                              float step_size, int *stats) {
    PSVO_REQUIRE(n_rays >= 0 && step_size > 0.0f, "ray_stats: bad arguments");
    if (n_rays == 0) return PSVO_OK;
    psvo::launch(k_ray_stats, dim3(1), dim3(1024), 0, as_stream(stream), n_rays, ray_nv, ray_dsum, step_size,
                       stats);
    return check_launch("ray_stats");
}

extern "C" int psvo_hit_rank(void *stream, int64_t n_rays, const int *ray_nv, int *ray_rank, int *rank_ray) {
    PSVO_REQUIRE(n_rays >= 0, "hit_rank: n_rays < 0");
    if (n_rays == 0) return PSVO_OK;
    psvo::launch(k_hit_rank, dim3(1), dim3(1024), 0, as_stream(stream), n_rays, ray_nv, ray_rank, rank_ray);
    return check_launch("hit_rank");
}

namespace psvo {
namespace {

// ---------------------------------------------------------------------------
// fused ray_intersect_vox: octree query → stable sort by t_in → max_distance
// trim, plus per-ray Σ(t_out - t_in) for the sampler's probs / steps.
//
// One wave per ray, KEY-ORDERED CHUNKED traversal instead of one-node-at-a-
// time DFS.  Every node has a path key Σ_d (7 − u_d)·8^(16−d); the
// reference's depth-first emission order (children popped 7→0,
// intersect_gpu.cu:191-270) is ascending key order, and the first n_max = 50
// leaves it emits are the 50 smallest leaf keys.  The wave keeps an LDS stack
// of untested candidates sorted by key (smallest on top) and each round pops
// up to 64 of them — one per lane — and tests them together: one dependent
// memory round trip per round (the candidate's centre and its whole
// structure row, children included, are independent loads), instead of one
// per AABB test.  Hit internal nodes push their existing children (keys
// ascending toward the top, so every child precedes every remaining
// candidate: preorder keys).  Once 50 leaves are known the 50th key bounds
// the search and every candidate beyond it is dropped (the DFS would never
// have reached it).  The stable sort by t_in breaks ties by key = DFS order.
// A round whose children would overflow the stack re-queues its tail lanes;
// a ray that cannot progress at all, or a tree deeper than the reference's
// 16-level stack, falls back to the serial DFS on lane 0 (same results,
// counted in stats[PSVO_STAT_SPILLS]).
constexpr int kStk = 512;    // candidate stack entries per ray
constexpr int kBfsL = 128;   // leaf list capacity (≤ 49 + 64 between compactions)
// the packed walk's two-chunk rounds (trace_pass TWO): for deep trees only —
// config E's traversal 73 → 67 µs, room0's +0.7 µs (profiles/r06_ab_two_chunk.txt)
constexpr int64_t kTwoChunkNodes = 1 << 18;

#ifdef PSVO_IS_STAMPS  // the diagnostic build's per-ray segment cycles (query_common.h IS_*)
constexpr int kIsStampRays = 16384;
__device__ unsigned long long psvo_g_is_stamps[kIsStampRays][8];
#endif

struct KeyLds {
    uint64_t skey[kStk];
    int snode[kStk];
    uint8_t sdep[kStk];
    uint64_t lkey[kBfsL];
    int lidx[kBfsL];
    float lt0[kBfsL], lt1[kBfsL];
    float hd[kMaxHits];  // t_out - t_in in sorted order
    int dfs_node[kLevels], dfs_mask[kLevels];
};

__device__ __forceinline__ uint64_t key_digit(int u, int depth) {
    return (uint64_t)(7 - u) << (3 * (kLevels - depth));
}

// inclusive prefix sum over the wave of v in [0, 16) (a node's child count):
// one ballot + lane-mask count per bit instead of six dependent cross-lane
// shuffles
__device__ __forceinline__ int wave_incl_scan16(int v) {
    int s = v;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const uint64_t m = __ballot((v >> b) & 1);
        s += (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)) << b;
    }
    return s;
}

// number of keys below k in the ascending list a[0, n), n <= 64: a
// branch-free binary search of 7 uniform steps (the leaf list is kept sorted
// by merging each round's leaves into it, so the prune's threshold — the 50th
// smallest key — is simply its last entry; no per-round selection)
__device__ __forceinline__ int count_below(const uint64_t *a, int n, uint64_t k) {
    int lo = 0;
#pragma unroll
    for (int step = kWave; step > 0; step >>= 1)
        if (lo + step <= n && a[lo + step - 1] < k) lo += step;
    return lo;
}


// The packed traversal's start below the root.  Every ray descends the same
// few top levels one round each (room0: 9 rounds per ray, one per level), so
// the records above the start level m (records [0, n_top), breadth-first,
// n_top <= 128; tree_pack.hip stores n_top and m in the root's spare word and
// the parent record in the others') are tested all at once — one round of
// independent loads — and "hit with every ancestor" is resolved by pointer
// jumping over the parent links (cross-lane, no LDS passes).  A node is
// tested by the reference's walk iff its parent passed (PSVO_STAT_VISITS
// counts exactly those).  The children of the passing level-(m−1) records
// are the level-m candidates, pushed in record order (within a level,
// breadth-first order is descending key order), the smallest key on top —
// the state the rounds would have reached, minus their latency.  The top
// levels hold no leaves (tree_pack.hip checks), so no prune can have applied.
// Returns the stack depth, or −1 (more than kStk candidates: the caller
// starts at the root).
__device__ int top_start(KeyLds &S, const PackRec *__restrict__ packed, const float o[3], const float inv[3],
                         float half, int n_top, int m, int lane, int &visits) {
    constexpr int kB = kPackTopMax / kWave;  // n_top <= kPackTopMax
    bool pa[kB];           // hit, then: hit and every ancestor hit
    int anc[kB], par[kB], first[kB], cmask[kB];
#pragma unroll
    for (int b = 0; b < kB; ++b) {
        const int j = b * kWave + lane;
        pa[b] = false;
        anc[b] = par[b] = -1;
        first[b] = -1;
        cmask[b] = 0;
        if (j < n_top) {
            const float4 pc = packed[j].c;
            const int4 pi = packed[j].i;
            float a = 0.f, t = 0.f;
            pa[b] = ray_aabb_nb(o, inv, pc.x, pc.y, pc.z, half * (float)__float_as_int(pc.w), a, t);
            par[b] = anc[b] = j == 0 ? -1 : pi.w;
            first[b] = pi.y;
            cmask[b] = pi.z;
        }
    }
    // pointer jumping: pa[j] = AND of the hits from j up to (excluding) anc[j]
    for (;;) {
        bool more = false;
#pragma unroll
        for (int b = 0; b < kB; ++b) more = more || anc[b] >= 0;
        if (!__ballot(more)) break;
        int wd[kB];
#pragma unroll
        for (int b = 0; b < kB; ++b) wd[b] = (anc[b] & 0x3FF) | (pa[b] ? 0x400 : 0);  // anc -1 → 0x3FF
        bool npa[kB];
        int nanc[kB];
#pragma unroll
        for (int b = 0; b < kB; ++b) {
            const int a = anc[b];
            int w = 0;
#pragma unroll
            for (int sb = 0; sb < kB; ++sb) {
                const int v = __shfl(wd[sb], a & (kWave - 1), kWave);
                if ((a >> 6) == sb) w = v;
            }
            npa[b] = a >= 0 ? (pa[b] && (w & 0x400)) : pa[b];
            nanc[b] = a >= 0 ? ((w & 0x3FF) == 0x3FF ? -1 : (w & 0x3FF)) : -1;
        }
#pragma unroll
        for (int b = 0; b < kB; ++b) {
            pa[b] = npa[b];
            anc[b] = nanc[b];
        }
    }
    // tested by the reference's walk: the root, and every node whose parent passed
    int tested = 0;
#pragma unroll
    for (int b = 0; b < kB; ++b) {
        const int p = par[b];
        bool parent_ok = false;
#pragma unroll
        for (int sb = 0; sb < kB; ++sb) {
            const int v = __shfl((int)pa[sb], p & (kWave - 1), kWave);
            if ((p >> 6) == sb) parent_ok = v != 0;
        }
        tested += (b * kWave + lane < n_top) && (b * kWave + lane == 0 || (p >= 0 && parent_ok)) ? 1 : 0;
    }
    // the level-m candidates: children of the passing level-(m-1) records
    // (those whose children lie past the top records), in record order.
    // Their keys: the candidate's rank in descending record order (= key
    // order within a level) in the level-m digit positions — the same order
    // as the path keys for every key this ray ever compares.
    int cnt[kB];
    int total = 0;
#pragma unroll
    for (int b = 0; b < kB; ++b) {
        cnt[b] = (pa[b] && first[b] >= n_top) ? __popc(cmask[b]) : 0;
        total += cnt[b];
    }
    total = wave_sum(total);
    if (total > kStk) return -1;
    const int shift = 3 * (kLevels - m);
    int run = 0;
#pragma unroll
    for (int b = 0; b < kB; ++b) {
        const int incl = wave_incl_scan16(cnt[b]);
        if (cnt[b]) {
            int g = run + incl - cnt[b];
            for (int k = 0; k < cnt[b]; ++k, ++g) {
                S.skey[g] = (uint64_t)(total - 1 - g) << shift;
                S.snode[g] = first[b] + k;
                S.sdep[g] = (uint8_t)m;
            }
        }
        run += __builtin_amdgcn_readlane(incl, kWave - 1);
    }
    visits += tested;
    return total;
}

// look-back blocks this unit's launches helped (lookback.h: a predecessor
// that had not started) — diagnostic, read by lb_helps_trace
__device__ unsigned long long psvo_g_lb_helps;

// PACKED: candidates are records of the breadth-first packed tree
// (tree_pack.hip: centre + side and ref id / first child / child mask in one
// 32-B record, siblings contiguous) instead of reference node ids into the
// two AoS rows; the same floats, the same keys, the reference ids emitted.
// The per-ray work of k_intersect_sorted for the rays of block `cur` (one
// wave per ray): hit rows, ray_nv / ray_dsum, and the wave's totals in L.
// Inlined for the workgroup's own block; the look-back's help path calls
// trace_pass_help (not inlined: the own pass keeps its registers).
struct IsLds {
    int vis[kIsWaves], ov[kIsWaves], sp[kIsWaves], rd[kIsWaves], nv[kIsWaves], mc[kIsWaves], c0[kIsWaves];
};
template <bool PACKED, bool TWO = false>
__device__ __forceinline__ void trace_pass(int cur, int64_t n_rays, const float *__restrict__ rays_o,
                                           const float *__restrict__ rays_d, const float *__restrict__ centres,
                                           const int *__restrict__ structure, const PackRec *__restrict__ packed,
                                           float half, float max_distance, float step_size, int *__restrict__ hit_idx,
                                           float *__restrict__ hit_t0, float *__restrict__ hit_t1,
                                           int *__restrict__ ray_nv, float *__restrict__ ray_dsum, KeyLds &S,
                                           IsLds &L) {
    const int lane = threadIdx.x & (kWave - 1);
    const uint64_t below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    const int64_t r = (int64_t)cur * kIsWaves + threadIdx.x / kWave;
    int visits = 0, rounds = 0;
    int w_nv = 0, w_mc = 0, w_c0 = -1;  // this wave's ray: valid hits, ⌈Σ/step⌉ (lane 0), first hit's id
    bool overflow_stack = false, spill = false;
    if (r < n_rays) {
        IS_DECL;
        IS_MARK(is_t0);
        const float o[3] = {rays_o[r * 3 + 0], rays_o[r * 3 + 1], rays_o[r * 3 + 2]};
        const float d[3] = {rays_d[r * 3 + 0], rays_d[r * 3 + 1], rays_d[r * 3 + 2]};
        float inv[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) inv[a] = __fdiv_rn(1.0f, d[a]);
        int nl = 0, sp = -1;
        bool bounded = false;
        uint64_t kbound = ~0ull;
        if constexpr (PACKED) {
            const int tw = packed[0].i.w;  // records above the start level | start level << 16 (0: none)
            if (tw > 0) sp = top_start(S, packed, o, inv, half, tw & 0xFFFF, tw >> 16, lane, visits);
        }
        if (sp < 0) {
            if (lane == 0) {  // the root is the first candidate
                S.skey[0] = 0;
                S.snode[0] = 0;
                S.sdep[0] = 0;
            }
            sp = 1;
        }
        wave_lds_sync();
        // merge one group's fresh leaves (keys ascending with the lane) into
        // the key-sorted list
        auto merge_leaves = [&](bool fresh, uint64_t key, int ref, float a, float b) {
            const uint64_t lb = __ballot(fresh);
            if (lb) {
                const int m = __popcll(lb), q = __popcll(lb & below);
                if (fresh) S.lkey[kWave + q] = key;  // scratch past the list (nl <= 50)
                const bool hold = lane < nl;
                uint64_t hk = 0;
                int hi = 0;
                float h0 = 0.f, h1 = 0.f;
                if (hold) {
                    hk = S.lkey[lane];
                    hi = S.lidx[lane];
                    h0 = S.lt0[lane];
                    h1 = S.lt1[lane];
                }
                wave_lds_sync();
                // final positions: own rank + the other list's keys below (keys are unique)
                const int pn = q + count_below(S.lkey, nl, key);
                const int po = lane + count_below(S.lkey + kWave, m, hk);
                wave_lds_sync();
                if (fresh && pn < kMaxHits) {
                    S.lkey[pn] = key;
                    S.lidx[pn] = ref;
                    S.lt0[pn] = a;
                    S.lt1[pn] = b;
                }
                if (hold && po < kMaxHits) {
                    S.lkey[po] = hk;
                    S.lidx[po] = hi;
                    S.lt0[po] = h0;
                    S.lt1[po] = h1;
                }
                nl = min(nl + m, kMaxHits);
                wave_lds_sync();
                if (nl == kMaxHits) {  // the 50 smallest keys kept; later candidates beyond them are dropped
                    kbound = S.lkey[kMaxHits - 1];
                    bounded = true;
                }
#ifdef PSVO_IS_STAMPS
                ++is_lr;
#endif
            } else {
                wave_lds_sync();
            }
        };
        while (sp > 0) {  // wave-uniform trip count
            ++rounds;
            IS_MARK(is_ta);
            const int n = min(sp, kWave);
            // PACKED: a full top chunk brings the next 64 entries along (group
            // B, one more record load in flight per lane); they are processed
            // in this round when every entry of both chunks is live and the
            // stack holds all their children — the heavy rays of a deep tree
            // (config E: up to ≈ 1,500 AABB tests) then walk half the rounds.
            // B's keys exceed A's and no B entry descends from an A entry, so
            // A's children stay above B's on the stack (key order); otherwise
            // B stays where it is, untouched (only read), for later rounds.
            const int nB = (PACKED && TWO) ? min(max(sp - kWave, 0), kWave) : 0;
            uint64_t key = 0, keyB = 0;
            int node = 0, dep = 0, nodeB = 0, depB = 0;
            if (lane < n) {
                const int e = sp - 1 - lane;
                key = S.skey[e];
                node = S.snode[e];
                dep = S.sdep[e];
            }
            if (lane < nB) {
                const int e = sp - 1 - kWave - lane;
                keyB = S.skey[e];
                nodeB = S.snode[e];
                depB = S.sdep[e];
            }
            // popped keys ascend with the lane: the live lanes are a prefix
            const bool live = lane < n && !(bounded && key > kbound);
            const int n_eff = __popcll(__ballot(live));
            const bool liveB = lane < nB && !(bounded && keyB > kbound);
            const bool two = nB > 0 && n_eff == kWave && __popcll(__ballot(liveB)) == nB;
            int row[8];
            int side = 0, first = 0, cmask = 0, ref = node;
            int sideB = 0, firstB = 0, cmaskB = 0, refB = nodeB;
            float a = 0.f, b = 0.f, aB = 0.f, bB = 0.f;
            bool hit = false, hitB = false;
            if (live) {
                if constexpr (PACKED) {
                    const float4 pc = packed[node].c;
                    const int4 pi = packed[node].i;
                    float4 pcB = make_float4(0.f, 0.f, 0.f, 0.f);
                    int4 piB = make_int4(0, 0, 0, 0);
                    if (two && liveB) {
                        pcB = packed[nodeB].c;
                        piB = packed[nodeB].i;
                    }
                    side = __float_as_int(pc.w);
                    ref = pi.x;
                    first = pi.y;
                    cmask = pi.z;
                    hit = ray_aabb_nb(o, inv, pc.x, pc.y, pc.z, half * (float)side, a, b);
                    if (two && liveB) {
                        sideB = __float_as_int(pcB.w);
                        refB = piB.x;
                        firstB = piB.y;
                        cmaskB = piB.z;
                        hitB = ray_aabb_nb(o, inv, pcB.x, pcB.y, pcB.z, half * (float)sideB, aB, bB);
                    }
                } else {
                    const int *rw = structure + (int64_t)node * 9;
#pragma unroll
                    for (int u = 0; u < 8; ++u) row[u] = rw[u];
                    side = rw[8];
                    const float *pc = centres + (int64_t)node * 3;
                    hit = ray_aabb_nb(o, inv, pc[0], pc[1], pc[2], half * (float)side, a, b);
                }
            }
            IS_MARK(is_tb);
            IS_ADD(1, is_ta, is_tb);
            const bool leaf = hit && side == 1;
            const bool inner = hit && side != 1;
            const bool leafB = hitB && sideB == 1;
            const bool innerB = hitB && sideB != 1;
            if (__ballot((inner && dep >= kLevels) || (innerB && depB >= kLevels))) {  // deeper than the reference's stack
                spill = true;
                break;
            }
            int c = 0, cB = 0;
            if (inner) {
                if constexpr (PACKED) {
                    c = __popc(cmask);
                } else {
#pragma unroll
                    for (int u = 0; u < 8; ++u) c += row[u] > -1;
                }
            }
            if (innerB) cB = __popc(cmaskB);
            const int incl = wave_incl_scan16(c);
            if (two) {
                const int inclB = wave_incl_scan16(cB);
                const int TA = __builtin_amdgcn_readlane(incl, kWave - 1);
                const int TB = __builtin_amdgcn_readlane(inclB, kWave - 1);
                const int floorB = sp - kWave - nB;
                if (floorB + TA + TB <= kStk) {  // (wave-uniform) both chunks accepted
                    wave_lds_sync();  // every lane has read its candidates before the stack is rewritten
                    // B's children, then A's on top, each in reverse key order
                    if (innerB) {
                        int g = inclB - cB;
                        const int cd = depB + 1;
#pragma unroll
                        for (int u = 7; u >= 0; --u) {
                            if ((cmaskB >> u) & 1) {
                                const int pos = floorB + (TB - 1 - g);
                                S.skey[pos] = keyB | key_digit(u, cd);
                                S.snode[pos] = firstB + __popc(cmaskB & ((1 << u) - 1));
                                S.sdep[pos] = (uint8_t)cd;
                                ++g;
                            }
                        }
                    }
                    if (inner) {
                        int g = incl - c;
                        const int cd = dep + 1;
#pragma unroll
                        for (int u = 7; u >= 0; --u) {
                            if ((cmask >> u) & 1) {
                                const int pos = floorB + TB + (TA - 1 - g);
                                S.skey[pos] = key | key_digit(u, cd);
                                S.snode[pos] = first + __popc(cmask & ((1 << u) - 1));
                                S.sdep[pos] = (uint8_t)cd;
                                ++g;
                            }
                        }
                    }
                    IS_MARK(is_ta);
                    IS_ADD(2, is_tb, is_ta);
                    visits += 1 + (liveB ? 1 : 0);
                    sp = floorB + TA + TB;
                    merge_leaves(leaf, key, ref, a, b);
                    merge_leaves(leafB, keyB, refB, aB, bB);
                    IS_MARK(is_tb);
                    IS_ADD(3, is_ta, is_tb);
                    continue;
                }
            }
            // a prune drops everything below the popped chunk (all keys > kbound)
            const int floor_ = (n_eff < n) ? 0 : sp - n;
            const bool ok = !live || floor_ + (n_eff - 1 - lane) + incl <= kStk;
            const uint64_t bad = __ballot(!ok);
            const int J = bad ? (int)__ffsll((unsigned long long)bad) - 1 : n_eff;  // accepted lanes [0, J)
            if (J == 0 && n_eff > 0) {
                spill = true;
                break;
            }
            const int T = J > 0 ? __builtin_amdgcn_readlane(incl, J - 1) : 0;
            const bool acc = lane < J;
            wave_lds_sync();  // every lane has read its candidate before the stack is rewritten
            if (live && !acc) {  // re-queued tail keeps its order on top of the floor
                const int pos = floor_ + (n_eff - 1 - lane);
                S.skey[pos] = key;
                S.snode[pos] = node;
                S.sdep[pos] = (uint8_t)dep;
            }
            const int base = floor_ + (n_eff - J);
            if (acc && inner) {
                int g = incl - c;  // rank of this lane's first (smallest-key) child
                const int cd = dep + 1;
#pragma unroll
                for (int u = 7; u >= 0; --u) {
                    const bool present = PACKED ? ((cmask >> u) & 1) != 0 : row[u] > -1;
                    if (present) {
                        const int pos = base + (T - 1 - g);
                        S.skey[pos] = key | key_digit(u, cd);
                        S.snode[pos] = PACKED ? first + __popc(cmask & ((1 << u) - 1)) : row[u];
                        S.sdep[pos] = (uint8_t)cd;
                        ++g;
                    }
                }
            }
            IS_MARK(is_ta);
            IS_ADD(2, is_tb, is_ta);
            visits += acc ? 1 : 0;
            sp = base + T;
            merge_leaves(acc && leaf, key, ref, a, b);
            IS_MARK(is_tb);
            IS_ADD(3, is_ta, is_tb);
        }
        if (spill) {  // serial DFS on lane 0 (reference order by construction; key = emission index)
            int cnt = 0;
            bool ov = false;
            if (lane == 0) {
                visits += dfs_ray<1>(o, d, centres, structure, half, kMaxHits, S.dfs_node, S.dfs_mask, S.lidx, S.lt0,
                                     S.lt1, &cnt, &ov);
                for (int i = 0; i < cnt; ++i) S.lkey[i] = (uint64_t)i;
            }
            cnt = __shfl(cnt, 0, kWave);
            overflow_stack = overflow_stack || __shfl((int)ov, 0, kWave);
            nl = cnt;
            wave_lds_sync();
        }
        IS_MARK(is_ta);
        // stable sort by t_in (ties: DFS order = key = list order, both paths
        // leave the list key-sorted), trim at max_distance; nl <= 50: one
        // entry per lane, the others' t_in read lane to lane
        int nv = 0;
        const float ti = lane < nl ? S.lt0[lane] : 0.f;
        int rank = 0;
        for (int j = 0; j < nl; ++j) {
            const float tj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ti), j));
            rank += (tj < ti) || (tj == ti && j < lane);
        }
        if (lane < nl) {
            const bool in = !(ti > max_distance);
            nv += in;
            const float bi = S.lt1[lane];
            S.hd[rank] = bi - ti;
            if (in) {
                hit_idx[r * kMaxHits + rank] = S.lidx[lane];
                hit_t0[r * kMaxHits + rank] = ti;
                hit_t1[r * kMaxHits + rank] = bi;
            }
        }
        nv = wave_sum(nv);
        {  // the first (nearest) hit's voxel id, for the sampler's by-rank copy
            const uint64_t m0 = __ballot(lane < nl && rank == 0 && !(ti > max_distance));
            const int c0 = __builtin_amdgcn_readlane(lane < nl ? S.lidx[lane] : -1, m0 ? __ffsll((unsigned long long)m0) - 1 : 0);
            w_c0 = m0 ? c0 : -1;
        }
        for (int l = nv + lane; l < kMaxHits; l += kWave) {
            hit_idx[r * kMaxHits + l] = -1;
            hit_t0[r * kMaxHits + l] = max_distance;
            hit_t1[r * kMaxHits + l] = max_distance;
        }
        wave_lds_sync();
        if (lane == 0) {
            float dsum = 0.0f;
            for (int l = 0; l < nv; ++l) dsum = dsum + S.hd[l];
            ray_nv[r] = nv;
            ray_dsum[r] = dsum;
            w_nv = nv;
            w_mc = nv > 0 ? (int)ceilf(__fdiv_rn(dsum, step_size)) : 0;  // k_ray_stats' arithmetic
        }
#ifdef PSVO_IS_STAMPS
        IS_MARK(is_tb);
        IS_ADD(4, is_ta, is_tb);
        const int is_vis = wave_sum(visits);
        if (lane == 0 && r < kIsStampRays) {
            psvo_g_is_stamps[r][0] = is_tb - is_t0;
            for (int k = 1; k < 5; ++k) psvo_g_is_stamps[r][k] = is_acc[k];
            psvo_g_is_stamps[r][5] = (unsigned long long)rounds;
            psvo_g_is_stamps[r][6] = is_lr;
            psvo_g_is_stamps[r][7] = (unsigned long long)is_vis;
        }
#endif
    }
    // visits / overflow: one atomic per block (per-ray P, R_hit and max ceil
    // are reduced by k_ray_stats: thousands of same-address atomics serialise
    // at the memory side)
    const int wvis = wave_sum(visits);
    const int wov = wave_max(overflow_stack ? 1 : 0);
    if (lane == 0) {
        L.vis[threadIdx.x / kWave] = wvis;
        L.ov[threadIdx.x / kWave] = wov;
        L.sp[threadIdx.x / kWave] = spill ? 1 : 0;
        L.rd[threadIdx.x / kWave] = rounds;  // wave-uniform
        L.nv[threadIdx.x / kWave] = w_nv;
        L.mc[threadIdx.x / kWave] = w_mc;
        L.c0[threadIdx.x / kWave] = w_c0;
    }
}

// A helped block's per-ray values for its aggregate (lookback.h: a
// predecessor that has not started), one wave per ray: the hits by the
// serial DFS (dfs_ray: the reference's emission order — the 50 smallest DFS
// keys the wave traversal keeps), then the same stable (t_in, DFS order)
// ranks, max_distance trim and left-to-right Σ(t_out − t_in) as trace_pass,
// so the hit count and ⌈Σ/step⌉ are the same bits; the AABB-test count is
// the DFS's (a statistic) and no rounds.  Nothing is written to the hit
// rows: the block's owner writes them when it runs.  Small on purpose — a
// second copy of the wave traversal here cost the own pass 3 µs.
__device__ __forceinline__ void help_trace_pass(int cur, int64_t n_rays, const float *rays_o, const float *rays_d,
                                             const float *centres, const int *structure, float half,
                                             float max_distance, float step_size, KeyLds &S, IsLds &L) {
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    const int64_t r = (int64_t)cur * kIsWaves + w;
    int nv = 0, mc = 0, visits = 0;
    if (r < n_rays) {
        const float o[3] = {rays_o[r * 3 + 0], rays_o[r * 3 + 1], rays_o[r * 3 + 2]};
        const float d[3] = {rays_d[r * 3 + 0], rays_d[r * 3 + 1], rays_d[r * 3 + 2]};
        int cnt = 0;
        bool ov = false;
        if (lane == 0)
            visits = dfs_ray<1>(o, d, centres, structure, half, kMaxHits, S.dfs_node, S.dfs_mask, S.lidx, S.lt0,
                                S.lt1, &cnt, &ov);
        cnt = __shfl(cnt, 0, kWave);
        visits = __shfl(visits, 0, kWave);
        wave_lds_sync();
        const float ti = lane < cnt ? S.lt0[lane] : 0.f;
        int rank = 0;
        for (int j = 0; j < cnt; ++j) {
            const float tj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ti), j));
            rank += (tj < ti) || (tj == ti && j < lane);
        }
        if (lane < cnt) S.hd[rank] = S.lt1[lane] - ti;
        nv = wave_sum(lane < cnt && !(ti > max_distance) ? 1 : 0);
        wave_lds_sync();
        if (lane == 0) {
            float dsum = 0.0f;
            for (int l = 0; l < nv; ++l) dsum = dsum + S.hd[l];
            mc = nv > 0 ? (int)ceilf(__fdiv_rn(dsum, step_size)) : 0;
        }
        mc = __shfl(mc, 0, kWave);
        wave_lds_sync();
    }
    if (lane == 0) {
        L.vis[w] = visits;
        L.rd[w] = 0;
        L.nv[w] = nv;
        L.mc[w] = mc;
    }
}

// wave 0: a block's aggregate {hit rays, P, max ⌈Σ/step⌉, AABB tests, rounds}
__device__ __forceinline__ void trace_agg(const IsLds &L, uint32_t (&agg)[5], uint64_t &hm) {
    const int lane = threadIdx.x & (kWave - 1);
    hm = __ballot(lane < kIsWaves && L.nv[lane] > 0);
    agg[0] = (uint32_t)__popcll(hm);
    agg[1] = agg[2] = agg[3] = agg[4] = 0u;
#pragma unroll
    for (int w = 0; w < kIsWaves; ++w) {
        agg[1] = max(agg[1], (uint32_t)L.nv[w]);
        agg[2] = max(agg[2], (uint32_t)L.mc[w]);
        agg[3] += (uint32_t)L.vis[w];
        agg[4] += (uint32_t)L.rd[w];
    }
}

template <bool PACKED, bool TWO = false>
__global__ __launch_bounds__(64 * kIsWaves) void k_intersect_sorted(int64_t n_rays, const float *__restrict__ rays_o,
                                                          const float *__restrict__ rays_d,
                                                          const float *__restrict__ centres,
                                                          const int *__restrict__ structure,
                                                          const PackRec *__restrict__ packed, float voxel_size,
                                                          float max_distance, float step_size,
                                                          int *__restrict__ hit_idx, float *__restrict__ hit_t0,
                                                          float *__restrict__ hit_t1, int *__restrict__ ray_nv,
                                                          float *__restrict__ ray_dsum, int *__restrict__ stats,
                                                          int *__restrict__ blk_out, int *__restrict__ ray_rank,
                                                          int *__restrict__ rank_ray, unsigned long long *lb_desc,
                                                          uint32_t lb_tag, int *__restrict__ nv_rank,
                                                          int *__restrict__ col0_rank, LbCtl ctl) {
    // lb_desc != nullptr: the statistics / hit-rank pass (k_ray_stats_rank)
    // runs in this launch by decoupled look-back (lookback.h): each workgroup
    // ranks its own hit rays, the last one writes P / R_hit / max ⌈Σ/step⌉.
    // A workgroup whose look-back finds a predecessor that has not started
    // traces that block's rays too (their aggregate: lookback.h) — the
    // pass loop below; `own` is the first pass.
    __shared__ KeyLds lds_all[kIsWaves];
    KeyLds &S = lds_all[threadIdx.x / kWave];
    const int lane = threadIdx.x & (kWave - 1);
    const int blk = (int)blockIdx.x;
    if (lb_desc) {
        lb_debug_delay(ctl, blk);
        if (threadIdx.x == 0) lb_mark_started<5>(lb_desc, blk, (int)gridDim.x, lb_tag);
    }
    const float half = voxel_size * 0.5f;
    const uint64_t below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    __shared__ IsLds L;
    __shared__ int s_cmd;
    trace_pass<PACKED, TWO>(blk, n_rays, rays_o, rays_d, centres, structure, packed, half, max_distance, step_size, hit_idx,
                       hit_t0, hit_t1, ray_nv, ray_dsum, S, L);
    __syncthreads();
    if (threadIdx.x == 0) {
        int v = 0, ov = 0, sps = 0, rd = 0;
        for (int w = 0; w < kIsWaves; ++w) {
            v += L.vis[w];
            ov |= L.ov[w];
            sps += L.sp[w];
            rd += L.rd[w];
        }
        if (lb_desc) {
            // summed by the look-back below
        } else if (blk_out) {  // summed by k_ray_stats_rank: no same-address atomics (they serialise at the memory side)
            blk_out[2 * blk] = v;
            blk_out[2 * blk + 1] = rd;
        } else {
            atomicAdd(stats + PSVO_STAT_VISITS, v);
            atomicAdd(stats + PSVO_STAT_ROUNDS, rd);
        }
        if (sps) atomicAdd(stats + PSVO_STAT_SPILLS, sps);
        if (ov) atomicOr(stats + PSVO_STAT_FLAGS, kStatFlagDfsOverflow);
    }
    if (!lb_desc) return;
    // wave 0: the workgroup's aggregate → its exclusive prefix (lookback.h);
    // a predecessor that has not started: this workgroup traces that block's
    // rays too and publishes its aggregate (a helped block's statistics
    // arrive through it), then resumes its own look-back
    uint32_t own_agg[5], own_ex[5] = {0u, 0u, 0u, 0u, 0u};
    uint64_t own_hm = 0;
    int own_nv = 0, own_c0 = -1, lb_rc = kLbDone, spins = 0;
    if (threadIdx.x < kWave) {
        trace_agg(L, own_agg, own_hm);
        own_nv = lane < kIsWaves ? L.nv[lane] : 0;
        own_c0 = lane < kIsWaves ? L.c0[lane] : -1;
    }
    for (int cmd = -1;;) {  // one look-back call site; cmd ≥ 0: a block helped first
        if (cmd >= 0) {
            help_trace_pass(cmd, n_rays, rays_o, rays_d, centres, structure, half, max_distance, step_size, S, L);
            __syncthreads();
        }
        if (threadIdx.x < kWave) {
            if (cmd >= 0) {
                uint32_t agg[5];
                uint64_t hm;
                trace_agg(L, agg, hm);
                lb_publish<5>(lb_desc, cmd, lane, agg, lb_tag);
                if (lane == 0) atomicAdd(&psvo_g_lb_helps, 1ull);
            }
            lb_rc = lb_scan_help<5, 0b00110u>(lb_desc, blk, (int)gridDim.x, lb_tag, lane, own_agg, own_ex, spins,
                                               ctl.spin_max);
            if (lane == 0) s_cmd = lb_rc;
        }
        __syncthreads();
        cmd = __builtin_amdgcn_readfirstlane(s_cmd);
        if (cmd < 0) break;
    }
    if (threadIdx.x >= kWave) return;
    const bool ok = lb_rc == kLbDone;
    const uint32_t(&ex)[5] = own_ex;    // the exclusive prefix
    const uint32_t(&agg)[5] = own_agg;  // the own aggregate
    const int nv_l = own_nv;
    const uint64_t hm = own_hm;
    const int64_t rr = (int64_t)blk * kIsWaves + lane;
    if (lane < kIsWaves && rr < n_rays) {  // an abandoned wait (!ok) leaves `ex` undefined: no rank stores
        const int rk = (int)ex[0] + __popcll(hm & below);
        ray_rank[rr] = (nv_l > 0 && ok) ? rk : -1;
        if (nv_l > 0 && ok) {
            rank_ray[rk] = (int)rr;
            if (nv_rank) {  // by rank: the sampler's reads of other rows, one load each
                nv_rank[rk] = nv_l;
                col0_rank[rk] = own_c0;
            }
        }
    }
    if (lane == 0 && blk == (int)gridDim.x - 1) {  // the stats words were zeroed by the last read-back
        // an abandoned wait: no hit ray (the sampler then does nothing; the flag reports it)
        const int p = ok ? (int)max(ex[1], agg[1]) : 0, rh = ok ? (int)(ex[0] + agg[0]) : 0;
        const int mc = ok ? (int)max(ex[2], agg[2]) : 0;
        stats[PSVO_STAT_P] = p;
        stats[PSVO_STAT_R_HIT] = rh;
        stats[PSVO_STAT_MAX_CEIL] = mc;
        stats[kStatQuery + PSVO_STAT_P] = p;  // the sampler's copy (never re-zeroed inside its launch)
        stats[kStatQuery + PSVO_STAT_R_HIT] = rh;
        stats[kStatQuery + PSVO_STAT_MAX_CEIL] = mc;
        atomicAdd(stats + PSVO_STAT_VISITS, (int)(ex[3] + agg[3]));
        atomicAdd(stats + PSVO_STAT_ROUNDS, (int)(ex[4] + agg[4]));
    }
    if (!ok && lane == 0) atomicOr(stats + PSVO_STAT_FLAGS, kLbFlagTimeout);
}

}  // namespace
}  // namespace psvo

extern "C" int psvo_ray_intersect_sorted(void *stream, int64_t n_rays, const float *rays_o, const float *rays_d,
                                         const float *centres, const int *structure, float voxel_size,
                                         float max_distance, float step_size, int *hit_idx, float *hit_t0,
                                         float *hit_t1, int *ray_nv, float *ray_dsum, int *stats) {
    PSVO_REQUIRE(n_rays >= 0, "ray_intersect_sorted: n_rays < 0");
    PSVO_REQUIRE(step_size > 0.0f && voxel_size > 0.0f, "ray_intersect_sorted: step/voxel must be > 0");
    if (n_rays == 0) return PSVO_OK;
    hipStream_t st = as_stream(stream);
    psvo::launch(k_intersect_sorted<false>, dim3(div_up(n_rays, kIsWaves)), dim3(kIsWaves * kWave), 0, st,
                       n_rays, rays_o, rays_d, centres, structure, nullptr, voxel_size, max_distance, step_size,
                       hit_idx, hit_t0, hit_t1, ray_nv, ray_dsum, stats, nullptr, nullptr, nullptr, nullptr, 0u,
                       nullptr, nullptr, LbCtl{});
    psvo::launch(k_ray_stats, dim3(1), dim3(1024), 0, st, n_rays, ray_nv, ray_dsum, step_size, stats);
    return check_launch("ray_intersect_sorted");
}

extern "C" int psvo_ray_intersect_sorted_packed(void *stream, int64_t n_rays, const float *rays_o, const float *rays_d,
                                                const void *packed, const float *centres, const int *structure,
                                                float voxel_size, float max_distance, float step_size, int *hit_idx,
                                                float *hit_t0, float *hit_t1, int *ray_nv, float *ray_dsum,
                                                int *stats) {
    PSVO_REQUIRE(n_rays >= 0, "ray_intersect_sorted_packed: n_rays < 0");
    PSVO_REQUIRE(step_size > 0.0f && voxel_size > 0.0f, "ray_intersect_sorted_packed: step/voxel must be > 0");
    PSVO_REQUIRE(packed && ((uintptr_t)packed & 15) == 0, "ray_intersect_sorted_packed: packed records (16-B aligned)");
    if (n_rays == 0) return PSVO_OK;
    hipStream_t st = as_stream(stream);
    // (the two-chunk walk: the same hits; the deep-tree parity tests run it here)
    psvo::launch(k_intersect_sorted<true, true>, dim3(div_up(n_rays, kIsWaves)), dim3(kIsWaves * kWave), 0, st,
                       n_rays, rays_o, rays_d, centres, structure, static_cast<const PackRec *>(packed), voxel_size,
                       max_distance, step_size, hit_idx, hit_t0, hit_t1, ray_nv, ray_dsum, stats, nullptr, nullptr,
                       nullptr, nullptr, 0u, nullptr, nullptr, LbCtl{});
    psvo::launch(k_ray_stats, dim3(1), dim3(1024), 0, st, n_rays, ray_nv, ray_dsum, step_size, stats);
    return check_launch("ray_intersect_sorted_packed");
}

namespace psvo {
// psvo_ray_intersect_sorted + psvo_hit_rank with the two single-block
// reductions fused into one launch (engine_query.cpp, render.hip)
int intersect_ranked(hipStream_t st, int64_t n_rays, const float *rays_o, const float *rays_d, const float *centres,
                     const int *structure, float voxel_size, float max_distance, float step_size, int *hit_idx,
                     float *hit_t0, float *hit_t1, int *ray_nv, float *ray_dsum, int *stats, int *ray_rank,
                     int *rank_ray, const PackRec *packed, int *blk_out, unsigned long long *lb_desc,
                     uint32_t lb_tag, int *nv_rank, int *col0_rank, int64_t n_nodes) {
    PSVO_REQUIRE(n_rays >= 0, "intersect_ranked: n_rays < 0");
    PSVO_REQUIRE((nv_rank == nullptr) == (col0_rank == nullptr) && (!nv_rank || lb_desc),
                 "intersect_ranked: the by-rank copies come with the look-back pass");
    PSVO_REQUIRE(step_size > 0.0f && voxel_size > 0.0f, "intersect_ranked: step/voxel must be > 0");
    PSVO_REQUIRE(!lb_desc || (n_rays <= kLbMaxRays && lb_tag != 0), "intersect_ranked: look-back arguments");
    if (n_rays == 0) return PSVO_OK;
    // lb_desc: the statistics / rank pass inside the traversal launch (look-
    // back; the stats words are zero: memset / the last read-back)
    if (packed)
        psvo::launch(n_nodes >= kTwoChunkNodes ? k_intersect_sorted<true, true> : k_intersect_sorted<true, false>,
                     dim3(div_up(n_rays, kIsWaves)), dim3(kIsWaves * kWave), 0, st, n_rays, rays_o, rays_d, centres,
                     structure, packed, voxel_size, max_distance, step_size, hit_idx, hit_t0, hit_t1, ray_nv,
                     ray_dsum, stats, blk_out, ray_rank, rank_ray, lb_desc, lb_tag, nv_rank, col0_rank, lb_ctl(1));
    else
        psvo::launch(k_intersect_sorted<false>, dim3(div_up(n_rays, kIsWaves)), dim3(kIsWaves * kWave), 0, st,
                           n_rays, rays_o, rays_d, centres, structure, nullptr, voxel_size, max_distance, step_size,
                           hit_idx, hit_t0, hit_t1, ray_nv, ray_dsum, stats, blk_out, ray_rank, rank_ray, lb_desc,
                           lb_tag, nv_rank, col0_rank, lb_ctl(1));
    if (!lb_desc)
        psvo::launch(k_ray_stats_rank, dim3(1), dim3(1024), 0, st, n_rays, ray_nv, ray_dsum, step_size, stats,
                           ray_rank, rank_ray, blk_out, (int)div_up(n_rays, kIsWaves));
    return check_launch("intersect_ranked");
}

// the traversal's helped-block counter (psvo_debug_lb_helps)
int lb_helps_trace(int64_t *out1, bool reset) {
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
extern "C" int psvo_debug_is_stamps(void *dst, int64_t bytes) {
    if (bytes < (int64_t)sizeof(psvo::psvo_g_is_stamps)) return -1;
    return hipMemcpyFromSymbol(dst, HIP_SYMBOL(psvo::psvo_g_is_stamps), sizeof(psvo::psvo_g_is_stamps)) == hipSuccess ? 0 : -2;
}
#endif
