// Sparse voxel octree builder on the device: the same
// tree as octree.cpp / the reference's Octree::insert (octree.cpp:104-294) —
// node ids in CREATION ORDER, root 0, every voxel inserting itself as a
// SURFACE leaf and its 7 +1 corner neighbours as FEATURE leaves — and the
// export of get_centres_and_children (octree.cpp:561-687) plus the renderer's
// map_states arrays (mapping.py:300-406), without the per-frame CPU walk and
// host→device copy.
//
// Sequential semantics, parallel construction.  Walk w = 8·i + j (voxel i,
// corner j) visits depths d = 1..D; the sequential insert creates node
// (d, path prefix) at the FIRST walk (in w order) whose path reaches it, in
// the order (w, d).  So one insert call is:
//   1. every (w, d) hashes its node key into a device hash table (open
//      addressing, 64-bit CAS) and atomicMin's its walk index into the slot;
//      walks with j = 0 flag their leaf SURFACE;
//   2. (w, d) is a creator iff its slot has no node yet and holds min-walk w;
//   3. an exclusive scan of the creator flags in (w, d) order is exactly the
//      creation order: id = count + rank;
//   4. creators write their node (code of the creating walk, side, type) and
//      link themselves into their parent's child slot; SURFACE flags promote
//      leaves (FEATURE → SURFACE, octree.cpp:247-248).
// The table persists across inserts (existing nodes are never creators), so
// incremental inserts extend the tree exactly like repeated CPU inserts.
// Node arrays (code, side, type, child[8]) are struct-of-arrays in HBM;
// capacity doubles (with a rehash) when a batch could overflow it.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "psvo_common.h"

namespace psvo {
namespace {

constexpr int kDtMaxBits = 21;  // utils.h:12
constexpr int8_t kDtNonLeaf = -1, kDtSurface = 0, kDtFeature = 1;
constexpr uint64_t kEmptyKey = ~0ull;

__host__ __device__ __forceinline__ uint64_t dt_spread3(uint64_t v) {
    uint64_t x = v & 0x1fffffull;
    x = (x | x << 32) & 0x1f00000000ffffull;
    x = (x | x << 16) & 0x1f0000ff0000ffull;
    x = (x | x << 8) & 0x100f00f00f00f00full;
    x = (x | x << 4) & 0x10c30c30c30c30c3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}
__device__ __forceinline__ uint64_t dt_squeeze3(uint64_t v) {
    uint64_t x = v & 0x1249249249249249ull;
    x = (x | x >> 2) & 0x10c30c30c30c30c3ull;
    x = (x | x >> 4) & 0x100f00f00f00f00full;
    x = (x | x >> 8) & 0x1f0000ff0000ffull;
    x = (x | x >> 16) & 0x1f00000000ffffull;
    x = (x | x >> 32) & 0x1fffffull;
    return x;
}
__device__ __forceinline__ uint64_t dt_prefix_mask(int i) {  // utils.h:56-77
    return i >= 20 ? 0x7fffffffffffffffull : ~((1ull << (60 - 3 * i)) - 1) & 0x7fffffffffffffffull;
}
__device__ __forceinline__ uint64_t dt_morton(int x, int y, int z) {  // utils.h (code of a corner)
    return (dt_spread3((uint64_t)(int64_t)x) | dt_spread3((uint64_t)(int64_t)y) << 1 |
            dt_spread3((uint64_t)(int64_t)z) << 2) &
           dt_prefix_mask(kDtMaxBits - 1);
}
// identity of the node at depth d on the path of (x, y, z): the path bits
// below size/2 (the walk ignores higher bits, octree.cpp:157-160) and d
__device__ __forceinline__ uint64_t dt_key(int x, int y, int z, int d, int D) {
    const int sh = D - d;
    const uint64_t m = (d >= 21) ? 0x1fffffull : ((1ull << d) - 1);
    const uint64_t xs = ((uint64_t)(uint32_t)x >> sh) & m, ys = ((uint64_t)(uint32_t)y >> sh) & m,
                   zs = ((uint64_t)(uint32_t)z >> sh) & m;
    return ((dt_spread3(xs) | dt_spread3(ys) << 1 | dt_spread3(zs) << 2) << 5) | (uint64_t)d;
}
__device__ __forceinline__ uint64_t dt_hash(uint64_t k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}

struct DtTable {
    unsigned long long *key;
    unsigned int *minw;
    int *id;
    unsigned int *flags;
    uint64_t mask;  // capacity - 1 (power of two)
};

constexpr int kDtMaxProbe = 256;
constexpr uint64_t kDtNoSlot = ~0ull;
// k_dt_walk's status word: a probe run overflowed (the batch is redone in a
// larger table); some leaf became SURFACE (the generation advances)
constexpr int kDtWalkOverflow = 1, kDtWalkChanged = 2;

// slot of `k`, inserting it if absent; kDtNoSlot if the probe run exceeds
// kDtMaxProbe (the host grows the table and redoes the batch)
__device__ __forceinline__ uint64_t dt_insert(const DtTable &t, uint64_t k) {
    uint64_t s = dt_hash(k) & t.mask;
    for (int probe = 0; probe < kDtMaxProbe; ++probe) {
        const unsigned long long cur = t.key[s];
        if (cur == k) return s;
        if (cur == kEmptyKey) {
            const unsigned long long prev = atomicCAS(t.key + s, kEmptyKey, (unsigned long long)k);
            if (prev == kEmptyKey || prev == k) return s;
        }
        s = (s + 1) & t.mask;
    }
    return kDtNoSlot;
}
__device__ __forceinline__ int64_t dt_find(const DtTable &t, uint64_t k) {
    uint64_t s = dt_hash(k) & t.mask;
    for (int probe = 0; probe < kDtMaxProbe; ++probe) {
        const unsigned long long cur = t.key[s];
        if (cur == k) return (int64_t)s;
        if (cur == kEmptyKey) return -1;
        s = (s + 1) & t.mask;
    }
    return -1;
}

__constant__ int kDtIncX[8] = {0, 0, 0, 0, 1, 1, 1, 1};
__constant__ int kDtIncY[8] = {0, 0, 1, 1, 0, 0, 1, 1};
__constant__ int kDtIncZ[8] = {0, 1, 0, 1, 0, 1, 0, 1};

struct DtNodes {
    unsigned long long *code;
    int *side;
    int8_t *type;
    int *child;  // [cap][8]
};

__global__ void k_dt_fill(DtTable t, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > t.mask) return;
    t.key[i] = kEmptyKey;
    t.minw[i] = 0xffffffffu;
    t.id[i] = -1;
    t.flags[i] = 0;
    (void)n;
}
__global__ void k_dt_fill_child(int *child, int64_t from, int64_t to) {
    const int64_t i = from + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < to) child[i] = -1;
}

// (re)insert existing nodes [0, n) into a fresh table: key from the stored path
// (code of a node = prefix of its creating walk; the path bits are recovered
// from the code's coordinates)
__global__ void k_dt_rehash(DtTable t, DtNodes nd, int64_t n, int D) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t c = nd.code[i];
    const int x = (int)dt_squeeze3(c), y = (int)dt_squeeze3(c >> 1), z = (int)dt_squeeze3(c >> 2);
    const int d = D - (31 - __clz(nd.side[i]));  // side = size >> d
    const uint64_t s = dt_insert(t, dt_key(x, y, z, d, D));
    if (s == kDtNoSlot) return;  // cannot happen below load 1/2 (the table holds >= 2 slots per node)
    t.id[s] = (int)i;
    if (nd.type[i] == kDtSurface) t.flags[s] = 1u;
}

// 1. keys + min walk + SURFACE flags
__global__ void k_dt_walk(DtTable t, const int *__restrict__ vox, int64_t n_walks, int D, unsigned w_base,
                          int *__restrict__ overflow) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_walks * D) return;
    const int64_t w = e / D;
    const int d = (int)(e - w * D) + 1;
    const int64_t i = w >> 3;
    const int j = (int)(w & 7);
    const int x = vox[3 * i] + kDtIncX[j], y = vox[3 * i + 1] + kDtIncY[j], z = vox[3 * i + 2] + kDtIncZ[j];
    const uint64_t s = dt_insert(t, dt_key(x, y, z, d, D));
    if (s == kDtNoSlot) {
        if (!(__atomic_load_n(overflow, __ATOMIC_RELAXED) & kDtWalkOverflow)) atomicOr(overflow, kDtWalkOverflow);
        return;
    }
    // the shallow keys are shared by nearly every walk: a plain read first
    // keeps the same-address atomics (which serialise) to the few that can win
    const unsigned wv = w_base + (unsigned)w;
    if (wv < __atomic_load_n(t.minw + s, __ATOMIC_RELAXED)) atomicMin(t.minw + s, wv);
    if (d == D && j == 0 && !(__atomic_load_n(t.flags + s, __ATOMIC_RELAXED) & 1u)) {
        atomicOr(t.flags + s, 1u);
        // a leaf that was not SURFACE before (new, or a FEATURE leaf promoted): the tree changes
        if (!(__atomic_load_n(overflow, __ATOMIC_RELAXED) & kDtWalkChanged)) atomicOr(overflow, kDtWalkChanged);
    }
}

// 2. creator flags (w, d order)
__global__ void k_dt_flag(DtTable t, const int *__restrict__ vox, int64_t n_walks, int D, unsigned w_base,
                          int *__restrict__ flag) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_walks * D) return;
    const int64_t w = e / D;
    const int d = (int)(e - w * D) + 1;
    const int64_t i = w >> 3;
    const int j = (int)(w & 7);
    const int x = vox[3 * i] + kDtIncX[j], y = vox[3 * i + 1] + kDtIncY[j], z = vox[3 * i + 2] + kDtIncZ[j];
    const int64_t s = dt_find(t, dt_key(x, y, z, d, D));
    flag[e] = (s >= 0 && t.id[s] < 0 && t.minw[s] == w_base + (unsigned)w) ? 1 : 0;
}

// block-local exclusive scan + block totals; totals scanned by one block; offsets added
__global__ __launch_bounds__(1024) void k_dt_scan_local(const int *__restrict__ in, int64_t n, int *__restrict__ out,
                                                        int *__restrict__ totals) {
    __shared__ int ws[16];
    const int64_t i = (int64_t)blockIdx.x * 1024 + threadIdx.x;
    const int v = i < n ? in[i] : 0;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) {
        const int t = __shfl_up(inc, sh, 64);
        if (lane >= sh) inc += t;
    }
    if (lane == 63) ws[w] = inc;
    __syncthreads();
    if (w == 0) {
        int s = lane < 16 ? ws[lane] : 0;
#pragma unroll
        for (int sh = 1; sh < 16; sh <<= 1) {
            const int t = __shfl_up(s, sh, 64);
            if (lane >= sh) s += t;
        }
        if (lane < 16) ws[lane] = s;
    }
    __syncthreads();
    const int excl = (w > 0 ? ws[w - 1] : 0) + inc - v;
    if (i < n) out[i] = excl;
    if (threadIdx.x == 1023) totals[blockIdx.x] = ws[15];
}
__global__ __launch_bounds__(1024) void k_dt_scan_totals(int *__restrict__ totals, int64_t nb, int *__restrict__ sum) {
    __shared__ int part[1024];
    const int64_t per = (nb + 1023) / 1024;
    const int64_t b0 = threadIdx.x * per, b1 = b0 + per < nb ? b0 + per : nb;
    int local = 0;
    for (int64_t b = b0; b < b1; ++b) local += totals[b];
    part[threadIdx.x] = local;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int v = threadIdx.x >= off ? part[threadIdx.x - off] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    int run = part[threadIdx.x] - local;
    for (int64_t b = b0; b < b1; ++b) {
        const int t = totals[b];
        totals[b] = run;
        run += t;
    }
    if (threadIdx.x == 1023) *sum = part[1023];
}
__global__ void k_dt_scan_add(int *__restrict__ out, int64_t n, const int *__restrict__ totals) {
    const int64_t i = (int64_t)blockIdx.x * 1024 + threadIdx.x;
    if (i < n) out[i] += totals[blockIdx.x];
}

// 4a. creators: ids and node rows
__global__ void k_dt_create(DtTable t, DtNodes nd, const int *__restrict__ vox, int64_t n_walks, int D, int shift,
                            int size, const int *__restrict__ flag, const int *__restrict__ rank, int64_t count) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_walks * D || !flag[e]) return;
    const int64_t w = e / D;
    const int d = (int)(e - w * D) + 1;
    const int64_t i = w >> 3;
    const int j = (int)(w & 7);
    const int x = vox[3 * i] + kDtIncX[j], y = vox[3 * i + 1] + kDtIncY[j], z = vox[3 * i + 2] + kDtIncZ[j];
    const int64_t s = dt_find(t, dt_key(x, y, z, d, D));
    const int id = (int)(count + rank[e]);
    t.id[s] = id;
    nd.code[id] = dt_morton(x, y, z) & dt_prefix_mask(d + shift);
    nd.side[id] = size >> d;
    nd.type[id] = d == D ? kDtFeature : kDtNonLeaf;
}

// 4b. links (every id assigned) and SURFACE promotion
__global__ void k_dt_link(DtTable t, DtNodes nd, const int *__restrict__ vox, int64_t n_walks, int D, int size,
                          const int *__restrict__ flag) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_walks * D) return;
    const int64_t w = e / D;
    const int d = (int)(e - w * D) + 1;
    const int64_t i = w >> 3;
    const int j = (int)(w & 7);
    const int x = vox[3 * i] + kDtIncX[j], y = vox[3 * i + 1] + kDtIncY[j], z = vox[3 * i + 2] + kDtIncZ[j];
    if (flag[e]) {
        const int64_t s = dt_find(t, dt_key(x, y, z, d, D));
        const int parent = d == 1 ? 0 : t.id[dt_find(t, dt_key(x, y, z, d - 1, D))];
        const int edge = size >> d;
        const int cid = ((x & edge) > 0) + 2 * ((y & edge) > 0) + 4 * ((z & edge) > 0);
        nd.child[(int64_t)parent * 8 + cid] = t.id[s];
    }
    if (d == D && j == 0) nd.type[t.id[dt_find(t, dt_key(x, y, z, d, D))]] = kDtSurface;
}

// get_centres_and_children rows + the render arrays (mapping.py:328-372)
__global__ void k_dt_export(DtTable t, DtNodes nd, int64_t n, int D, float voxel_size, float *__restrict__ voxels,
                            float *__restrict__ children, int *__restrict__ features, float *__restrict__ centres,
                            int *__restrict__ structure) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int8_t ty = nd.type[i];
    const uint64_t c = nd.code[i];
    const int x = (int)dt_squeeze3(c), y = (int)dt_squeeze3(c >> 1), z = (int)dt_squeeze3(c >> 2);
    const int side = nd.side[i];
    const bool live = ty != kDtFeature;  // FEATURE rows are never reached by the reference BFS
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (live) {
        v[0] = (float)x;
        v[1] = (float)y;
        v[2] = (float)z;
        v[3] = (float)side;
    }
    if (voxels) {
#pragma unroll
        for (int k = 0; k < 4; ++k) voxels[i * 4 + k] = v[k];
    }
    if (centres) {  // (xyz + side/2) · voxel, as mapping.py:328 in fp32
#pragma unroll
        for (int k = 0; k < 3; ++k) centres[i * 3 + k] = __fmul_rn(__fadd_rn(v[k], __fmul_rn(v[3], 0.5f)), voxel_size);
    }
    int ch[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int cc = live ? nd.child[i * 8 + k] : -1;
        ch[k] = (cc >= 0 && nd.type[cc] != kDtFeature) ? cc : -1;
        if (children) children[i * 8 + k] = (float)ch[k];
        if (structure) structure[i * 9 + k] = ch[k];
    }
    if (structure) structure[i * 9 + 8] = (int)v[3];
    if (features) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            int f = -1;
            if (ty == kDtSurface) {  // find(corner) (octree.cpp:419-439): the leaf at the corner's path
                const int64_t s = dt_find(t, dt_key(x + kDtIncX[k], y + kDtIncY[k], z + kDtIncZ[k], D, D));
                f = s >= 0 ? t.id[s] : -1;
            }
            features[i * 8 + k] = f;
        }
    }
}

__global__ void k_dt_count_type(const int8_t *__restrict__ type, int64_t n, int8_t want, int *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int v = (i < n && type[i] == want) ? 1 : 0;
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) v += __shfl_xor(v, sh, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(out, v);
}

__global__ void k_dt_probe(DtTable t, const int *__restrict__ vox, int64_t n, int D, int corners, int *__restrict__ hit) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * corners) return;
    const int64_t i = e / corners;
    const int j = (int)(e - i * corners);
    const int64_t s = dt_find(t, dt_key(vox[3 * i] + kDtIncX[j], vox[3 * i + 1] + kDtIncY[j], vox[3 * i + 2] + kDtIncZ[j], D, D));
    hit[e] = (s >= 0 && t.id[s] >= 0) ? 1 : 0;
}

// ---- one depth frame into the tree (psvo_dtree_insert_depth) ----
// Mapping.create_voxels_pointcloud (mapping.py:258-295) without the per-pixel
// insert: the pixels' voxel keys, the first occurrence of every distinct key
// (a frame-local hash set holding the minimum pixel index), of those the ones
// the tree has no SURFACE leaf for, compacted in pixel order — the list the
// walk … link stages above then insert.  A later duplicate and a voxel that
// is already a SURFACE leaf change nothing in Octree::insert, so the tree is
// the one raw insertion of every valid pixel builds.

// state of a pixel: 0 no depth, 1 valid, 2 depth > 0 but no int32 key
// World point ((v0·R[k][0] + v1·R[k][1]) + v2·R[k][2]) + t[k] of v = dir · depth,
// every product and sum rounded to fp32 on its own (no contraction), then
// torch's floor division by the voxel size.
__device__ __forceinline__ int fi_pixel_key(float depth, float d0, float d1, float d2, const float *P, float voxel_size,
                                            int *key) {
    // plain operators with contraction off for this block: __fmul_rn / __fadd_rn
    // are `x * y` / `x + y` in the HIP headers and inline into contractible code
#pragma clang fp contract(off)
    key[0] = key[1] = key[2] = 0;
    if (!(depth > 0.f)) return 0;
    const float v0 = d0 * depth, v1 = d1 * depth, v2 = d2 * depth;
    bool ok = true;
    int q[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float p0 = v0 * P[4 * k], p1 = v1 * P[4 * k + 1], p2 = v2 * P[4 * k + 2];
        const float wk = ((p0 + p1) + p2) + P[4 * k + 3];
        const float f = div_floor(wk, voxel_size);
        // torch's .int() is defined only for a finite quotient inside int32
        const bool in = isfinite(wk) && f >= -2147483648.f && f < 2147483648.f;
        ok = ok && in;
        q[k] = in ? (int)f : 0;
    }
    if (!ok) return 2;
    key[0] = q[0], key[1] = q[1], key[2] = q[2];
    return 1;
}

// keys i32[n,3] and valid u8[n]; four consecutive pixels per lane, 16-B loads
// and stores when every pointer allows (vec); stats (or null): += valid, skipped
__global__ __launch_bounds__(256) void k_fi_keys(int64_t n, const float *__restrict__ depth,
                                                 const float *__restrict__ dirs, const float *__restrict__ pose,
                                                 float voxel_size, int *__restrict__ keys,
                                                 uint8_t *__restrict__ valid, int vec, int *__restrict__ stats) {
    float P[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) P[i] = pose[i];
    const int64_t p0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    int n_valid = 0, n_skipped = 0;
    if (p0 < n) {
        const bool full = vec && p0 + 4 <= n;
        float dep[4] = {0.f, 0.f, 0.f, 0.f}, dir[12];
        if (full) {
            const float4 a = *reinterpret_cast<const float4 *>(depth + p0);
            const float4 *dv = reinterpret_cast<const float4 *>(dirs + 3 * p0);
            const float4 b0 = dv[0], b1 = dv[1], b2 = dv[2];
            dep[0] = a.x, dep[1] = a.y, dep[2] = a.z, dep[3] = a.w;
            dir[0] = b0.x, dir[1] = b0.y, dir[2] = b0.z, dir[3] = b0.w;
            dir[4] = b1.x, dir[5] = b1.y, dir[6] = b1.z, dir[7] = b1.w;
            dir[8] = b2.x, dir[9] = b2.y, dir[10] = b2.z, dir[11] = b2.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool in = p0 + j < n;
                dep[j] = in ? depth[p0 + j] : 0.f;
#pragma unroll
                for (int k = 0; k < 3; ++k) dir[3 * j + k] = in ? dirs[3 * (p0 + j) + k] : 0.f;
            }
        }
        int key[12];
        uint8_t ok[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int s = fi_pixel_key(dep[j], dir[3 * j], dir[3 * j + 1], dir[3 * j + 2], P, voxel_size, key + 3 * j);
            ok[j] = s == 1;
            n_valid += s == 1;
            n_skipped += s == 2;
        }
        if (full) {
            int4 *kv = reinterpret_cast<int4 *>(keys + 3 * p0);
            kv[0] = make_int4(key[0], key[1], key[2], key[3]);
            kv[1] = make_int4(key[4], key[5], key[6], key[7]);
            kv[2] = make_int4(key[8], key[9], key[10], key[11]);
            *reinterpret_cast<uchar4 *>(valid + p0) = make_uchar4(ok[0], ok[1], ok[2], ok[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (p0 + j >= n) break;
#pragma unroll
                for (int k = 0; k < 3; ++k) keys[3 * (p0 + j) + k] = key[3 * j + k];
                valid[p0 + j] = ok[j];
            }
        }
    }
    if (stats) {
#pragma unroll
        for (int sh = 32; sh > 0; sh >>= 1) {
            n_valid += __shfl_xor(n_valid, sh, 64);
            n_skipped += __shfl_xor(n_skipped, sh, 64);
        }
        if ((threadIdx.x & 63) == 0) {
            if (n_valid) atomicAdd(stats + PSVO_FRAME_STAT_VALID, n_valid);
            if (n_skipped) atomicAdd(stats + PSVO_FRAME_STAT_SKIPPED, n_skipped);
        }
    }
}

// The frame's set: open addressing with linear probing over `mask + 1` slots
// of {key, minimum pixel index}, at least two slots per pixel, so a probe
// always meets the key or an empty slot (the bound below only keeps a
// corrupted set from spinning).  The walk, the hash key and the node code
// read the low 21 bits of a coordinate (dt_key, dt_morton, dt_spread3), so
// those 63 bits identify the voxel.
struct FiSet {
    unsigned long long *key;
    unsigned int *minp;
    uint64_t mask;
};
__device__ __forceinline__ uint64_t fi_pack(const int *k) {
    return ((uint64_t)k[0] & 0x1fffffull) | ((uint64_t)k[1] & 0x1fffffull) << 21 | ((uint64_t)k[2] & 0x1fffffull) << 42;
}
// head of a run: a valid pixel whose previous pixel is not a valid pixel with
// the same key; every other valid pixel is a duplicate and never touches the set
__device__ __forceinline__ bool fi_head(const int *__restrict__ keys, const uint8_t *__restrict__ valid, int64_t p,
                                        uint64_t &pk) {
    if (!valid[p]) return false;
    pk = fi_pack(keys + 3 * p);
    return !(p > 0 && valid[p - 1] && fi_pack(keys + 3 * (p - 1)) == pk);
}

__global__ __launch_bounds__(256) void k_fi_set(FiSet s, const int *__restrict__ keys,
                                                const uint8_t *__restrict__ valid, int64_t n) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t pk;
    if (p >= n || !fi_head(keys, valid, p, pk)) return;
    uint64_t i = dt_hash(pk) & s.mask;
    for (uint64_t probe = 0; probe <= s.mask; ++probe) {
        unsigned long long cur = s.key[i];
        if (cur == kEmptyKey) {
            cur = atomicCAS(s.key + i, kEmptyKey, (unsigned long long)pk);
            if (cur == kEmptyKey) cur = pk;
        }
        if (cur == pk) {
            if ((unsigned)p < __atomic_load_n(s.minp + i, __ATOMIC_RELAXED)) atomicMin(s.minp + i, (unsigned)p);
            return;
        }
        i = (i + 1) & s.mask;
    }
}

// survivors: run heads that hold their key's minimum pixel index and whose
// voxel is not a SURFACE leaf yet.  lrank[p] = rank among the block's
// survivors in pixel order (ballot + mbcnt in the wave, a scan of the 16 wave
// totals), −1 for the others; totals[block] = the block's survivors.
__global__ __launch_bounds__(1024) void k_fi_flag(FiSet s, DtTable t, DtNodes nd, int D, const int *__restrict__ keys,
                                                  const uint8_t *__restrict__ valid, int64_t n,
                                                  int *__restrict__ lrank, int *__restrict__ totals,
                                                  int *__restrict__ stats) {
    __shared__ int ws[16];
    const int64_t p = (int64_t)blockIdx.x * 1024 + threadIdx.x;
    bool first = false, surv = false;
    uint64_t pk;
    if (p < n && fi_head(keys, valid, p, pk)) {
        uint64_t i = dt_hash(pk) & s.mask;
        for (uint64_t probe = 0; probe <= s.mask; ++probe) {
            const unsigned long long cur = s.key[i];
            if (cur == pk) {
                first = s.minp[i] == (unsigned)p;
                break;
            }
            if (cur == kEmptyKey) break;
            i = (i + 1) & s.mask;
        }
        if (first) {
            const int *k = keys + 3 * p;
            const int64_t sl = dt_find(t, dt_key(k[0], k[1], k[2], D, D));
            const int id = sl >= 0 ? t.id[sl] : -1;
            surv = !(id >= 0 && nd.type[id] == kDtSurface);
        }
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(surv), bal_first = __ballot(first);
    const int in_wave = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
    if (lane == 0) {
        ws[w] = __popcll(bal);
        if (bal_first) atomicAdd(stats + PSVO_FRAME_STAT_DISTINCT, __popcll(bal_first));
    }
    __syncthreads();
    if (w == 0) {
        int v = lane < 16 ? ws[lane] : 0;
#pragma unroll
        for (int sh = 1; sh < 16; sh <<= 1) {
            const int u = __shfl_up(v, sh, 64);
            if (lane >= sh) v += u;
        }
        if (lane < 16) ws[lane] = v;
    }
    __syncthreads();
    if (p < n) lrank[p] = surv ? (w > 0 ? ws[w - 1] : 0) + in_wave : -1;
    if (threadIdx.x == 1023) totals[blockIdx.x] = ws[15];
}

// totals: the blocks' exclusive offsets (k_dt_scan_totals)
__global__ __launch_bounds__(1024) void k_fi_compact(const int *__restrict__ keys, const int *__restrict__ lrank,
                                                     const int *__restrict__ totals, int64_t n, int *__restrict__ list) {
    const int64_t p = (int64_t)blockIdx.x * 1024 + threadIdx.x;
    if (p >= n) return;
    const int r = lrank[p];
    if (r < 0) return;
    const int64_t o = (int64_t)totals[blockIdx.x] + r;
#pragma unroll
    for (int k = 0; k < 3; ++k) list[3 * o + k] = keys[3 * p + k];
}

}  // namespace
}  // namespace psvo

using namespace psvo;

struct psvo_dtree {
    int size = 0, D = 0, shift = 0;
    int64_t count = 0, cap = 0;
    unsigned w_next = 0;  // walk counter across inserts (min-walk order stays global)
    DtTable t{};
    DtNodes nd{};
    int *scratch = nullptr;  // flags | ranks | totals | sum | overflow
    int64_t scratch_n = 0;
    uint64_t generation = 0;  // advances when an insert created a node or promoted a leaf
    char *frame_ws = nullptr;  // psvo_dtree_insert_depth's workspace (FrameLayout), reused across frames
    int64_t frame_ws_bytes = 0;
};

namespace {

int dt_alloc_nodes(psvo_dtree *tr, int64_t cap, hipStream_t st) {
    DtNodes n{};
    if (hipMalloc(&n.code, cap * sizeof(unsigned long long)) != hipSuccess ||
        hipMalloc(&n.side, cap * sizeof(int)) != hipSuccess || hipMalloc(&n.type, cap * sizeof(int8_t)) != hipSuccess ||
        hipMalloc(&n.child, cap * 8 * sizeof(int)) != hipSuccess)
        return set_error(PSVO_E_LAUNCH, "dtree: out of device memory (%lld nodes)", (long long)cap);
    if (tr->count > 0) {
        (void)hipMemcpyAsync(n.code, tr->nd.code, tr->count * sizeof(unsigned long long), hipMemcpyDeviceToDevice, st);
        (void)hipMemcpyAsync(n.side, tr->nd.side, tr->count * sizeof(int), hipMemcpyDeviceToDevice, st);
        (void)hipMemcpyAsync(n.type, tr->nd.type, tr->count * sizeof(int8_t), hipMemcpyDeviceToDevice, st);
        (void)hipMemcpyAsync(n.child, tr->nd.child, tr->count * 8 * sizeof(int), hipMemcpyDeviceToDevice, st);
    }
    psvo::launch(k_dt_fill_child, dim3(div_up((cap - tr->count) * 8, 256)), dim3(256), 0, st, n.child,
                       tr->count * 8, cap * 8);
    if (tr->cap > 0) {
        (void)hipStreamSynchronize(st);
        (void)hipFree(tr->nd.code);
        (void)hipFree(tr->nd.side);
        (void)hipFree(tr->nd.type);
        (void)hipFree(tr->nd.child);
    }
    tr->nd = n;
    tr->cap = cap;
    return PSVO_OK;
}

int dt_alloc_table(psvo_dtree *tr, hipStream_t st, uint64_t min_slots) {
    uint64_t slots = 1024;
    while (slots < min_slots || slots < (uint64_t)tr->count * 2) slots <<= 1;
    DtTable t{};
    if (hipMalloc(&t.key, slots * sizeof(unsigned long long)) != hipSuccess ||
        hipMalloc(&t.minw, slots * sizeof(unsigned)) != hipSuccess || hipMalloc(&t.id, slots * sizeof(int)) != hipSuccess ||
        hipMalloc(&t.flags, slots * sizeof(unsigned)) != hipSuccess)
        return set_error(PSVO_E_LAUNCH, "dtree: out of device memory (hash table)");
    t.mask = slots - 1;
    psvo::launch(k_dt_fill, dim3(div_up((int64_t)slots, 256)), dim3(256), 0, st, t, slots);
    if (tr->count > 0)
        psvo::launch(k_dt_rehash, dim3(div_up(tr->count, 256)), dim3(256), 0, st, t, tr->nd, tr->count, tr->D);
    if (tr->t.key) {
        (void)hipStreamSynchronize(st);
        (void)hipFree(tr->t.key);
        (void)hipFree(tr->t.minw);
        (void)hipFree(tr->t.id);
        (void)hipFree(tr->t.flags);
    }
    tr->t = t;
    return PSVO_OK;
}

}  // namespace

extern "C" void *psvo_dtree_new(void *stream, int grid_dim, int64_t capacity) {
    if (grid_dim < 2 || (grid_dim & (grid_dim - 1)) || grid_dim > (1 << 16)) {
        set_error(PSVO_E_INVALID, "dtree_new: grid_dim must be a power of two in [2, 65536]");
        return nullptr;
    }
    hipStream_t st = as_stream(stream);
    psvo_dtree *tr = new psvo_dtree;
    tr->size = grid_dim;
    int D = 0;
    while ((1 << D) < grid_dim) ++D;
    tr->D = D;
    tr->shift = kDtMaxBits - D - 1;
    const int64_t cap0 = capacity > 1024 ? capacity : 1024;
    if (dt_alloc_nodes(tr, cap0, st) != PSVO_OK || dt_alloc_table(tr, st, (uint64_t)cap0 * 2) != PSVO_OK) {
        delete tr;
        return nullptr;
    }
    // root: id 0, code 0, side = grid_dim, key (d = 0)
    const unsigned long long zero = 0;
    const int side = grid_dim;
    const int8_t nl = kDtNonLeaf;
    (void)hipMemcpyAsync(tr->nd.code, &zero, sizeof(zero), hipMemcpyHostToDevice, st);
    (void)hipMemcpyAsync(tr->nd.side, &side, sizeof(side), hipMemcpyHostToDevice, st);
    (void)hipMemcpyAsync(tr->nd.type, &nl, sizeof(nl), hipMemcpyHostToDevice, st);
    tr->count = 1;
    psvo::launch(k_dt_rehash, dim3(1), dim3(64), 0, st, tr->t, tr->nd, (int64_t)1, tr->D);
    if (hipStreamSynchronize(st) != hipSuccess) {
        set_error(PSVO_E_LAUNCH, "dtree_new: device init failed");
        delete tr;
        return nullptr;
    }
    return tr;
}

extern "C" void psvo_dtree_free(void *tree) {
    psvo_dtree *tr = static_cast<psvo_dtree *>(tree);
    if (!tr) return;
    (void)hipDeviceSynchronize();
    (void)hipFree(tr->nd.code);
    (void)hipFree(tr->nd.side);
    (void)hipFree(tr->nd.type);
    (void)hipFree(tr->nd.child);
    (void)hipFree(tr->t.key);
    (void)hipFree(tr->t.minw);
    (void)hipFree(tr->t.id);
    (void)hipFree(tr->t.flags);
    (void)hipFree(tr->scratch);
    (void)hipFree(tr->frame_ws);
    delete tr;
}

namespace {

// one batch of voxels (n > 0) through the walk … link stages; *created: the
// nodes it made, *changed: it made one or turned a leaf SURFACE
int dt_insert_batch(psvo_dtree *tr, hipStream_t st, const int *vox, int64_t n, int *created_out, bool *changed) {
    const int64_t n_walks = n * 8, ne = n_walks * tr->D;
    PSVO_REQUIRE(ne < (int64_t)1 << 31 && (uint64_t)tr->w_next + (uint64_t)n_walks < 0xffffffffull,
                 "dtree_insert: batch too large (%lld voxels)", (long long)n);
    const int64_t nb = div_up(ne, 1024);
    const int64_t need = 2 * ne + nb + 2;
    if (need > tr->scratch_n) {
        (void)hipStreamSynchronize(st);
        (void)hipFree(tr->scratch);
        if (hipMalloc(&tr->scratch, need * sizeof(int)) != hipSuccess)
            return set_error(PSVO_E_LAUNCH, "dtree_insert: out of device memory");
        tr->scratch_n = need;
    }
    int *flag = tr->scratch, *rank = flag + ne, *totals = rank + ne, *sum = totals + nb, *overflow = sum + 1;
    const dim3 g(div_up(ne, 256)), b(256);
    // table: about 2.4 new nodes per voxel on surface scans; keep load <= 1/2
    // for that and grow (rehash from the node arrays, batch redone) if a
    // probe run still overflows
    uint64_t want = 2 * (uint64_t)(tr->count + 3 * n);
    int ov = 0;
    for (int attempt = 0;; ++attempt) {
        if (want > tr->t.mask + 1) {
            int rc = dt_alloc_table(tr, st, want);
            if (rc) return rc;
        }
        (void)hipMemsetAsync(overflow, 0, sizeof(int), st);
        psvo::launch(k_dt_walk, g, b, 0, st, tr->t, vox, n_walks, tr->D, tr->w_next, overflow);
        if (hipMemcpyAsync(&ov, overflow, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return set_error(PSVO_E_LAUNCH, "dtree_insert: walk failed (%s)", hipGetErrorString(hipGetLastError()));
        if (!(ov & kDtWalkOverflow)) break;
        if (attempt >= 6) return set_error(PSVO_E_OVERFLOW, "dtree_insert: hash table overflow");
        want = 4 * (tr->t.mask + 1);
        int rc = dt_alloc_table(tr, st, want);
        if (rc) return rc;
    }
    psvo::launch(k_dt_flag, g, b, 0, st, tr->t, vox, n_walks, tr->D, tr->w_next, flag);
    psvo::launch(k_dt_scan_local, dim3(nb), dim3(1024), 0, st, flag, ne, rank, totals);
    psvo::launch(k_dt_scan_totals, dim3(1), dim3(1024), 0, st, totals, nb, sum);
    psvo::launch(k_dt_scan_add, dim3(nb), dim3(1024), 0, st, rank, ne, totals);
    int created = 0;
    if (hipMemcpyAsync(&created, sum, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return set_error(PSVO_E_LAUNCH, "dtree_insert: scan failed (%s)", hipGetErrorString(hipGetLastError()));
    if (tr->count + created > tr->cap) {  // node arrays: exactly what this batch creates
        int64_t cap = tr->cap;
        while (cap < tr->count + created) cap *= 2;
        int rc = dt_alloc_nodes(tr, cap, st);
        if (rc) return rc;
    }
    psvo::launch(k_dt_create, g, b, 0, st, tr->t, tr->nd, vox, n_walks, tr->D, tr->shift, tr->size, flag, rank,
                       tr->count);
    psvo::launch(k_dt_link, g, b, 0, st, tr->t, tr->nd, vox, n_walks, tr->D, tr->size, flag);
    tr->count += created;
    tr->w_next += (unsigned)n_walks;
    *created_out = created;
    *changed = created > 0 || (ov & kDtWalkChanged);
    return check_launch("dtree_insert");
}

// psvo_dtree_insert_depth's workspace: a host-only function of (h, w)
struct FrameLayout {
    int64_t n, slots, nb;
    int64_t keys, valid, set_key, set_min, lrank, totals, stats, list, bytes;  // byte offsets, 256-B aligned
};
constexpr int64_t kFrameMaxPix = (int64_t)1 << 24;
bool frame_layout(int h, int w, FrameLayout &L) {
    if (h <= 0 || w <= 0 || (int64_t)h * w > kFrameMaxPix) return false;
    L.n = (int64_t)h * w;
    L.slots = 64;
    while (L.slots < 2 * L.n) L.slots <<= 1;  // load <= 1/2 even if every pixel is its own voxel
    L.nb = (L.n + 1023) / 1024;
    int64_t o = 0;
    auto take = [&o](int64_t bytes) {
        const int64_t at = o;
        o += (bytes + 255) / 256 * 256;
        return at;
    };
    L.keys = take(L.n * 3 * sizeof(int));
    L.valid = take(L.n);
    L.set_key = take(L.slots * sizeof(unsigned long long));  // set_key | set_min: one memset clears both
    L.set_min = take(L.slots * sizeof(unsigned));
    L.lrank = take(L.n * sizeof(int));
    L.totals = take(L.nb * sizeof(int));
    L.stats = take(PSVO_FRAME_STAT_WORDS * sizeof(int));
    L.list = take(L.n * 3 * sizeof(int));
    L.bytes = o;
    return true;
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

void launch_frame_keys(hipStream_t st, int64_t n, const float *depth, const float *dirs, const float *pose,
                       float voxel_size, int *keys, uint8_t *valid, int *stats) {
    const int vec = aligned16(depth) && aligned16(dirs) && aligned16(keys) && (reinterpret_cast<uintptr_t>(valid) & 3) == 0;
    psvo::launch(k_fi_keys, dim3(div_up(div_up(n, 4), 256)), dim3(256), 0, st, n, depth, dirs, pose, voxel_size, keys,
                 valid, vec, stats);
}

}  // namespace

extern "C" int psvo_dtree_insert(void *tree, void *stream, const int *vox, int64_t n) {
    psvo_dtree *tr = static_cast<psvo_dtree *>(tree);
    PSVO_REQUIRE(tr != nullptr && n >= 0 && (n == 0 || vox != nullptr), "dtree_insert: bad arguments");
    if (n == 0) return PSVO_OK;
    int created = 0;
    bool changed = false;
    const int rc = dt_insert_batch(tr, as_stream(stream), vox, n, &created, &changed);
    if (rc == PSVO_OK && changed) ++tr->generation;
    return rc;
}

extern "C" uint64_t psvo_dtree_generation(void *tree) {
    const psvo_dtree *tr = static_cast<const psvo_dtree *>(tree);
    return tr ? tr->generation : 0;
}

extern "C" int psvo_depth_voxel_keys(void *stream, int64_t n_pix, const float *depth, const float *dirs_cam,
                                     const float *pose34, float voxel_size, int *keys, uint8_t *valid) {
    PSVO_REQUIRE(n_pix >= 0 && n_pix <= (int64_t)1 << 31 && voxel_size > 0.f, "depth_voxel_keys: bad arguments");
    if (n_pix == 0) return PSVO_OK;
    PSVO_REQUIRE(depth && dirs_cam && pose34 && keys && valid, "depth_voxel_keys: null pointer");
    launch_frame_keys(as_stream(stream), n_pix, depth, dirs_cam, pose34, voxel_size, keys, valid, nullptr);
    return check_launch("depth_voxel_keys");
}

extern "C" int64_t psvo_dtree_frame_workspace_bytes(int h, int w) {
    FrameLayout L;
    return frame_layout(h, w, L) ? L.bytes : -1;
}

extern "C" int psvo_dtree_insert_depth(void *tree, void *stream, int h, int w, const float *depth,
                                       const float *dirs_cam, const float *pose34, float voxel_size,
                                       int64_t *stats_out) {
    psvo_dtree *tr = static_cast<psvo_dtree *>(tree);
    FrameLayout L;
    PSVO_REQUIRE(tr != nullptr && frame_layout(h, w, L) && depth && dirs_cam && pose34 && voxel_size > 0.f,
                 "dtree_insert_depth: bad arguments (frames of 1 .. 2^24 pixels, device images, voxel_size > 0)");
    hipStream_t st = as_stream(stream);
    if (L.bytes > tr->frame_ws_bytes) {
        (void)hipStreamSynchronize(st);
        (void)hipFree(tr->frame_ws);
        tr->frame_ws = nullptr;
        tr->frame_ws_bytes = 0;
        if (hipMalloc(&tr->frame_ws, L.bytes) != hipSuccess)
            return set_error(PSVO_E_LAUNCH, "dtree_insert_depth: out of device memory (%lld bytes)", (long long)L.bytes);
        tr->frame_ws_bytes = L.bytes;
    }
    char *ws = tr->frame_ws;
    int *keys = reinterpret_cast<int *>(ws + L.keys), *lrank = reinterpret_cast<int *>(ws + L.lrank),
        *totals = reinterpret_cast<int *>(ws + L.totals), *stats = reinterpret_cast<int *>(ws + L.stats),
        *list = reinterpret_cast<int *>(ws + L.list);
    uint8_t *valid = reinterpret_cast<uint8_t *>(ws + L.valid);
    FiSet set{reinterpret_cast<unsigned long long *>(ws + L.set_key), reinterpret_cast<unsigned int *>(ws + L.set_min),
              (uint64_t)L.slots - 1};
    // empty key and "no pixel yet" are both all ones
    (void)hipMemsetAsync(ws + L.set_key, 0xff, L.set_min - L.set_key + L.slots * sizeof(unsigned), st);
    (void)hipMemsetAsync(stats, 0, PSVO_FRAME_STAT_WORDS * sizeof(int), st);
    launch_frame_keys(st, L.n, depth, dirs_cam, pose34, voxel_size, keys, valid, stats);
    psvo::launch(k_fi_set, dim3(div_up(L.n, 256)), dim3(256), 0, st, set, keys, valid, L.n);
    psvo::launch(k_fi_flag, dim3(L.nb), dim3(1024), 0, st, set, tr->t, tr->nd, tr->D, keys, valid, L.n, lrank, totals,
                 stats);
    psvo::launch(k_dt_scan_totals, dim3(1), dim3(1024), 0, st, totals, L.nb, stats + PSVO_FRAME_STAT_NEW);
    psvo::launch(k_fi_compact, dim3(L.nb), dim3(1024), 0, st, keys, lrank, totals, L.n, list);
    int hs[PSVO_FRAME_STAT_WORDS] = {};
    if (hipMemcpyAsync(hs, stats, sizeof(hs), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return set_error(PSVO_E_LAUNCH, "dtree_insert_depth: frame pass failed (%s)", hipGetErrorString(hipGetLastError()));
    const int64_t n_new = hs[PSVO_FRAME_STAT_NEW];
    int64_t created = 0;
    // the stages index a batch's (walk, depth) pairs in 32 bits: a list of
    // survivors longer than that goes in as consecutive batches, which is the
    // same sequential insertion
    const int64_t per_batch = (((int64_t)1 << 31) - 1) / (8 * tr->D);
    for (int64_t at = 0; at < n_new; at += per_batch) {
        int made = 0;
        bool changed = false;
        const int rc = dt_insert_batch(tr, st, list + 3 * at, n_new - at < per_batch ? n_new - at : per_batch, &made, &changed);
        if (rc) return rc;
        created += made;
        if (changed) ++tr->generation;  // every survivor lacks a SURFACE leaf: inserting it makes or promotes one
    }
    if (stats_out) {
        for (int i = 0; i < PSVO_FRAME_STAT_WORDS; ++i) stats_out[i] = hs[i];
        stats_out[PSVO_FRAME_STAT_CREATED] = created;
        stats_out[PSVO_FRAME_STAT_WORKSPACE_BYTES] = L.bytes;
    }
    return PSVO_OK;
}

extern "C" int64_t psvo_dtree_count(void *tree) {
    const psvo_dtree *tr = static_cast<const psvo_dtree *>(tree);
    return tr ? tr->count : -1;
}

extern "C" int64_t psvo_dtree_count_leaves(void *tree, void *stream) {
    psvo_dtree *tr = static_cast<psvo_dtree *>(tree);
    if (!tr) return -1;
    hipStream_t st = as_stream(stream);
    int *out = tr->scratch;
    if (!out) {
        if (hipMalloc(&tr->scratch, 64 * sizeof(int)) != hipSuccess) return -1;
        tr->scratch_n = 64;
        out = tr->scratch;
    }
    (void)hipMemsetAsync(out, 0, sizeof(int), st);
    psvo::launch(k_dt_count_type, dim3(div_up(tr->count, 256)), dim3(256), 0, st, tr->nd.type, tr->count,
                       kDtSurface, out);
    int v = 0;
    (void)hipMemcpyAsync(&v, out, sizeof(int), hipMemcpyDeviceToHost, st);
    if (hipStreamSynchronize(st) != hipSuccess) return -1;
    return v;
}

extern "C" int psvo_dtree_export(void *tree, void *stream, float voxel_size, float *voxels, float *children,
                                 int *features, float *centres, int *structure) {
    psvo_dtree *tr = static_cast<psvo_dtree *>(tree);
    PSVO_REQUIRE(tr != nullptr, "dtree_export: null tree");
    psvo::launch(k_dt_export, dim3(div_up(tr->count, 256)), dim3(256), 0, as_stream(stream), tr->t, tr->nd,
                       tr->count, tr->D, voxel_size, voxels, children, features, centres, structure);
    return check_launch("dtree_export");
}

extern "C" int psvo_dtree_probe(void *tree, void *stream, const int *vox, int64_t n, int corners, int *hit) {
    psvo_dtree *tr = static_cast<psvo_dtree *>(tree);
    PSVO_REQUIRE(tr != nullptr && n >= 0 && (corners == 1 || corners == 8), "dtree_probe: bad arguments");
    if (n == 0) return PSVO_OK;
    psvo::launch(k_dt_probe, dim3(div_up(n * corners, 256)), dim3(256), 0, as_stream(stream), tr->t, vox, n,
                       tr->D, corners, hit);
    return check_launch("dtree_probe");
}
