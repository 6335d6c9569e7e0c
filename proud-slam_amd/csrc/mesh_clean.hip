// Mesh cleaning on the device (the clean_mseh branch).
//
// Reference: MeshExtractor.create_mesh with clean_mseh=True (mesh_util.py:
// 80-147): back-project the depth frame (get_valid_points), re-bin every
// accumulated depth point into 1-cm cells and keep each cell's mean
// (downsample_points, the project's restatement of open3d voxel_down_sample),
// then keep the faces with a vertex within voxel_size/2 of a depth point
// (cKDTree.query_ball_point).  Three stages, one entry point each:
//   psvo_mesh_depth_points      w = R·(dir·depth) + t in fp32 (fi_pixel_key's
//                               operation order, octree_gpu.hip), widened to fp64
//   psvo_mesh_points_downsample per-axis minimum → cell key floor((p − m)/cell)
//                               packed 3 × 21 bits → stable radix sort of
//                               (key, index) → per cell the in-order sum
//                               (0 + p_i0 + p_i1 + …)/count: np.unique +
//                               np.add.at bit for bit, no atomic order anywhere
//   psvo_mesh_ball_any          points sorted by coarse cell; per vertex nine
//                               binary searches (the three z-neighbours of an
//                               (x, y) column are one contiguous key range),
//                               fp64 distance test, out at the first hit
// The sorts and the scan are rocPRIM's (radix_sort_pairs is stable); the key,
// grouping, mean and ball kernels are this file's.
#pragma clang fp contract(off)

#include <cstring>  // before rocprim: its headers use memset unqualified

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "psvo_common.h"

namespace psvo {
namespace {

constexpr int kCellBits = 21;
constexpr int64_t kCellMax = (int64_t)1 << kCellBits;  // cells per axis a key can hold
constexpr int kShortSeg = 32;                          // longer cells are summed by a whole wave
constexpr int kLongBlocks = 256;

// status bits of a call (the control words below)
constexpr unsigned kBadValue = 1u, kBadExtent = 2u;

// control words at the head of a workspace: the per-axis minimum as ordered
// u64, the status bits and the long-cell count
struct Ctl {
    unsigned long long mn[3];
    unsigned status;
    unsigned n_long;
};

constexpr size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

// doubles ↔ u64 whose unsigned order is the doubles' order
__device__ __forceinline__ unsigned long long ord_of(double d) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(d);
    return (b >> 63) ? ~b : b | 0x8000000000000000ull;
}
__device__ __forceinline__ double ord_to(unsigned long long u) {
    const unsigned long long b = (u >> 63) ? u & 0x7fffffffffffffffull : ~u;
    return __longlong_as_double((long long)b);
}

__global__ __launch_bounds__(256) void k_depth_points(int64_t n, const float *__restrict__ depth,
                                                      const float *__restrict__ dirs, const float *__restrict__ pose,
                                                      double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float d = depth[i];
    const float v0 = dirs[3 * i] * d, v1 = dirs[3 * i + 1] * d, v2 = dirs[3 * i + 2] * d;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float p0 = v0 * pose[4 * k], p1 = v1 * pose[4 * k + 1], p2 = v2 * pose[4 * k + 2];
        const float wk = ((p0 + p1) + p2) + pose[4 * k + 3];
        out[3 * i + k] = (double)wk;
    }
}

// per-axis minimum of the finite points (order-free: a minimum), non-finite flagged
__global__ __launch_bounds__(256) void k_points_min(int64_t n, const double *__restrict__ p, Ctl *__restrict__ ctl) {
    unsigned long long m[3] = {~0ull, ~0ull, ~0ull};
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double x = p[3 * i + a];
            if (isfinite(x)) {
                const unsigned long long o = ord_of(x);
                m[a] = o < m[a] ? o : m[a];
            } else {
                bad = true;
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            const unsigned long long o = __shfl_xor(m[a], s, 64);
            m[a] = o < m[a] ? o : m[a];
        }
    }
    if ((threadIdx.x & 63) == 0)
        for (int a = 0; a < 3; ++a)
            if (m[a] != ~0ull) atomicMin(&ctl->mn[a], m[a]);
    if (bad) atomicOr(&ctl->status, kBadValue);
}

// key = floor((p − m)/cell) per axis (fp64, IEEE division), packed x·2⁴² + y·2²¹ + z:
// its unsigned order is the lexicographic (x, y, z) order np.unique(axis=0) gives
__global__ __launch_bounds__(256) void k_points_keys(int64_t n, const double *__restrict__ p, double cell,
                                                     Ctl *__restrict__ ctl, unsigned long long *__restrict__ keys,
                                                     unsigned *__restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    unsigned long long key = 0;
    unsigned bad = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double m = ord_to(ctl->mn[a]);
        const double f = floor((p[3 * i + a] - m) / cell);
        long long c = 0;
        if (!(f >= 0.0 && f < (double)kCellMax))  // also a non-finite quotient
            bad |= isfinite(p[3 * i + a]) ? kBadExtent : kBadValue;
        else
            c = (long long)f;
        key = (key << kCellBits) | (unsigned long long)c;
    }
    if (bad) atomicOr(&ctl->status, bad);
    keys[i] = key;
    idx[i] = (unsigned)i;
}

__global__ __launch_bounds__(256) void k_heads(int64_t n, const unsigned long long *__restrict__ keys,
                                               unsigned *__restrict__ head) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    head[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
}

// one lane per sorted position; a cell's first position sums its members in
// sorted (= input index) order when there are at most kShortSeg, else hands
// the cell to k_cell_mean_long.  The last position writes the count word:
// the distinct cells, or −status when the input was refused.
__global__ __launch_bounds__(256) void k_cell_mean(int64_t n, const double *__restrict__ p,
                                                   const unsigned *__restrict__ idx,
                                                   const unsigned *__restrict__ head,
                                                   const unsigned *__restrict__ seg, Ctl *__restrict__ ctl,
                                                   unsigned *__restrict__ long_list, double *__restrict__ out,
                                                   int64_t *__restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (i == n - 1) *count = ctl->status ? -(int64_t)ctl->status : (int64_t)seg[n - 1];
    if (!head[i]) return;
    int64_t end = i + 1;
    const int64_t lim = i + kShortSeg < n ? i + kShortSeg : n;
    while (end < lim && !head[end]) ++end;
    if (end < n && !head[end]) {  // more than kShortSeg members
        long_list[atomicAdd(&ctl->n_long, 1u)] = (unsigned)i;
        return;
    }
    double s[3] = {0.0, 0.0, 0.0};
    for (int64_t j = i; j < end; ++j) {
        const int64_t q = idx[j];
#pragma unroll
        for (int a = 0; a < 3; ++a) s[a] = s[a] + p[3 * q + a];
    }
    const double cnt = (double)(end - i);
    const int64_t row = (int64_t)seg[i] - 1;
#pragma unroll
    for (int a = 0; a < 3; ++a) out[3 * row + a] = s[a] / cnt;
}

// one wave per long cell: 64 members loaded at a time, added in order by
// every lane alike (the lanes' values read with wave-uniform shuffles)
__global__ __launch_bounds__(256) void k_cell_mean_long(int64_t n, const double *__restrict__ p,
                                                        const unsigned *__restrict__ idx,
                                                        const unsigned *__restrict__ head,
                                                        const unsigned *__restrict__ seg, const Ctl *__restrict__ ctl,
                                                        const unsigned *__restrict__ long_list,
                                                        double *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const unsigned n_waves = gridDim.x * (blockDim.x >> 6);
    const unsigned n_long = ctl->n_long;
    for (unsigned w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); w < n_long; w += n_waves) {
        const int64_t first = long_list[w];
        double s[3] = {0.0, 0.0, 0.0};
        int64_t members = 0;
        for (int64_t base = first;; base += 64) {
            const int64_t j = base + lane;
            const bool stop = j >= n || (j > first && head[j]);
            const unsigned long long stops = __ballot(stop);
            const int take = stops ? __builtin_ctzll(stops) : 64;
            double x[3] = {0.0, 0.0, 0.0};
            if (lane < take) {
                const int64_t q = idx[j];
#pragma unroll
                for (int a = 0; a < 3; ++a) x[a] = p[3 * q + a];
            }
            for (int t = 0; t < take; ++t) {
#pragma unroll
                for (int a = 0; a < 3; ++a) s[a] = s[a] + __shfl(x[a], t, 64);
            }
            members += take;
            if (take < 64) break;
        }
        if (lane == 0) {
            const double cnt = (double)members;
            const int64_t row = (int64_t)seg[first] - 1;
#pragma unroll
            for (int a = 0; a < 3; ++a) out[3 * row + a] = s[a] / cnt;
        }
    }
}

// ---- ball query ---------------------------------------------------------------
// Coarse cells of side h = r·(1 + 2⁻²⁰) from the points' minimum m.  A pair
// the test accepts has |d| ≤ r·(1 + 2⁻⁵¹) per axis, i.e. at most 1 − 2⁻²¹ cells
// apart, and a computed cell coordinate below 2²¹ is off by less than 2⁻³⁰:
// the floors differ by at most one, so the 27 neighbours hold every hit.
__device__ __forceinline__ double coarse_coord(double x, double m, double h) { return floor((x - m) / h); }

__global__ __launch_bounds__(256) void k_ball_gather(int64_t m, const double *__restrict__ p,
                                                     const unsigned *__restrict__ idx, double *__restrict__ sorted) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int64_t q = idx[i];
#pragma unroll
    for (int a = 0; a < 3; ++a) sorted[3 * i + a] = p[3 * q + a];
}

__global__ __launch_bounds__(256) void k_ball_any(int64_t m, const unsigned long long *__restrict__ keys,
                                                  const double *__restrict__ sorted, int64_t n_verts,
                                                  const float *__restrict__ verts, double r, double h,
                                                  const Ctl *__restrict__ ctl, uint8_t *__restrict__ hit,
                                                  int64_t *__restrict__ status) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v == 0) *status = -(int64_t)ctl->status;
    if (v >= n_verts) return;
    const double x[3] = {(double)verts[3 * v], (double)verts[3 * v + 1], (double)verts[3 * v + 2]};
    double c[3];
    bool near = ctl->status == 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        c[a] = coarse_coord(x[a], ord_to(ctl->mn[a]), h);
        near = near && c[a] >= -1.0 && c[a] <= (double)kCellMax;  // false for a NaN
    }
    bool found = false;
    if (near) {
        const long long cx = (long long)c[0], cy = (long long)c[1], cz = (long long)c[2];
        const long long z0 = cz - 1 < 0 ? 0 : cz - 1, z1 = cz + 1 > kCellMax - 1 ? kCellMax - 1 : cz + 1;
        const double r2 = r * r;
        for (int n9 = 0; n9 < 9 && !found && z0 <= z1; ++n9) {
            const long long nx = cx + n9 / 3 - 1, ny = cy + n9 % 3 - 1;
            if (nx < 0 || nx >= kCellMax || ny < 0 || ny >= kCellMax) continue;
            const unsigned long long col = ((unsigned long long)nx << (2 * kCellBits)) |
                                           ((unsigned long long)ny << kCellBits);
            const unsigned long long k0 = col | (unsigned long long)z0, k1 = col | (unsigned long long)z1;
            int64_t lo = 0, hi = m;  // the first sorted point with key >= k0
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (keys[mid] < k0)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            for (int64_t j = lo; j < m && keys[j] <= k1; ++j) {
                const double dx = x[0] - sorted[3 * j], dy = x[1] - sorted[3 * j + 1], dz = x[2] - sorted[3 * j + 2];
                if ((dx * dx + dy * dy) + dz * dz <= r2) {
                    found = true;
                    break;
                }
            }
        }
    }
    hit[v] = found ? 1 : 0;
}

// workspace layouts (256-byte aligned parts after the control words)
struct DownWs {
    Ctl *ctl;
    unsigned long long *keys_in, *keys_out;
    unsigned *idx_in, *idx_out, *head, *seg, *long_list;
    void *tmp;
    size_t tmp_bytes, total;
};

hipError_t sort_pairs(void *tmp, size_t &bytes, unsigned long long *kin, unsigned long long *kout, unsigned *vin,
                      unsigned *vout, int64_t n, hipStream_t st) {
    return rocprim::radix_sort_pairs(tmp, bytes, kin, kout, vin, vout, (size_t)n, 0u, (unsigned)(3 * kCellBits), st);
}

hipError_t scan_heads(void *tmp, size_t &bytes, unsigned *in, unsigned *out, int64_t n, hipStream_t st) {
    return rocprim::inclusive_scan(tmp, bytes, in, out, (size_t)n, rocprim::plus<unsigned>(), st);
}

bool down_layout(int64_t n, void *base, DownWs &w) {
    size_t sort_b = 0, scan_b = 0;
    if (sort_pairs(nullptr, sort_b, nullptr, nullptr, nullptr, nullptr, n, nullptr) != hipSuccess) return false;
    if (scan_heads(nullptr, scan_b, nullptr, nullptr, n, nullptr) != hipSuccess) return false;
    w.tmp_bytes = sort_b > scan_b ? sort_b : scan_b;
    char *b = static_cast<char *>(base);
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char *q = b + off;
        off += align_up(bytes);
        return q;
    };
    w.ctl = reinterpret_cast<Ctl *>(take(sizeof(Ctl)));
    w.keys_in = reinterpret_cast<unsigned long long *>(take((size_t)n * 8));
    w.keys_out = reinterpret_cast<unsigned long long *>(take((size_t)n * 8));
    w.idx_in = reinterpret_cast<unsigned *>(take((size_t)n * 4));
    w.idx_out = reinterpret_cast<unsigned *>(take((size_t)n * 4));
    w.head = reinterpret_cast<unsigned *>(take((size_t)n * 4));
    w.seg = reinterpret_cast<unsigned *>(take((size_t)n * 4));
    w.long_list = reinterpret_cast<unsigned *>(take(((size_t)n / kShortSeg + 1) * 4));
    w.tmp = take(w.tmp_bytes);
    w.total = off;
    return true;
}

struct BallWs {
    Ctl *ctl;
    unsigned long long *keys_in, *keys_out;
    unsigned *idx_in, *idx_out;
    double *sorted;
    void *tmp;
    size_t tmp_bytes, total;
};

bool ball_layout(int64_t m, void *base, BallWs &w) {
    w.tmp_bytes = 0;
    if (sort_pairs(nullptr, w.tmp_bytes, nullptr, nullptr, nullptr, nullptr, m, nullptr) != hipSuccess) return false;
    char *b = static_cast<char *>(base);
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char *q = b + off;
        off += align_up(bytes);
        return q;
    };
    w.ctl = reinterpret_cast<Ctl *>(take(sizeof(Ctl)));
    w.keys_in = reinterpret_cast<unsigned long long *>(take((size_t)m * 8));
    w.keys_out = reinterpret_cast<unsigned long long *>(take((size_t)m * 8));
    w.idx_in = reinterpret_cast<unsigned *>(take((size_t)m * 4));
    w.idx_out = reinterpret_cast<unsigned *>(take((size_t)m * 4));
    w.sorted = reinterpret_cast<double *>(take((size_t)m * 24));
    w.tmp = take(w.tmp_bytes);
    w.total = off;
    return true;
}

// minimum → keys → stable sort; false: a HIP call failed
bool keys_sorted(hipStream_t st, int64_t n, const double *p, double cell, Ctl *ctl, unsigned long long *kin,
                 unsigned long long *kout, unsigned *vin, unsigned *vout, void *tmp, size_t tmp_bytes) {
    // minimum words: all ones (no point yet); status and long count: 0
    if (hipMemsetAsync(ctl, 0xFF, sizeof(ctl->mn), st) != hipSuccess) return false;
    if (hipMemsetAsync(&ctl->status, 0, 2 * sizeof(unsigned), st) != hipSuccess) return false;
    const int blocks = div_up(n, 256);
    psvo::launch(k_points_min, dim3(blocks < 2048 ? blocks : 2048), dim3(256), 0, st, n, p, ctl);
    psvo::launch(k_points_keys, dim3(blocks), dim3(256), 0, st, n, p, cell, ctl, kin, vin);
    return sort_pairs(tmp, tmp_bytes, kin, kout, vin, vout, n, st) == hipSuccess;
}

constexpr int64_t kMaxPoints = ((int64_t)1 << 31) - 1 - 256;  // u32 indices, int grids of 256 threads

}  // namespace
}  // namespace psvo

using namespace psvo;

extern "C" int psvo_mesh_depth_points(void *stream, int64_t n, const float *depth, const float *dirs,
                                      const float *pose, double *out) {
    PSVO_REQUIRE(n >= 0 && n <= kMaxPoints, "mesh_depth_points: bad pixel count %lld", (long long)n);
    if (n == 0) return PSVO_OK;
    PSVO_REQUIRE(depth && dirs && pose && out, "mesh_depth_points: null pointer");
    psvo::launch(k_depth_points, dim3(div_up(n, 256)), dim3(256), 0, as_stream(stream), n, depth, dirs, pose, out);
    return check_launch("mesh_depth_points");
}

extern "C" int64_t psvo_mesh_downsample_workspace_bytes(int64_t n) {
    DownWs w{};
    if (n <= 0 || n > kMaxPoints || !down_layout(n, nullptr, w)) return -1;
    return (int64_t)w.total;
}

extern "C" int psvo_mesh_points_downsample(void *stream, int64_t n, const double *points, double cell,
                                           void *workspace, double *out, int64_t *count) {
    PSVO_REQUIRE(n > 0 && n <= kMaxPoints, "mesh_points_downsample: bad point count %lld", (long long)n);
    PSVO_REQUIRE(cell > 0.0 && cell < 1e300, "mesh_points_downsample: bad cell size");
    PSVO_REQUIRE(points && workspace && out && count, "mesh_points_downsample: null pointer");
    DownWs w{};
    PSVO_REQUIRE(down_layout(n, workspace, w), "mesh_points_downsample: workspace query failed");
    hipStream_t st = as_stream(stream);
    if (!keys_sorted(st, n, points, cell, w.ctl, w.keys_in, w.keys_out, w.idx_in, w.idx_out, w.tmp, w.tmp_bytes))
        return set_error(PSVO_E_LAUNCH, "mesh_points_downsample: sort failed");
    const int blocks = div_up(n, 256);
    psvo::launch(k_heads, dim3(blocks), dim3(256), 0, st, n, w.keys_out, w.head);
    if (scan_heads(w.tmp, w.tmp_bytes, w.head, w.seg, n, st) != hipSuccess)
        return set_error(PSVO_E_LAUNCH, "mesh_points_downsample: scan failed");
    psvo::launch(k_cell_mean, dim3(blocks), dim3(256), 0, st, n, points, w.idx_out, w.head, w.seg, w.ctl,
                 w.long_list, out, count);
    psvo::launch(k_cell_mean_long, dim3(kLongBlocks), dim3(256), 0, st, n, points, w.idx_out, w.head, w.seg, w.ctl,
                 w.long_list, out);
    return check_launch("mesh_points_downsample");
}

extern "C" int psvo_mesh_points_status(int64_t word) {
    if (word >= 0) return PSVO_OK;
    if ((-word) & kBadValue) return set_error(PSVO_E_INVALID, "mesh points: a coordinate is not finite");
    return set_error(PSVO_E_INVALID, "mesh points: the points span %lld cells or more on an axis",
                     (long long)kCellMax);
}

extern "C" int64_t psvo_mesh_ball_workspace_bytes(int64_t m) {
    BallWs w{};
    if (m <= 0 || m > kMaxPoints || !ball_layout(m, nullptr, w)) return -1;
    return (int64_t)w.total;
}

extern "C" int psvo_mesh_ball_any(void *stream, int64_t m, const double *points, int64_t n_verts, const float *verts,
                                  double radius, void *workspace, uint8_t *hit, int64_t *status) {
    PSVO_REQUIRE(m >= 0 && m <= kMaxPoints && n_verts >= 0 && n_verts <= kMaxPoints, "mesh_ball_any: bad sizes");
    PSVO_REQUIRE(radius > 0.0 && radius < 1e300, "mesh_ball_any: bad radius");
    PSVO_REQUIRE(status, "mesh_ball_any: null pointer");
    hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(status, 0, sizeof(int64_t), st) != hipSuccess)
        return set_error(PSVO_E_LAUNCH, "mesh_ball_any: memset failed");
    if (n_verts == 0) return PSVO_OK;
    PSVO_REQUIRE(verts && hit, "mesh_ball_any: null pointer");
    if (m == 0) {
        if (hipMemsetAsync(hit, 0, (size_t)n_verts, st) != hipSuccess)
            return set_error(PSVO_E_LAUNCH, "mesh_ball_any: memset failed");
        return PSVO_OK;
    }
    PSVO_REQUIRE(points && workspace, "mesh_ball_any: null pointer");
    BallWs w{};
    PSVO_REQUIRE(ball_layout(m, workspace, w), "mesh_ball_any: workspace query failed");
    const double h = radius * (1.0 + 1.0 / 1048576.0);
    if (!keys_sorted(st, m, points, h, w.ctl, w.keys_in, w.keys_out, w.idx_in, w.idx_out, w.tmp, w.tmp_bytes))
        return set_error(PSVO_E_LAUNCH, "mesh_ball_any: sort failed");
    psvo::launch(k_ball_gather, dim3(div_up(m, 256)), dim3(256), 0, st, m, points, w.idx_out, w.sorted);
    psvo::launch(k_ball_any, dim3(div_up(n_verts, 256)), dim3(256), 0, st, m, w.keys_out, w.sorted, n_verts, verts,
                 radius, h, w.ctl, hit, status);
    return check_launch("mesh_ball_any");
}
