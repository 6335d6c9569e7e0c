"""Numpy references and input builders for the mesh-cleaning stages
(csrc/mesh_clean.hip), shared by test_mesh_clean_cpu.py (which pins them to
MeshExtractor.downsample_points and scipy's cKDTree) and test_gpu_mesh_clean.py
(which pins the kernels to them).  Nothing here touches the GPU."""
import functools

import numpy as np

CELL = 0.01     # downsample_points' default cell
VOXEL = 0.25    # ball cases: r = VOXEL / 2 = 0.125 is exact in fp32 and fp64
R = VOXEL * 0.5


# ---- references -------------------------------------------------------------
def downsample_ref(points, cell=CELL):
    """downsample_points restated: stable sort by cell key, then per cell the
    sequential fp64 sum (0 + p_i0 + p_i1 + …) in input order, over the count."""
    p = np.asarray(points, np.float64)
    n = p.shape[0]
    if n == 0:
        return p
    key = np.floor((p - p.min(0)) / cell).astype(np.int64)
    order = np.lexsort((key[:, 2], key[:, 1], key[:, 0]))  # stable, x the primary key
    ks = key[order]
    head = np.ones(n, bool)
    head[1:] = (ks[1:] != ks[:-1]).any(1)
    seg = np.cumsum(head) - 1
    pos = np.arange(n)
    rank = pos - np.maximum.accumulate(np.where(head, pos, 0))
    out = np.zeros((seg[-1] + 1, 3))
    by_rank = np.argsort(rank, kind="stable")
    bounds = np.searchsorted(rank[by_rank], np.arange(rank.max() + 2))
    for r in range(rank.max() + 1):  # one member of every cell per pass: plain += is exact here
        sel = by_rank[bounds[r]:bounds[r + 1]]
        out[seg[sel]] = out[seg[sel]] + p[order[sel]]
    return out / np.bincount(seg)[:, None]


def ball_ref(points, verts, r=R, tie=1e-9):
    """Brute force (hit, near_tie) per vertex: hit = ∃j (dx·dx + dy·dy) + dz·dz ≤ r·r
    with d = double(vert) − point; near_tie = ∃j | |d| − r | ≤ tie·r."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    v = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    hit = np.zeros(v.shape[0], bool)
    near = np.zeros(v.shape[0], bool)
    if p.shape[0] == 0:
        return hit, near
    step = max(1, (1 << 22) // p.shape[0])
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(0, v.shape[0], step):
            d = v[a:a + step, None, :] - p[None, :, :]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            hit[a:a + step] = (d2 <= r * r).any(1)
            near[a:a + step] = (np.abs(np.sqrt(d2) - r) <= tie * r).any(1)
    return hit, near


def backproject32(pose, depth, dirs):
    """w_k = ((v0·R_k0 + v1·R_k1) + v2·R_k2) + t_k, v = dir·depth, every
    operation rounded to fp32 (numpy rounds each fp32 operation on its own)."""
    P = np.asarray(pose, np.float32)
    d = np.asarray(depth, np.float32).reshape(-1)
    v = np.asarray(dirs, np.float32).reshape(-1, 3) * d[:, None]
    out = np.empty((d.shape[0], 3), np.float32)
    for k in range(3):
        out[:, k] = ((v[:, 0] * P[k, 0] + v[:, 1] * P[k, 1]) + v[:, 2] * P[k, 2]) + P[k, 3]
    return out


def backproject64(pose, depth, dirs):
    """The same formula in fp64 from the fp32 inputs, and the bound's scale
    |v0 R_k0| + |v1 R_k1| + |v2 R_k2| + |t_k|."""
    P = np.asarray(pose, np.float32).astype(np.float64)
    d = np.asarray(depth, np.float32).reshape(-1).astype(np.float64)
    v = np.asarray(dirs, np.float32).reshape(-1, 3).astype(np.float64) * d[:, None]
    ref = v @ P[:3, :3].T + P[:3, 3]
    scale = np.abs(v) @ np.abs(P[:3, :3]).T + np.abs(P[:3, 3])
    return ref, scale


# ---- back-projection inputs ---------------------------------------------------
def general_frame(h=37, w=53, seed=0):
    """(pose f32 [4,4], depth f32 [h,w] with zeros, dirs f32 [h,w,3])."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    pose = np.eye(4, dtype=np.float32)
    pose[:3, :3] = q
    pose[:3, 3] = rng.uniform(-3, 12, 3)
    iy, ix = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    dirs = np.stack([(ix - w / 2) / 40.0, (iy - h / 2) / 40.0, np.ones_like(ix, float)], -1).astype(np.float32)
    depth = rng.uniform(0.5, 4.0, (h, w)).astype(np.float32)
    depth[rng.random((h, w)) < 0.05] = 0.0
    return pose, depth, dirs


def accumulate_frames(n=3, h=37, w=53):
    """Overlapping views of one wall (so later calls re-bin earlier means and the
    minimum moves): [(pose, depth, dirs)]."""
    out = []
    for i in range(n):
        pose, depth, dirs = general_frame(h, w, seed=10 + i)
        pose[:3, :3] = np.eye(3, dtype=np.float32)
        pose[:3, 3] = np.float32([1.0 - 0.07 * i, 2.0 + 0.03 * i, -0.5])
        depth = (1.0 + 0.02 * np.sin(np.arange(h * w).reshape(h, w) * (0.1 + i))).astype(np.float32)
        depth[::9, ::7] = 0.0
        out.append((pose, depth, dirs * np.float32(0.25)))
    return out


# ---- downsample inputs --------------------------------------------------------
@functools.lru_cache(maxsize=None)
def downsample_cases():
    """name → f64 [N, 3] (treat as read-only)."""
    rng = np.random.default_rng(7)
    cases = {"one": np.array([[0.3, -1.7, 2.9]])}
    # 4099 points: one cell of 1100, six cells of 70-100, the rest spread thin; members interleaved
    parts = []
    origin = np.array([2.0, -1.0, 0.5])
    for cell_id, count in [((3, 4, 5), 1100), ((0, 0, 1), 70), ((9, 2, 2), 81), ((9, 2, 3), 93),
                           ((20, 20, 20), 100), ((21, 20, 20), 77), ((40, 1, 7), 65)]:
        parts.append(origin + (np.array(cell_id) + rng.uniform(0.1, 0.9, (count, 3))) * CELL)
    rest = 4099 - sum(x.shape[0] for x in parts) - 1
    parts.append(origin + rng.uniform(0.0, 0.5, (rest, 3)))
    parts.append(origin[None])  # pins the minimum: the cells above are where they say
    pts = np.concatenate(parts, 0)
    cases["clustered"] = pts[rng.permutation(pts.shape[0])]
    assert cases["clustered"].shape[0] == 4099
    # exactly on cell boundaries (m + k·cell as fp64 computes it: the quotient lands on either side of k), and the minimum itself, repeated
    m = np.array([-0.32, 0.16, 0.64])
    k = rng.integers(0, 60, (600, 3))
    on = m + k * CELL
    on2 = (m + k[:200] * (CELL / 2)) + k[:200] * (CELL / 2)  # a second rounding of the same boundaries
    cases["boundaries"] = np.concatenate([np.repeat(m[None], 5, 0), on, on2, np.nextafter(on[:100], -np.inf),
                                          np.nextafter(on[:100], np.inf)], 0)[rng.permutation(1005)]
    cases["negative"] = np.concatenate([rng.uniform(-3.0, -2.6, (700, 3)), rng.uniform(-0.2, 0.2, (700, 3)) - [2.8, 2.8, 2.8],
                                        -rng.uniform(0, 0.05, (300, 3))], 0)
    base = rng.uniform(0.0, 0.3, (300, 3))
    dup = np.concatenate([base] * 5 + [np.nextafter(base, np.inf), np.zeros((3, 3)), -np.zeros((3, 3))], 0)
    cases["duplicates"] = dup[rng.permutation(dup.shape[0])]
    for v in cases.values():
        v.setflags(write=False)
    return cases


# ---- ball inputs -------------------------------------------------------------
def _f32(x):
    return np.asarray(x, np.float32)


@functools.lru_cache(maxsize=None)
def ball_cases():
    """name → (points f64 [M, 3], verts f32 [V, 3]); r = R.  Every case has hits and misses."""
    rng = np.random.default_rng(11)
    cases = {}
    # a lone point: exactly r away hits, the next fp32 above misses (all values exact binary fractions)
    p = np.array([[1.0, 2.0, 3.0]])
    up = np.nextafter(np.float32(1.0 + R), np.float32(np.inf))
    dn = np.nextafter(np.float32(2.0 - R), np.float32(-np.inf))
    cases["exact_r"] = (p, _f32([[1.0 + R, 2.0, 3.0], [up, 2.0, 3.0], [1.0, 2.0 - R, 3.0], [1.0, dn, 3.0],
                                 [1.0, 2.0, 3.0 - R], [1.0 + R, 2.0 + R, 3.0]]))
    # the only hit in each of the 26 neighbouring coarse cells (and the vertex's own), then vertices with none;
    # the anchor point at g0 pins the cells' origin
    g0 = np.array([-4.0, 8.0, 0.5])
    pts, vs = [g0], []
    offs = [(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1)]
    for i, o in enumerate(offs):
        centre = g0 + (np.array([8 * (i + 1), 8, 8]) + 0.5) * R
        vs.append(centre)
        pts.append(centre + np.array(o) * 0.55 * R)
    for i in range(14):
        vs.append(g0 + (np.array([8 * (i + 1) + 4, 8, 8]) + 0.5) * R)
    cases["neighbours"] = (np.array(pts), _f32(vs))
    cases["negative"] = (rng.uniform(-3.0, -1.0, (800, 3)), _f32(rng.uniform(-3.2, -0.8, (500, 3))))
    # vertices far outside the points' bounds, on both sides
    pf = rng.uniform(0.0, 1.0, (200, 3))
    far = _f32([[1e6, 0.5, 0.5], [-1e6, 0.5, 0.5], [0.5, 1e30, 0.5], [0.5, 0.5, -1e30], [3e38, 3e38, 3e38],
                [-3e38, 0.5, 0.5], [0.5, -70000.0, 0.5], [2.0 ** 21 * R, 0.5, 0.5], [0.5, 0.5, 2.0 ** 22 * R]])
    cases["far"] = (pf, np.concatenate([far, _f32(rng.uniform(0.0, 1.0, (10, 3))), _f32(rng.uniform(-9, -8, (3, 3)))], 0))
    # one coarse cell with 1500 points
    cases["dense_cell"] = (5.0 + rng.uniform(0.0, R, (1500, 3)), _f32(5.0 + rng.uniform(-1.5 * R, 2.5 * R, (600, 3))))
    # 21952 distinct coarse cells
    g = np.stack(np.meshgrid(*[np.arange(28)] * 3, indexing="ij"), -1).reshape(-1, 3)
    many = -2.0 + g * (2.25 * R) + rng.uniform(0.05, 0.95, (g.shape[0], 3)) * R
    cases["many_cells"] = (many[rng.permutation(many.shape[0])], _f32(rng.uniform(-2.2, -2.0 + 28 * 2.25 * R + 0.2, (2000, 3))))
    cases["random"] = (rng.uniform(0.0, 4.0, (7500, 3)), _f32(rng.uniform(-0.1, 4.1, (3000, 3))))
    for a, b in cases.values():
        a.setflags(write=False)
        b.setflags(write=False)
    return cases


@functools.lru_cache(maxsize=None)
def ball_expected(name):
    """(hit, near_tie) of a ball case, computed once."""
    p, v = ball_cases()[name]
    return ball_ref(p, v, R)


# ---- end-to-end frames (fp32 back-projection exact under any operation order) ------------
def exact_frame(which, shift=0, h=64, w=96):
    """A camera inside room0 facing the wall x = 18 (which = 0) or y = 10
    (which = 1): the rotation is a signed axis permutation, t, dirs and depth
    are multiples of 2⁻⁶ with |dirs| < 8 and depth in [1, 4).  Returns (pose f32
    [4,4], depth f32 [h,w], dirs f32 [h,w,3]); `shift` moves the camera sideways
    by shift·2⁻⁶ so successive frames overlap."""
    iy, ix = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    dirs = np.stack([(ix - w // 2) / 64.0, (iy - h // 2) / 64.0, np.ones_like(ix, float)], -1).astype(np.float32)
    depth = (3.5 + ((ix * 7 + iy * 3 + which) % 5) / 64.0).astype(np.float32)
    pose = np.eye(4, dtype=np.float32)
    if which == 0:   # camera z → +x, x → −y, y → −z
        pose[:3, :3] = [[0, 0, 1], [-1, 0, 0], [0, -1, 0]]
        pose[:3, 3] = [14.5, 13.0 + shift / 64.0, 11.5]
    else:            # camera z → −y, x → −x, y → −z
        pose[:3, :3] = [[-1, 0, 0], [0, 0, -1], [0, -1, 0]]
        pose[:3, 3] = [14.0 + shift / 64.0, 13.5, 11.5]
    assert (dirs * 64 == np.round(dirs * 64)).all() and np.abs(dirs).max() < 8
    assert (depth * 64 == np.round(depth * 64)).all() and depth.min() >= 1 and depth.max() < 4
    return pose, depth, dirs
