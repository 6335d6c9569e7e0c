"""Shared inputs and the reference of the covisibility tests
(test_covis_cpu.py, test_gpu_covis.py).

visible_ref forms a frame's rays with the arithmetic include/psvo.h pins
(torch-CPU elementwise ops: every product and sum rounded to fp32 on its own,
as frame_insert_case.restated_keys does for points), walks them through the
CPU oracle's DFS with a cap no ray reaches (n_max = 256, asserted), applies
the two depth tests in fp32 and sets the bits.  t_in is the oracle's bit for
bit, so every comparison against it is exact.

Case A: frame_insert_case.frames() — synthetic room0, 4 frames of 170 x 300 —
on the tree after all four, truncation 0.1, max_distance 10.
Case B: a row of 80 voxels (20 + i, 30, 40), voxel size 0.2, and one ray
along it: t_in = 0.95 + 0.2 i, no value on a tie.  Depth 20: exactly
i <= 45 (max_distance decides); depth 5: i <= 20 (the depth bound decides).
The reference's 50-leaf cap keeps the 50 FARTHEST voxels of that row.
"""
import functools

import numpy as np
import torch

import frame_insert_case as C
from oracle import oracle as O

TRUNCATION = 0.1
MAX_DISTANCE = 10.0
N_MAX = 256

# Case A, counted on the CPU with the oracle (visible_ref)
A_NODES = 7427
A_MAX_HITS = 12
A_SIZES = {1: (681, 1570, 579, 376), 4: (665, 1508, 565, 373)}
A_INTER = {1: {(0, 2): 520, (1, 3): 92}, 4: {(0, 2): 502, (1, 3): 82}}  # every other pair: 0


def words_of(n_nodes):
    return (int(n_nodes) + 31) // 32


def frame_rays(depth, rays_d, pose, px_step):
    """(o f32[n,3], d f32[n,3], depth f32[n]) of the frame's contributing
    pixels (y % px_step == 0, x % px_step == 0, depth > 0) in pixel order."""
    depth = torch.as_tensor(depth, dtype=torch.float32).cpu()
    c = torch.as_tensor(rays_d, dtype=torch.float32).cpu()[::px_step, ::px_step].reshape(-1, 3)
    z = depth[::px_step, ::px_step].reshape(-1)
    pose = torch.as_tensor(pose, dtype=torch.float32).cpu()
    R, t = pose[:3, :3], pose[:3, 3]
    cols = []
    for j in range(3):  # (c0·R[j][0] + c1·R[j][1]) + c2·R[j][2], each op rounded to fp32
        s = c[:, 0] * R[j, 0]
        s = s + c[:, 1] * R[j, 1]
        s = s + c[:, 2] * R[j, 2]
        cols.append(s)
    d = torch.stack(cols, -1)
    keep = z > 0  # NaN: False
    o = t[None].expand(d.shape[0], 3)
    return o[keep].contiguous().numpy(), d[keep].contiguous().numpy(), z[keep].contiguous().numpy()


def rays_visible_ref(o, d, z, centres, structure, voxel_size, truncation, max_distance, n_max=N_MAX):
    """(u32 words, max hits per ray) of explicit rays with per-ray depth z."""
    centres = np.ascontiguousarray(centres, np.float32)
    structure = np.ascontiguousarray(structure, np.int32)
    words = np.zeros(words_of(centres.shape[0]), np.uint32)
    if o.shape[0] == 0:
        return words, 0
    idx, t0, _, _ = O.svo_intersect_flat(o, d, centres, structure, voxel_size, n_max=n_max)
    hits = (idx != -1).sum(1)
    if n_max >= N_MAX:
        assert int(hits.max()) < n_max, "a ray reached the cap: the reference would not be cap-free"
    bound = z.astype(np.float32) + np.float32(truncation)  # one fp32 add
    ok = (idx != -1) & (t0 <= bound[:, None]) & ~(t0 > np.float32(max_distance))
    v = np.unique(idx[ok]).astype(np.int64)
    np.bitwise_or.at(words, v >> 5, (np.uint32(1) << (v & 31).astype(np.uint32)))
    return words, int(hits.max())


def visible_ref(frame, ms, voxel_size, truncation=TRUNCATION, max_distance=MAX_DISTANCE, px_step=4):
    """The visible set of (depth, rays_d, pose) on the CPU map_states' tree, as u32 words."""
    o, d, z = frame_rays(*frame, px_step)
    return rays_visible_ref(o, d, z, ms["voxel_center_xyz"].numpy(), ms["voxel_structure"].numpy(), voxel_size,
                            truncation, max_distance)[0]


def popcount(words):
    return int(np.unpackbits(np.ascontiguousarray(words).view(np.uint8)).sum())


def ids_of(words):
    return np.flatnonzero(np.unpackbits(np.ascontiguousarray(words, np.uint32).view(np.uint8), bitorder="little"))


@functools.lru_cache(maxsize=None)
def case_a_tree(shift=0.0):
    """CPU map_states arrays of the tree after all four frames."""
    return C.reference(shift)[-1][3]


def case_a_frames(shift=0.0):
    return [(d, r, C.shifted(p, shift) if shift else p) for d, r, p in C.frames()]


@functools.lru_cache(maxsize=None)
def case_a_ref(px_step, shift=0.0):
    """u32 [4, words]: the four frames' sets on the final tree — computed once, shared, never written."""
    ms = case_a_tree(shift)
    out = np.stack([visible_ref(f, ms, C.scene().voxel_size, px_step=px_step) for f in case_a_frames(shift)])
    out.setflags(write=False)
    return out


# ---- Case B -----------------------------------------------------------------
B_VOXEL = 0.2
B_ROW = 80
B_ORIGIN = (3.05, 6.1, 8.1)
B_DIR = (1.0, 0.0005, 0.0003)
B_COUNTS = {20.0: 46, 5.0: 21}
B_CAPPED = {20.0: 16, 5.0: 0}  # what the 50-leaf cap leaves of them


@functools.lru_cache(maxsize=None)
def case_b_tree():
    """(CPU map_states arrays, node id of row voxel i for i < 80)."""
    from psvo.octree import map_states
    keys = np.array([(20 + i, 30, 40) for i in range(B_ROW)], np.int32)
    tree = C.raw_tree(128, B_VOXEL, [keys])
    ms = map_states(tree, torch.zeros(1), B_VOXEL, device="cpu")
    ms = {n: ms[n] for n in C.MS_KEYS}
    centres, side = ms["voxel_center_xyz"].numpy(), ms["voxel_structure"].numpy()[:, 8]
    ids = []
    for i in range(B_ROW):
        want = (np.array([20 + i, 30, 40], np.float32) + 0.5) * np.float32(B_VOXEL)
        m = np.flatnonzero((side == 1) & (np.abs(centres - want).max(1) < 1e-4))
        assert m.size == 1
        ids.append(int(m[0]))
    return ms, tuple(ids)


def ray_frame(origin, direction, depth):
    """One ray as a 1 x 1 frame: dirs_cam = direction, identity rotation, t = origin."""
    pose = torch.eye(4, dtype=torch.float32)
    pose[:3, 3] = torch.tensor(origin, dtype=torch.float32)
    return (torch.full((1, 1), float(depth), dtype=torch.float32),
            torch.tensor(direction, dtype=torch.float32).reshape(1, 1, 3), pose)


# the same row seen from its far end: t_in = 16.75 - 0.2 i.  Depth 20: exactly i >= 34 (46 voxels), depth 5:
# i >= 59 (21).  A walk that visits children in ascending order meets THESE voxels last, so a leaf cap
# that the forward ray cannot see in such a walk shows here (and the other way round for 7→0 order).
B_ORIGIN_REV = (20.95, 6.1, 8.1)
B_DIR_REV = (-1.0, 0.0005, 0.0003)


def case_b_frame(depth, reverse=False):
    return ray_frame(B_ORIGIN_REV if reverse else B_ORIGIN, B_DIR_REV if reverse else B_DIR, depth)


def case_b_ref(depth, n_max=N_MAX, reverse=False):
    ms, _ = case_b_tree()
    o, d, z = frame_rays(*case_b_frame(depth, reverse), 1)
    return rays_visible_ref(o, d, z, ms["voxel_center_xyz"].numpy(), ms["voxel_structure"].numpy(), B_VOXEL,
                            TRUNCATION, MAX_DISTANCE, n_max=n_max)[0]


B_TIE_VOXEL = 10


@functools.lru_cache(maxsize=None)
def case_b_tie_depth():
    """A depth for Case B's ray whose bound depth + truncation (one fp32 add)
    IS row voxel 10's t_in, bit for bit: `<=` keeps 11 voxels, `<` only 10."""
    ms, ids = case_b_tree()
    o, d, _ = frame_rays(*case_b_frame(1.0), 1)
    idx, t0, _, _ = O.svo_intersect_flat(o, d, ms["voxel_center_xyz"].numpy(), ms["voxel_structure"].numpy(), B_VOXEL,
                                         n_max=N_MAX)
    t_in = np.float32(t0[0][idx[0] == ids[B_TIE_VOXEL]][0])
    depth = np.float32(t_in - np.float32(TRUNCATION))
    for _ in range(8):  # the subtraction's rounding may leave the sum one ulp off
        s = np.float32(depth + np.float32(TRUNCATION))
        if s == t_in:
            return float(depth)
        depth = np.nextafter(depth, np.float32(np.inf if s < t_in else -np.inf), dtype=np.float32)
    raise AssertionError("no fp32 depth puts the bound on the voxel's t_in")
