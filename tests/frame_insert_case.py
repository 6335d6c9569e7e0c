"""Shared inputs and the reference of the depth-frame insertion tests
(test_frame_insert_cpu.py, test_gpu_frame_insert.py).

The reference restates Mapping.create_voxels_pointcloud's key arithmetic
(frame.py:69-71, mapping.py:263-264, 292) in torch-CPU elementwise ops, with
the matmul written out as the left-to-right sum include/psvo.h pins, and feeds
every valid pixel's key to the CPU Octree.  Frames: synthetic room0 seen from
camera_poses(scene, 4, seed=0) at scale 0.25 (170 x 300 pixels, all valid,
walls exactly on voxel boundaries — where floor(a / b) and torch's floor
division part ways for most pixels).
"""
import functools

import numpy as np
import torch

from psvo import synthetic as syn
from psvo.octree import Octree, map_states

MS_KEYS = ("voxel_center_xyz", "voxel_structure", "voxel_vertex_idx")

# distinct voxels per frame / of those new to the tree, unshifted pose
# (counted on the CPU with numpy and the oracle's octree)
DISTINCT = (666, 1559, 565, 374)
NEW = (666, 1559, 74, 295)
SHIFT = -12.0  # metres: puts coordinates below zero


def restated_keys(depth, rays_d, pose, voxel_size):
    """(keys i32[n,3], valid bool[n], skipped) of a frame; keys rows of
    pixels that are not valid are 0."""
    depth = torch.as_tensor(depth, dtype=torch.float32).cpu()
    rays_d = torch.as_tensor(rays_d, dtype=torch.float32).cpu()
    pose = torch.as_tensor(pose, dtype=torch.float32).cpu()
    vmap = (rays_d * depth[..., None]).reshape(-1, 3)            # frame.py:69
    has = (depth > 0).reshape(-1)                                # frame.py:71
    R, t = pose[:3, :3], pose[:3, 3]
    cols = []
    for k in range(3):                                           # points @ R^T + t, summed left to right
        s = vmap[:, 0] * R[k, 0]
        s = s + vmap[:, 1] * R[k, 1]
        s = s + vmap[:, 2] * R[k, 2]
        cols.append(s + t[k])
    points = torch.stack(cols, -1)
    voxels = torch.div(points, voxel_size, rounding_mode="floor")  # mapping.py:264
    ok = torch.isfinite(points).all(-1) & (voxels >= -2147483648.0).all(-1) & (voxels < 2147483648.0).all(-1)
    valid = has & ok
    keys = torch.zeros(voxels.shape, dtype=torch.int32)
    keys[valid] = voxels[valid].int()                            # mapping.py:292
    return keys, valid, int((has & ~ok).sum())


@functools.lru_cache(maxsize=None)
def scene():
    return syn.room0()


@functools.lru_cache(maxsize=None)
def frames():
    """[(depth [H,W], rays_d [H,W,3], pose 4x4 f32)] on the CPU."""
    sc = scene()
    out = []
    for T in syn.camera_poses(sc, 4, seed=0):
        f = syn.SyntheticFrame(sc, T, scale=0.25, device="cpu")
        out.append((f.depth, f.rays_d, torch.from_numpy(np.asarray(T, np.float32))))
    return out


def shifted(pose, metres=SHIFT):
    p = pose.clone()
    p[:3, 3] += metres
    return p


@functools.lru_cache(maxsize=None)
def reference(shift):
    """Per frame: (keys of the valid pixels i32[m,3] in pixel order, CPU
    builder's (voxels, children, features) after raw insertion of every key up
    to and including this frame, node count, its map_states)."""
    sc = scene()
    tree = Octree()
    tree.init(sc.grid_dim, 16, sc.voxel_size, 8)
    out = []
    for depth, rays_d, pose in frames():
        keys, valid, _ = restated_keys(depth, rays_d, shifted(pose, shift) if shift else pose, sc.voxel_size)
        k = keys[valid].numpy()
        tree.insert(k)
        ms = map_states(tree, torch.zeros(1), sc.voxel_size, device="cpu")
        out.append((k, tree.export_arrays(), tree.count_nodes(), {n: ms[n] for n in MS_KEYS}))
    return out


def raw_tree(grid_dim, voxel_size, key_batches):
    """CPU Octree after raw insertion of each batch of keys."""
    tree = Octree()
    tree.init(grid_dim, 16, voxel_size, 8)
    for k in key_batches:
        if len(k):
            tree.insert(np.ascontiguousarray(k, dtype=np.int32))
    return tree
