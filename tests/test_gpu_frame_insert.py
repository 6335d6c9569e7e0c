"""DeviceOctree.insert_frame / psvo_dtree_insert_depth / psvo_depth_voxel_keys
(csrc/octree_gpu.hip) against the torch-CPU restatement of the
reference's key arithmetic and raw insertion of every valid pixel's key
(frame_insert_case.py).  Every comparison is exact."""
import math

import numpy as np
import pytest
import torch

import frame_insert_case as C
from psvo import _lib as L
from psvo.octree import DeviceOctree, map_states

pytestmark = pytest.mark.gpu
DEV = "cuda"


def device_keys(depth, rays_d, pose, voxel_size):
    d = depth.to(DEV).contiguous().reshape(-1)
    r = rays_d.to(DEV).contiguous()
    p = pose[:3].to(DEV).contiguous()
    n = d.numel()
    keys = torch.full((n, 3), -7, dtype=torch.int32, device=DEV)
    valid = torch.full((n,), 9, dtype=torch.uint8, device=DEV)
    L.call("psvo_depth_voxel_keys", L.stream_of(DEV), n, d, r, p, float(voxel_size), keys, valid)
    return keys.cpu(), valid.cpu()


def new_tree(grid_dim, voxel_size, capacity=1 << 16):
    t = DeviceOctree(DEV)
    t.init(grid_dim, 16, voxel_size, 8, capacity=capacity)
    return t


def assert_tree_equals(dev, cpu):
    assert dev.count_nodes() == cpu.count_nodes()
    for a, b in zip(cpu.export_arrays(), dev.export_arrays()):
        np.testing.assert_array_equal(a, b.cpu().numpy())


def pinhole(h, w, f):
    """Camera directions [h, w, 3] of a pinhole of focal length f pixels."""
    iy, ix = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    return torch.stack([(ix - (w - 1) / 2) / f, (iy - (h - 1) / 2) / f, torch.ones_like(ix)], -1)


def pose_at(x, y, z):
    p = torch.eye(4)
    p[:3, 3] = torch.tensor([x, y, z])
    return p


def check_frame(depth, rays_d, pose, voxel_size, grid_dim, distinct=None):
    """insert_frame on a fresh tree == raw CPU insertion of the restated keys;
    the statistics equal the counts."""
    keys, valid, skipped = C.restated_keys(depth, rays_d, pose, voxel_size)
    k = keys[valid].numpy()
    uniq = {tuple(r) for r in k.tolist()}
    if distinct is not None:
        assert len(uniq) == distinct
    dev = new_tree(grid_dim, voxel_size)
    st = dev.insert_frame(depth, rays_d, pose)
    cpu = C.raw_tree(grid_dim, voxel_size, [k])
    assert_tree_equals(dev, cpu)
    assert (st["valid"], st["skipped"], st["distinct"], st["new"]) == (k.shape[0], skipped, len(uniq), len(uniq))
    assert st["created"] == cpu.count_nodes() - 1
    assert st["workspace_bytes"] == L.lib().psvo_dtree_frame_workspace_bytes(depth.shape[0], depth.shape[1])
    dk, dv = device_keys(depth, rays_d, pose, voxel_size)
    assert torch.equal(dv.bool(), valid) and torch.equal(dk, keys)
    return st


@pytest.mark.parametrize("shift", [0.0, C.SHIFT])
def test_keys_equal_restatement(shift):
    vs = C.scene().voxel_size
    for (depth, rays_d, pose), ref in zip(C.frames(), C.reference(shift)):
        pose = C.shifted(pose, shift) if shift else pose
        keys, valid = device_keys(depth, rays_d, pose, vs)
        assert valid.all() and valid.max() == 1
        np.testing.assert_array_equal(keys.numpy(), ref[0])
    if shift:
        assert min(ref[0].min() for ref in C.reference(shift)) < 0


@pytest.mark.parametrize("shift", [0.0, C.SHIFT])
def test_tree_equals_raw_insertion_frame_by_frame(shift):
    sc = C.scene()
    a, b = new_tree(sc.grid_dim, sc.voxel_size), new_tree(sc.grid_dim, sc.voxel_size)
    emb = torch.zeros(1, device=DEV)
    seen = set()
    for i, ((depth, rays_d, pose), (keys, arrays, count, ms_cpu)) in enumerate(zip(C.frames(), C.reference(shift))):
        st = a.insert_frame(depth.to(DEV), rays_d.to(DEV), (C.shifted(pose, shift) if shift else pose).to(DEV))
        b.insert(torch.from_numpy(keys))
        assert a.count_nodes() == b.count_nodes() == count
        for ref, xa, xb in zip(arrays, a.export_arrays(), b.export_arrays()):
            np.testing.assert_array_equal(ref, xa.cpu().numpy())
            np.testing.assert_array_equal(ref, xb.cpu().numpy())
        ms_a, ms_b = map_states(a, emb, sc.voxel_size), map_states(b, emb, sc.voxel_size)
        for k in C.MS_KEYS:
            assert torch.equal(ms_cpu[k], ms_a[k].cpu()), k
            assert torch.equal(ms_cpu[k], ms_b[k].cpu()), k
        uniq = {tuple(r) for r in keys.tolist()}
        assert (st["valid"], st["skipped"]) == (keys.shape[0], 0)
        assert (st["distinct"], st["new"]) == (len(uniq), len(uniq - seen))
        seen |= uniq
        if not shift:
            assert (st["distinct"], st["new"]) == (C.DISTINCT[i], C.NEW[i])
    assert a.count_leaf_nodes() == b.count_leaf_nodes() == len(seen)


def test_second_integration_of_a_frame_is_a_no_op():
    sc = C.scene()
    depth, rays_d, pose = C.frames()[0]
    t = new_tree(sc.grid_dim, sc.voxel_size)
    emb = torch.zeros(1, device=DEV)
    g0 = t.generation
    ms0 = map_states(t, emb, sc.voxel_size)
    st1 = t.insert_frame(depth, rays_d, pose)
    assert st1["new"] == C.NEW[0] and st1["created"] == t.count_nodes() - 1
    g1 = t.generation
    assert g1 > g0
    ms1 = map_states(t, emb, sc.voxel_size)
    assert ms1["voxel_center_xyz"] is not ms0["voxel_center_xyz"]
    assert ms1["voxel_center_xyz"].shape[0] == t.count_nodes()
    st2 = t.insert_frame(depth, rays_d, pose)
    assert (st2["valid"], st2["distinct"], st2["new"], st2["created"]) == (st1["valid"], st1["distinct"], 0, 0)
    assert t.generation == g1
    ms2 = map_states(t, emb, sc.voxel_size)
    for k in C.MS_KEYS:
        assert ms2[k] is ms1[k], k
    np.testing.assert_array_equal(ms2["voxel_structure"].cpu().numpy(), C.reference(0.0)[0][3]["voxel_structure"].numpy())


def test_raw_insert_advances_the_generation_only_when_the_tree_changes():
    t = new_tree(64, 0.2)
    vox = torch.tensor([[3, 4, 5], [3, 4, 5], [10, 2, 7]], dtype=torch.int32)
    g0 = t.generation
    t.insert(vox)
    g1 = t.generation
    assert g1 > g0
    t.insert(vox[:2])  # already SURFACE: nothing created, nothing promoted
    assert t.generation == g1
    n = t.count_nodes()
    t.insert(torch.tensor([[4, 5, 6]], dtype=torch.int32))  # a FEATURE corner of (3, 4, 5): promoted
    assert t.generation > g1 and t.count_nodes() > n


# a frustum narrower than a voxel (long runs of one key, across wave boundaries
# and row ends) and one several voxels wide (runs that end inside a row)
@pytest.mark.parametrize("focal_per_width", [40.0, 2.0])
@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (1, 64), (3, 65)])
def test_small_frames(h, w, focal_per_width):
    g = torch.Generator().manual_seed(h * 100 + w)
    depth = 2.0 + 0.05 * torch.rand((h, w), generator=g)
    st = check_frame(depth, pinhole(h, w, focal_per_width * w), pose_at(10.03, 10.07, 10.0), 0.2, 256)
    if focal_per_width == 40.0:
        assert st["distinct"] <= 4 < st["valid"] or h * w == 1


def test_one_voxel_frame():
    depth = torch.full((64, 64), 2.0)
    st = check_frame(depth, pinhole(64, 64, 4.0 * 64), pose_at(10.5, 10.5, 10.0), 1.0, 256, distinct=1)
    assert (st["valid"], st["new"]) == (4096, 1)


def test_alternating_planes_keep_first_occurrence_order():
    h, w = 4, 30
    depth = torch.where((torch.arange(h * w) // 3) % 2 == 0, 2.5, 3.5).reshape(h, w)  # A A A B B B A A A ...
    check_frame(depth, pinhole(h, w, 40.0 * w), pose_at(10.5, 10.5, 10.0), 1.0, 256, distinct=2)


def test_every_pixel_its_own_voxel():
    depth = torch.full((64, 64), 2.0)
    st = check_frame(depth, pinhole(64, 64, 64.0), pose_at(10.003, 10.003, 10.003), 0.01, 4096, distinct=4096)
    assert st["new"] == 4096


def test_holes_and_unrepresentable_pixels():
    h = w = 16
    g = torch.Generator().manual_seed(3)
    depth = 1.5 + torch.rand((h, w), generator=g)
    flat = depth.reshape(-1)
    perm = torch.randperm(h * w, generator=g)
    flat[perm[0:20]] = 0.0
    flat[perm[20:40]] = -1.0
    flat[perm[40:60]] = math.nan
    flat[perm[60:80]] = math.inf
    flat[perm[80:90]] = 1e12   # finite world point, quotient outside int32
    flat[perm[90:100]] = 3e38  # finite world point, the quotient overflows
    rays_d, pose = pinhole(h, w, 1.5 * w), pose_at(10.0, 10.0, 10.0)
    st = check_frame(depth, rays_d, pose, 0.2, 256)
    assert (st["valid"], st["skipped"]) == (h * w - 100, 40)

    t = new_tree(256, 0.2)
    t.insert_frame(depth, rays_d, pose)
    g1, n1 = t.generation, t.count_nodes()
    st0 = t.insert_frame(torch.zeros(h, w), rays_d, pose)
    assert {k: v for k, v in st0.items() if k != "workspace_bytes"} == dict(valid=0, skipped=0, distinct=0, new=0, created=0)
    assert (t.generation, t.count_nodes()) == (g1, n1)
    fresh = new_tree(256, 0.2)
    fresh.insert_frame(torch.zeros(h, w), rays_d, pose)
    assert fresh.count_nodes() == 1 and fresh.generation == 0


def test_growth_and_rehash_inside_insert_frame():
    sc = C.scene()
    t = new_tree(sc.grid_dim, sc.voxel_size, capacity=1024)
    for (depth, rays_d, pose), (_, arrays, count, _) in list(zip(C.frames(), C.reference(0.0)))[:2]:
        t.insert_frame(depth, rays_d, pose)
        assert t.count_nodes() == count > 1024
        for a, b in zip(arrays, t.export_arrays()):
            np.testing.assert_array_equal(a, b.cpu().numpy())


def test_coordinates_beyond_the_grid_are_neither_clamped_nor_dropped():
    sc = C.scene()
    depth, rays_d, pose = C.frames()[0]
    keys = C.reference(0.0)[0][0]
    assert keys.max() >= 64 > keys.min()  # part of the frame lies outside a 64-grid
    t = new_tree(64, sc.voxel_size)
    st = t.insert_frame(depth, rays_d, pose)
    assert st["valid"] == keys.shape[0] and st["skipped"] == 0
    assert_tree_equals(t, C.raw_tree(64, sc.voxel_size, [keys]))
