"""Mesh cleaning on the device (csrc/mesh_clean.hip) against the numpy
references of mesh_clean_case.py (pinned to the host code by
test_mesh_clean_cpu.py): back-projection within five fp32 roundings of the
fp64 formula, the downsample bit for bit, the ball mask equal to the brute
force, and create_mesh(clean_mseh=True) identical on the device and host
paths."""
import types

import numpy as np
import pytest
import torch

import mesh_clean_case as C

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the shared cases are read-only


def test_back_projection_bound_and_zero_depth():
    from psvo.mesh import depth_points_device
    pose, depth, dirs = C.general_frame(37, 53)
    out = depth_points_device(_dev(pose), _dev(depth), _dev(dirs))
    assert out.dtype == torch.float64 and tuple(out.shape) == (37 * 53, 3)
    got = out.cpu().numpy()
    ref, scale = C.backproject64(pose, depth, dirs)
    err = np.abs(got - ref)
    bound = 6 * 2.0 ** -24 * scale
    print("back-projection: max err / bound", float((err / bound).max()))
    assert (err <= bound).all()
    zero = depth.reshape(-1) == 0
    assert zero.sum() > 20
    np.testing.assert_array_equal(got[zero], np.broadcast_to(pose[:3, 3].astype(np.float64), (zero.sum(), 3)))
    # fp32 results widened: every value is an fp32 number
    np.testing.assert_array_equal(got, got.astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("name", list(C.downsample_cases()))
def test_downsample_bit_equal(name):
    from psvo.mesh import downsample_points_device
    p = C.downsample_cases()[name]
    ref = C.downsample_ref(p)
    out = downsample_points_device(_dev(p)).cpu().numpy()
    assert out.shape == ref.shape
    np.testing.assert_array_equal(out, ref)


def test_downsample_other_cell_size():
    from psvo.mesh import downsample_points_device
    p = C.downsample_cases()["clustered"]
    for cell in (0.05, 0.003):
        np.testing.assert_array_equal(downsample_points_device(_dev(p), cell).cpu().numpy(), C.downsample_ref(p, cell))


def test_depth_point_set_accumulates_bit_equal():
    """Three calls: old means + the frame's points re-binned, the origin moving."""
    from psvo.mesh import DepthPointSet, depth_points_device
    s = DepthPointSet(DEV)
    assert s.points is None and s.numpy() is None
    state = None
    for pose, depth, dirs in C.accumulate_frames():
        pts = depth_points_device(_dev(pose), _dev(depth), _dev(dirs)).cpu().numpy()
        state = C.downsample_ref(pts if state is None else np.concatenate([state, pts], 0))
        out = s.add_frame(_dev(pose), _dev(depth), _dev(dirs))
        assert out is s.points and out.is_cuda and out.dtype == torch.float64
        np.testing.assert_array_equal(s.numpy(), state)
    s.clear()
    assert s.points is None


def test_downsample_refuses_bad_input():
    from psvo import _lib as L
    from psvo.mesh import downsample_points_device
    p = np.array(C.downsample_cases()["negative"])
    for bad in (np.nan, np.inf, -np.inf):
        q = p.copy()
        q[17, 1] = bad
        with pytest.raises(L.PsvoError, match="not finite"):
            downsample_points_device(_dev(q))
    q = p.copy()
    q[5, 2] = q[:, 2].min() + 2.0 ** 21 * C.CELL * 1.0001  # past 2²¹ cells on one axis
    with pytest.raises(L.PsvoError, match="cells"):
        downsample_points_device(_dev(q))
    # the call after a refusal is unaffected
    np.testing.assert_array_equal(downsample_points_device(_dev(p)).cpu().numpy(), C.downsample_ref(p))


@pytest.mark.parametrize("name", list(C.ball_cases()))
def test_ball_equals_brute_force(name):
    from psvo.mesh import ball_any_device
    p, v = C.ball_cases()[name]
    hit, _ = C.ball_expected(name)
    out = ball_any_device(_dev(p), _dev(v), C.R)
    assert out.dtype == torch.bool and out.shape[0] == v.shape[0]
    np.testing.assert_array_equal(out.cpu().numpy(), hit)


def test_ball_non_finite_vertices_miss():
    from psvo.mesh import ball_any_device
    p, _ = C.ball_cases()["far"]
    v = np.float32([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf], p[0]])
    np.testing.assert_array_equal(ball_any_device(_dev(p), _dev(v), C.R).cpu().numpy(), [False, False, False, True])


def test_ball_empty_inputs():
    from psvo.mesh import ball_any_device
    p, v = C.ball_cases()["random"]
    none = ball_any_device(torch.zeros((0, 3), dtype=torch.float64, device=DEV), _dev(v), C.R)
    assert none.shape[0] == v.shape[0] and not none.any()
    empty = ball_any_device(_dev(p), torch.zeros((0, 3), dtype=torch.float32, device=DEV), C.R)
    assert empty.shape[0] == 0


# ---- end to end -------------------------------------------------------------
@pytest.fixture(scope="module")
def room():
    from psvo import synthetic as syn
    from psvo.decoder import Decoder
    from psvo.mesh import surface_states
    from psvo.octree import Octree
    scene = syn.room0()
    tree = Octree()
    tree.init(scene.grid_dim, 16, scene.voxel_size, 8)
    tree.insert(syn.surface_voxels(scene, seed=0))
    voxels, _, features = tree.export_arrays()
    gen = torch.Generator().manual_seed(0)
    emb = (torch.randn(voxels.shape[0], 16, generator=gen) * 0.3).to(DEV)
    torch.manual_seed(0)
    dec = Decoder(depth=2, width=128, in_dim=16, skips=[], embedder="none").to(DEV)
    sv, states = surface_states(torch.from_numpy(voxels), torch.from_numpy(features), emb, scene.voxel_size)
    return scene, dec, sv, states


def _extractor(scene, dirs):
    from psvo.mesh import MeshExtractor
    mx = MeshExtractor(types.SimpleNamespace(mapper_specs={"voxel_size": scene.voxel_size}))
    mx.rays_d = torch.from_numpy(dirs)
    return mx


def _same_mesh(a, b):
    np.testing.assert_array_equal(a.triangles, b.triangles)
    np.testing.assert_array_equal(a.vertices, b.vertices)
    np.testing.assert_array_equal(a.vertex_colors, b.vertex_colors)
    np.testing.assert_array_equal(a.vertex_normals, b.vertex_normals)


def test_create_mesh_clean_device_equals_host(room):
    scene, dec, sv, states = room
    # the third call's points all fall into cells the state already has: every mean is re-averaged
    frames = [C.exact_frame(0, 0), C.exact_frame(0, 3), C.exact_frame(0, 0)]
    mx_d, mx_h = _extractor(scene, frames[0][2]), _extractor(scene, frames[0][2])
    kw = dict(clean_mseh=True, require_color=True, offset=-10, res=8)
    full = mx_d.create_mesh(dec, states, scene.voxel_size, sv, require_color=True, offset=-10, res=8)
    assert mx_d.depth_points is None
    kept, sizes = [], []
    for pose, depth, _ in frames:
        md = mx_d.create_mesh(dec, states, scene.voxel_size, sv, torch.from_numpy(pose), torch.from_numpy(depth),
                              clean="device", **kw)
        mh = mx_h.create_mesh(dec, states, scene.voxel_size, sv, torch.from_numpy(pose), torch.from_numpy(depth),
                              clean="host", **kw)
        _same_mesh(md, mh)
        dp_d, dp_h = mx_d.depth_points, mx_h.depth_points
        assert dp_d.dtype == np.float64 and dp_d.shape == dp_h.shape
        np.testing.assert_array_equal(dp_d, dp_h)
        np.testing.assert_array_equal(md.vertices, full.vertices)
        kept.append(md.triangles.shape[0] / full.triangles.shape[0])
        sizes.append(dp_d.shape[0])
        assert 0 < kept[-1] < 1, kept
    n0 = 64 * 96
    assert sizes[0] <= n0 < sizes[1] <= 2 * n0 and sizes[2] < sizes[1] + n0 // 2, sizes  # accumulated, then merged
    # the default is the device path, and clean_mseh=False is what it was
    again = mx_d.create_mesh(dec, states, scene.voxel_size, sv, require_color=True, offset=-10, res=8)
    _same_mesh(again, full)


def test_create_mesh_clean_pose_list(room):
    """A list of 7 poses: frames 0 and 5, concatenated in order, one downsample, no state."""
    scene, dec, sv, states = room
    fr = [C.exact_frame(0, i) for i in range(5)] + [C.exact_frame(1, 0), C.exact_frame(1, 2)]
    poses = [torch.from_numpy(f[0]) for f in fr]
    depths = [torch.from_numpy(f[1]) for f in fr]
    kw = dict(clean_mseh=True, require_color=True, offset=-10, res=8)
    mx_d, mx_h = _extractor(scene, fr[0][2]), _extractor(scene, fr[0][2])
    md = mx_d.create_mesh(dec, states, scene.voxel_size, sv, poses, depths, **kw)
    mh = mx_h.create_mesh(dec, states, scene.voxel_size, sv, poses, depths, clean="host", **kw)
    _same_mesh(md, mh)
    assert mx_d.depth_points is None and mx_h.depth_points is None
    one = _extractor(scene, fr[0][2]).create_mesh(dec, states, scene.voxel_size, sv, poses[0], depths[0], **kw)
    assert md.triangles.shape[0] > one.triangles.shape[0] > 0  # frame 5 (the other wall) took part
