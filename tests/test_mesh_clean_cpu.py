"""The mesh-cleaning references (mesh_clean_case.py) against the host code they
restate: the stable-sort + sequential-sum downsample equals
MeshExtractor.downsample_points bit for bit on every input the GPU tests use,
and the brute-force ball mask equals scipy's cKDTree outside near-ties.  Also
that the cases discriminate, and that the library declares the new entry
points.  No GPU."""
import types

import numpy as np
import pytest

import mesh_clean_case as C
from psvo import _lib as L
from psvo.mesh import MeshExtractor

NEW_SYMBOLS = ["psvo_mesh_depth_points", "psvo_mesh_points_downsample", "psvo_mesh_ball_any"]


def _extractor():
    return MeshExtractor(types.SimpleNamespace(mapper_specs={"voxel_size": C.VOXEL}))


def test_new_entry_points_are_declared():
    for name in NEW_SYMBOLS:
        assert name in L.exported_symbols(), name
        assert hasattr(L.lib(), name), name


@pytest.mark.parametrize("name", list(C.downsample_cases()))
def test_downsample_ref_equals_host(name):
    p = C.downsample_cases()[name]
    ref = C.downsample_ref(p)
    host = _extractor().downsample_points(p)
    assert ref.shape == host.shape and ref.shape[0] >= 1
    np.testing.assert_array_equal(ref, host)


def test_downsample_ref_equals_host_clustered_sizes():
    """The clustered case has the cell sizes the kernels' paths switch on."""
    p = C.downsample_cases()["clustered"]
    key = np.floor((p - p.min(0)) / C.CELL).astype(np.int64)
    counts = np.unique(key, axis=0, return_counts=True)[1]
    assert (counts == 1).sum() > 100 and (counts > 64).sum() >= 6 and (counts > 1024).sum() == 1


def test_downsample_ref_equals_host_accumulating():
    """Three accumulating calls (old means + a frame's points, re-binned): the
    chain the DepthPointSet test runs, on fp32 back-projected frames."""
    state = None
    mx = _extractor()
    sizes = []
    for pose, depth, dirs in C.accumulate_frames():
        pts = C.backproject32(pose, depth, dirs).astype(np.float64)
        both = pts if state is None else np.concatenate([state, pts], 0)
        ref = C.downsample_ref(both)
        np.testing.assert_array_equal(ref, mx.downsample_points(both))
        state = ref
        sizes.append(ref.shape[0])
    assert sizes[0] < sizes[1] < sizes[2] < 3 * 37 * 53  # new cells every call, and merging


@pytest.mark.parametrize("name", list(C.ball_cases()))
def test_ball_ref_equals_kdtree_and_discriminates(name):
    from scipy.spatial import cKDTree
    p, v = C.ball_cases()[name]
    hit, near = C.ball_expected(name)
    tree = cKDTree(p).query_ball_point(v, C.R, return_length=True) > 0
    np.testing.assert_array_equal(hit[~near], tree[~near])
    share = hit.mean()
    assert 0.2 <= share <= 0.8, share


def test_ball_near_ties_are_rare():
    """Near-ties (| |d| − r | ≤ 1e-9·r) over all the cases' vertices: at most
    0.1 % — the ones the exact-radius case builds on purpose."""
    total = sum(C.ball_expected(n)[1].shape[0] for n in C.ball_cases())
    ties = sum(int(C.ball_expected(n)[1].sum()) for n in C.ball_cases())
    assert ties >= 2  # the exact-radius vertices
    assert ties <= 1e-3 * total, (ties, total)


def test_backproject32_within_bound_of_fp64():
    pose, depth, dirs = C.general_frame()
    ref, scale = C.backproject64(pose, depth, dirs)
    got = C.backproject32(pose, depth, dirs).astype(np.float64)
    assert (np.abs(got - ref) <= 6 * 2.0 ** -24 * scale).all()
    assert (depth == 0).sum() > 20


def test_exact_frames_backproject_exactly():
    """The end-to-end frames: fp32 back-projection equals the fp64 one (no
    rounding anywhere), so host and device see the same points."""
    for which, shift in ((0, 0), (0, 3), (1, 0)):
        pose, depth, dirs = C.exact_frame(which, shift)
        ref, _ = C.backproject64(pose, depth, dirs)
        np.testing.assert_array_equal(C.backproject32(pose, depth, dirs).astype(np.float64), ref)
