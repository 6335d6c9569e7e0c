"""Depth-frame insertion, the parts that need no GPU: the C ABI's new names,
the host-only workspace size, argument checks that must come before any
device call, and Octree.insert_frame (the CPU builder's dedup-then-insert)
against raw insertion of every pixel's key."""
import ctypes
import re

import numpy as np
import pytest

import frame_insert_case as C
from psvo import _lib as L
from psvo.octree import Octree

NEW_NAMES = ("psvo_depth_voxel_keys", "psvo_dtree_frame_workspace_bytes", "psvo_dtree_insert_depth",
             "psvo_dtree_generation")


def _invalid_code():
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psvo.h")).read()
    m = re.search(r"PSVO_E_INVALID\s*=\s*(-?\d+)", src)
    assert m, "PSVO_E_INVALID not found in include/psvo.h"
    return int(m.group(1))


def test_new_names_exported_and_declared():
    lib = L.lib()
    for name in NEW_NAMES:
        assert hasattr(lib, name), name
        assert name in L._SIGNATURES, name
        assert getattr(lib, name).argtypes == L._SIGNATURES[name][1]


def test_frame_workspace_bytes():
    f = L.lib().psvo_dtree_frame_workspace_bytes
    for h, w in ((0, 10), (10, 0), (-1, 5), (5, -1), (0, 0)):
        assert f(h, w) == -1, (h, w)
    assert f(4096, 4096) > 0 and f(4097, 4096) == -1  # 2^24 pixels is the limit
    sizes = [f(h, w) for h, w in ((1, 1), (5, 7), (64, 64), (170, 300), (340, 600), (680, 1200), (2048, 2048))]
    assert all(s > 0 for s in sizes)
    assert all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    assert sizes[0] < sizes[-1]
    # raw insertion's scratch: two ints per (walk, depth) = 2 · 8 corners · 8 depths · 4 B per pixel
    assert f(680, 1200) < 2 * 8 * 8 * 4 * 680 * 1200


def test_insert_depth_rejects_null_tree_before_any_device_call():
    lib = L.lib()
    stats = (ctypes.c_int64 * 8)()
    one = ctypes.c_void_p(16)  # never dereferenced: the arguments are refused first
    rc = lib.psvo_dtree_insert_depth(None, None, 4, 4, one, one, one, 0.2, stats)
    assert rc == _invalid_code()
    assert b"insert_depth" in lib.psvo_last_error()
    assert lib.psvo_dtree_generation(None) == 0


@pytest.mark.parametrize("shift", [0.0, C.SHIFT])
def test_cpu_insert_frame_equals_raw_insertion(shift):
    sc = C.scene()
    tree = Octree()
    tree.init(sc.grid_dim, 16, sc.voxel_size, 8)
    seen = set()
    for i, ((depth, rays_d, pose), (keys, arrays, count, _)) in enumerate(zip(C.frames(), C.reference(shift))):
        st = tree.insert_frame(depth, rays_d, C.shifted(pose, shift) if shift else pose)
        assert tree.count_nodes() == count
        for a, b in zip(arrays, tree.export_arrays()):
            np.testing.assert_array_equal(a, b)
        uniq = {tuple(r) for r in keys.tolist()}
        assert st["valid"] == keys.shape[0] == depth.numel() and st["skipped"] == 0
        assert st["distinct"] == len(uniq)
        assert st["new"] == len(uniq - seen)
        seen |= uniq
        if not shift:
            assert (st["distinct"], st["new"]) == (C.DISTINCT[i], C.NEW[i])
    if shift:
        assert min(k.min() for k, _, _, _ in C.reference(shift)) < 0  # the shifted pose does reach negative coordinates
