"""The whole-frame renderer's interface without a GPU: the header declares
it, the built library exports it, the tile workspace size is a function of
the tile alone, and FrameRenderer's argument checks raise ValueError before
any device access."""
import inspect
import os
import re

import pytest
import torch

from psvo import _lib as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(REPO, "include", "psvo.h")).read()


def test_header_declares_the_renderer():
    src = _header()
    assert re.search(r"\bint\s+psvo_render_frame\s*\(\s*psvo_engine\s*\*", src)
    m = re.search(r"\bint64_t\s+psvo_render_tile_bytes\s*\(([^)]*)\)", src)
    assert m and "n_rays" not in m.group(1) and m.group(1).count(",") == 2, m and m.group(1)
    assert re.search(r"typedef\s+struct\s+psvo_render_opts\s*\{[^}]*int64_t\s+tile_rays;[^}]*int\s+flags;[^}]*\}\s*"
                     r"psvo_render_opts\s*;", src)
    assert "PSVO_RENDER_STAT_WORDS" in src


def test_library_exports_the_renderer():
    lib = L.lib()
    for name in ("psvo_render_frame", "psvo_render_tile_bytes"):
        assert hasattr(lib, name), name
        assert name in L.exported_symbols()


def test_tile_bytes_is_a_function_of_the_tile():
    from psvo.render import tile_bytes
    assert list(inspect.signature(tile_bytes).parameters) == ["tile_rays", "max_steps", "width"]
    assert len(L._SIGNATURES["psvo_render_tile_bytes"][1]) == 3  # tile_rays, max_steps, width: no n_rays
    for width in (128, 256):
        base = tile_bytes(256, 100, width)
        assert base > 0
        assert tile_bytes(257, 100, width) > base and tile_bytes(16384, 100, width) > tile_bytes(4096, 100, width)
        assert tile_bytes(256, 101, width) > base and tile_bytes(256, 300, width) > tile_bytes(256, 200, width)
        # everything sized by samples: at least the sampler's rows and the per-sample sdf
        assert base >= 256 * 100 * 12
    assert tile_bytes(256, 100, 256) > tile_bytes(256, 100, 128)  # the width-256 tile keeps a feature buffer
    for bad in ((0, 100, 128), (256, 0, 128), (256, 100, 64)):
        assert tile_bytes(*bad) == -1


class _Dec:
    """The decoder's interface as FrameRenderer reads it (no device)."""

    def __init__(self, width=128, dtype=torch.float32):
        self.W = width
        shapes = [(width, 16), (width,), (width, width), (width,), (129, width), (129,), (width, 144), (width,),
                  (3, width), (3,)]
        self._p = [torch.zeros(s, dtype=dtype) for s in shapes]

    def fused_params(self):
        return self._p


def _cpu_map(n=4, e=10):
    return {"voxel_vertex_emb": torch.zeros(e, 16), "voxel_center_xyz": torch.zeros(n, 3),
            "voxel_structure": torch.zeros(n, 9, dtype=torch.int32),
            "voxel_vertex_idx": torch.zeros(n, 8, dtype=torch.int32)}


def test_constructor_checks_raise_before_device_access():
    from psvo.render import FrameRenderer
    ms = _cpu_map()
    for tile in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="tile_rays"):
            FrameRenderer(ms, _Dec(), 0.2, 0.01, tile_rays=tile)
    with pytest.raises(ValueError, match="step_size"):
        FrameRenderer(ms, _Dec(), 0.2, 0.0)
    with pytest.raises(ValueError, match="width"):
        FrameRenderer(ms, _Dec(64), 0.2, 0.01)
    bad = dict(ms, voxel_vertex_emb=torch.zeros(10, 8))
    with pytest.raises(ValueError, match="embeddings"):
        FrameRenderer(bad, _Dec(), 0.2, 0.01)
    bad = dict(ms, voxel_structure=torch.zeros(4, 8, dtype=torch.int32))
    with pytest.raises(ValueError, match="voxel_structure"):
        FrameRenderer(bad, _Dec(), 0.2, 0.01)
    with pytest.raises(ValueError, match="float32"):
        FrameRenderer(ms, _Dec(dtype=torch.float64), 0.2, 0.01)
    with pytest.raises(ValueError, match="CUDA device"):  # a map on the CPU: refused, not copied
        FrameRenderer(ms, _Dec(), 0.2, 0.01)


def test_ray_noise_and_camera_checks():
    from psvo import render as R
    ro, rd = torch.zeros(5, 3), torch.zeros(5, 3)
    assert R.check_rays(ro, rd) == 5 and R.check_rays(ro[None], rd[None]) == 5
    with pytest.raises(ValueError, match="float32"):
        R.check_rays(ro.double(), rd)
    with pytest.raises(ValueError, match=r"\[R,3\]"):
        R.check_rays(torch.zeros(5, 4), rd)
    with pytest.raises(ValueError, match=r"\[R,3\]"):
        R.check_rays(torch.zeros(2, 5, 3), rd)
    with pytest.raises(ValueError, match="origins"):
        R.check_rays(torch.zeros(4, 3), rd)
    with pytest.raises(ValueError, match="is on"):
        R.check_rays(ro, rd, torch.device("meta"))
    R.check_noise(torch.zeros(200, 7, 216), 1280, 216)
    for bad in (torch.zeros(200, 7), torch.zeros(100, 7, 216), torch.zeros(200, 7, 216, dtype=torch.int32)):
        with pytest.raises(ValueError, match="noise"):
            R.check_noise(bad)
    for r_hit, steps in ((1280, 215), (1401, 216), (1200, 216)):  # K' = ceil(R_hit / 200)
        with pytest.raises(ValueError, match="noise"):
            R.check_noise(torch.zeros(200, 7, 216), r_hit, steps)
    K, T = torch.eye(3), torch.eye(4)
    R.check_camera(T, K, 40, 32, (1200, 680))
    with pytest.raises(ValueError, match="pose_c2w"):
        R.check_camera(torch.eye(3), K, 40, 32)
    with pytest.raises(ValueError, match="K must"):
        R.check_camera(T, torch.eye(4), 40, 32)
    with pytest.raises(ValueError, match="w must"):
        R.check_camera(T, K, 0, 32)
    with pytest.raises(ValueError, match="src_wh"):
        R.check_camera(T, K, 40, 32, (0, 680))


def test_camera_dirs_are_frame_get_rays():
    """frame.get_rays (frame.py:43-58) at a scaled resolution, in fp32."""
    from psvo.render import camera_dirs
    K = [[600.0, 0.0, 599.5], [0.0, 600.0, 339.5], [0.0, 0.0, 1.0]]
    d = camera_dirs(K, 40, 32, (1200, 680))
    assert d.shape == (32, 40, 3) and d.dtype == torch.float32
    fx, fy, cx, cy = 600.0 * 40 / 1200, 600.0 * 32 / 680, 599.5 * 40 / 1200, 339.5 * 32 / 680
    ix, iy = torch.meshgrid(torch.arange(40), torch.arange(32), indexing="xy")
    ref = torch.stack([(ix - cx) / fx, (iy - cy) / fy, torch.ones_like(ix)], -1).float()
    assert torch.equal(d, ref)
    assert float(d[5, 7, 0]) == pytest.approx((7 - cx) / fx, rel=1e-6) and float(d[5, 7, 2]) == 1.0
