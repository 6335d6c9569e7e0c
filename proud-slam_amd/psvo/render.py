"""Whole-frame renderer (csrc/render.hip, psvo_render_frame): colour, depth and
hit mask of the map from a pose, as images — what Tracking.render_debug_images
(tracking.py:162-215) does every 50 frames and what a map evaluation at full
resolution needs — through a tiled, inference-only pipeline: the sdf trunk on
every sample with the interpolation fused into its operand load, the colour
head only on the composited samples, results scattered into original ray order
(fill_in(…, 0) fused).

The result is render_helpers.render_rays on the whole ray batch with the same
sampler noise, independent of the tile size (include/psvo.h); unlike
render_rays a view that sees nothing of the map is not an error (all zeros).
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib as L
from .engine import MapDesc

_vp, _i32, _i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64

STAT_NAMES = ("r_hit", "P", "max_steps", "S_max", "M", "M_composited", "n_tiles", "ray_bytes", "tile_bytes")
QUERY_ONLY = 1
DEFAULT_TILE_RAYS = 16384


class RenderOpts(ctypes.Structure):
    """Mirror of psvo_render_opts (include/psvo.h)."""
    _fields_ = [("tile_rays", _i64), ("flags", _i32)]


def tile_bytes(tile_rays, max_steps, width=128):
    """psvo_render_tile_bytes: the tile workspace (host arithmetic, no GPU)."""
    return int(L.lib().psvo_render_tile_bytes(int(tile_rays), int(max_steps), int(width)))


# ---- argument checks (no device access: they look at metadata only) --------
def check_tile_rays(tile_rays):
    if isinstance(tile_rays, bool) or not isinstance(tile_rays, int) or tile_rays < 1:
        raise ValueError(f"FrameRenderer: tile_rays must be an integer >= 1, got {tile_rays!r}")


def check_map(map_states, params):
    for k in ("voxel_vertex_emb", "voxel_center_xyz", "voxel_structure", "voxel_vertex_idx"):
        if k not in map_states or not isinstance(map_states[k], torch.Tensor):
            raise ValueError(f"FrameRenderer: map_states[{k!r}] must be a tensor")
    emb = map_states["voxel_vertex_emb"]
    if emb.dim() != 2 or emb.shape[1] != 16:
        raise ValueError(f"FrameRenderer: embeddings must be [E, 16], got {tuple(emb.shape)}")
    n = map_states["voxel_center_xyz"].shape[0]
    for k, cols in (("voxel_center_xyz", 3), ("voxel_structure", 9), ("voxel_vertex_idx", 8)):
        t = map_states[k]
        if t.dim() != 2 or t.shape != (n, cols):
            raise ValueError(f"FrameRenderer: map_states[{k!r}] must be [{n}, {cols}], got {tuple(t.shape)}")
    for t in [emb] + list(params):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("FrameRenderer: embeddings / decoder parameters must be contiguous float32")
    for t in [emb] + list(params) + [map_states[k] for k in ("voxel_center_xyz", "voxel_structure",
                                                             "voxel_vertex_idx")]:
        if not t.is_cuda or t.device != emb.device:
            raise ValueError("FrameRenderer: the map and the decoder must live on one CUDA device")


def check_rays(rays_o, rays_d, device=None):
    """-> the ray count R of rays_o / rays_d ([R,3] or [1,R,3])."""
    for name, t in (("rays_o", rays_o), ("rays_d", rays_d)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"render_rays: {name} must be a tensor")
        if t.dtype != torch.float32:
            raise ValueError(f"render_rays: {name} must be float32, got {t.dtype}")
        if not (t.dim() in (2, 3) and t.shape[-1] == 3 and (t.dim() == 2 or t.shape[0] == 1)):
            raise ValueError(f"render_rays: {name} must be [R,3] or [1,R,3], got {tuple(t.shape)}")
        if device is not None and t.device != device:
            raise ValueError(f"render_rays: {name} is on {t.device}, the map on {device}")
    if rays_o.shape[-2] != rays_d.shape[-2]:
        raise ValueError(f"render_rays: {rays_o.shape[-2]} origins for {rays_d.shape[-2]} directions")
    return int(rays_d.shape[-2])


def check_noise(noise, r_hit=None, max_steps=None):
    """The sampler noise is [200, K' = ceil(R_hit/200), max_steps] (the frame's
    layout); r_hit / max_steps None: only what holds for any frame."""
    if not isinstance(noise, torch.Tensor) or noise.dim() != 3 or noise.shape[0] != 200:
        raise ValueError(f"render_rays: noise must be a [200, K', max_steps] tensor, got "
                         f"{tuple(noise.shape) if isinstance(noise, torch.Tensor) else type(noise)}")
    if not noise.dtype.is_floating_point:
        raise ValueError(f"render_rays: noise must be floating point, got {noise.dtype}")
    if r_hit is not None:
        want = (200, -(-int(r_hit) // 200), int(max_steps))
        if tuple(noise.shape) != want:
            raise ValueError(f"render_rays: noise must be {want} for this frame ({r_hit} hit rays), got "
                             f"{tuple(noise.shape)}")


def check_camera(pose_c2w, K, w, h, src_wh=None):
    for name, t, shape in (("pose_c2w", pose_c2w, (4, 4)), ("K", K, (3, 3))):
        if tuple(getattr(t, "shape", ())) != shape:
            raise ValueError(f"render: {name} must be {list(shape)}, got {tuple(getattr(t, 'shape', ()))}")
    for name, v in (("w", w), ("h", h)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f"render: {name} must be an integer >= 1, got {v!r}")
    if src_wh is not None and not (len(src_wh) == 2 and src_wh[0] > 0 and src_wh[1] > 0):
        raise ValueError(f"render: src_wh must be (src_w, src_h) > 0, got {src_wh!r}")


def camera_dirs(K, w, h, src_wh=None, device="cpu"):
    """frame.get_rays (frame.py:43-58): fp32 ((ix − cx)/fx, (iy − cy)/fy, 1)
    [h,w,3], the intrinsics scaled by w/src_w, h/src_h."""
    k = [[float(K[i][j]) for j in range(3)] for i in range(3)]
    sw, sh = (w, h) if src_wh is None else src_wh
    fx, fy = k[0][0] * w / sw, k[1][1] * h / sh
    cx, cy = k[0][2] * w / sw, k[1][2] * h / sh
    ix, iy = torch.meshgrid(torch.arange(w, device=device), torch.arange(h, device=device), indexing="xy")
    return torch.stack([(ix - cx) / fx, (iy - cy) / fy, torch.ones_like(ix)], -1).float().contiguous()


class FrameRenderer:
    """map_states: psvo.octree.map_states dict (device); decoder:
    psvo.decoder.Decoder (width 128 or 256).  The map and the decoder are
    read, never written.  Owns its engine handle (as TrackingEngine does), so a
    MappingEngine's queued look-ahead is never disturbed; refresh(map_states)
    after the map has grown; close() frees the device buffers."""

    def __init__(self, map_states, decoder, voxel_size, step_size, truncation=0.1, max_distance=10.0,
                 tile_rays=DEFAULT_TILE_RAYS):
        check_tile_rays(tile_rays)
        for name, v in (("voxel_size", voxel_size), ("step_size", step_size), ("truncation", truncation),
                        ("max_distance", max_distance)):
            if not float(v) > 0.0:
                raise ValueError(f"FrameRenderer: {name} must be > 0, got {v!r}")
        width = getattr(decoder, "W", None)
        if width not in (128, 256):
            raise ValueError(f"FrameRenderer: decoder width {width!r} unsupported (128, 256)")
        self.params = [p.detach() for p in decoder.fused_params()]
        check_map(map_states, self.params)
        self.handle = None
        self.tile_rays = tile_rays
        self.width = width
        self.dev = map_states["voxel_vertex_emb"].device
        d = MapDesc()
        for i in range(10):
            d.dec[i] = self.params[i].data_ptr()
        d.width = width
        d.voxel_size, d.step_size, d.max_distance, d.truncation = voxel_size, step_size, max_distance, truncation
        d.max_depth = 10.0
        self.desc = d
        self.packed = None
        self.stats = (_i64 * len(STAT_NAMES))()
        self._dirs = {}
        self.refresh(map_states)
        h = L.lib().psvo_engine_new()
        if not h:
            raise L.PsvoError("psvo_engine_new failed")
        self.handle = _vp(h)

    def refresh(self, map_states):
        """Take the map's arrays again (after the map has grown) and rebuild
        the packed node records the traversal reads."""
        check_map(map_states, self.params)
        self.emb = map_states["voxel_vertex_emb"].detach()
        self.centres = map_states["voxel_center_xyz"].float().contiguous()
        self.structure = map_states["voxel_structure"].int().contiguous()
        self.vertex_idx = map_states["voxel_vertex_idx"].int().contiguous()
        d = self.desc
        d.n_nodes = self.centres.shape[0]
        d.centres, d.structure, d.vertex_idx = (t.data_ptr() for t in (self.centres, self.structure,
                                                                        self.vertex_idx))
        d.emb, d.n_emb = self.emb.data_ptr(), self.emb.shape[0]
        n = self.centres.shape[0]
        self.packed = torch.empty(n * 32, dtype=torch.uint8, device=self.dev)
        ws = torch.empty(int(L.lib().psvo_pack_tree_workspace_ints(n)), dtype=torch.int32, device=self.dev)
        L.call("psvo_pack_tree", L.stream_of(self.dev), n, self.centres, self.structure, ws, self.packed)
        d.packed = self.packed.data_ptr()

    # ---- the C call -------------------------------------------------------
    def _call(self, ro, rd, nz, seed, flags, color, depth, raw, mask):
        opts = RenderOpts(self.tile_rays, flags)
        rc = L.lib().psvo_render_frame(self.handle, L.stream_of(self.dev), ctypes.addressof(self.desc), ro.shape[0],
                                       ro.data_ptr(), rd.data_ptr(), nz.data_ptr() if nz is not None else None,
                                       int(seed), ctypes.addressof(opts),
                                       *(t.data_ptr() if t is not None else None for t in (color, depth, raw, mask)),
                                       ctypes.addressof(self.stats))
        if rc != 0:
            raise L.PsvoError(f"psvo_render_frame failed (code {rc}): {L.lib().psvo_last_error().decode()}")
        return dict(zip(STAT_NAMES, (int(v) for v in self.stats)))

    def render_rays(self, rays_o, rays_d, noise=None, seed=None):
        """World rays [R,3] (or [1,R,3]) → {"color" [R,3], "depth" [R],
        "ray_mask" [R] bool, "raw" [R] (z_min), "stats"}, original ray order,
        zeros where a ray hits nothing.  noise: the sampler's uniforms [200, K',
        max_steps] in the frame's layout (checked against the frame's own R_hit
        and max_steps before it is read), else drawn on the device from seed
        (None: a fresh one)."""
        if self.handle is None:
            raise ValueError("FrameRenderer: closed")
        n = check_rays(rays_o, rays_d, self.dev)
        if noise is not None:
            check_noise(noise)
        ro = rays_o.reshape(-1, 3).contiguous()
        rd = rays_d.reshape(-1, 3).contiguous()
        nz = None
        if noise is not None:
            q = self._call(ro, rd, None, 0, QUERY_ONLY, None, None, None, None)
            if q["r_hit"] > 0:
                check_noise(noise, q["r_hit"], q["max_steps"])
                nz = noise.to(device=self.dev, dtype=torch.float32).contiguous()
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        color = torch.empty((n, 3), dtype=torch.float32, device=self.dev)
        depth = torch.empty((n,), dtype=torch.float32, device=self.dev)
        raw = torch.empty((n,), dtype=torch.float32, device=self.dev)
        mask = torch.empty((n,), dtype=torch.uint8, device=self.dev)
        stats = self._call(ro, rd, nz, seed, 0, color, depth, raw, mask)
        return {"color": color, "depth": depth, "ray_mask": mask.bool(), "raw": raw, "stats": stats}

    def rays_of(self, pose_c2w, K, w, h, src_wh=None):
        """The frame's world rays as render_debug_images forms them: the cached
        camera directions @ Rᵀ, origin t → rays_o, rays_d [h·w, 3]."""
        check_camera(pose_c2w, K, w, h, src_wh)
        key = (tuple(float(K[i][j]) for i in range(3) for j in range(3)), w, h,
               None if src_wh is None else (float(src_wh[0]), float(src_wh[1])))
        dirs = self._dirs.get(key)
        if dirs is None:
            dirs = self._dirs[key] = camera_dirs(K, w, h, src_wh, self.dev)
        T = torch.as_tensor(pose_c2w, dtype=torch.float32).to(self.dev)
        rays_d = (dirs @ T[:3, :3].transpose(-1, -2)).reshape(-1, 3).contiguous()
        rays_o = T[:3, 3].reshape(1, 3).expand_as(rays_d).contiguous()
        return rays_o, rays_d

    def render(self, pose_c2w, K, w, h, src_wh=None, noise=None, seed=None):
        """-> color [h,w,3], depth [h,w,1], mask [h,w] (the images
        render_debug_images builds with fill_in)."""
        rays_o, rays_d = self.rays_of(pose_c2w, K, w, h, src_wh)
        out = self.render_rays(rays_o, rays_d, noise=noise, seed=seed)
        self.last_stats = out["stats"]
        return out["color"].view(h, w, 3), out["depth"].view(h, w, 1), out["ray_mask"].view(h, w)

    def evaluate(self, pose_c2w, K, rgb, depth, seed=None):
        """Image PSNR and depth L1 of the map's render against a frame's rgb
        [H,W,3] (in [0,1]) / depth [H,W], over the pixels the map covers and
        the sensor measured (mask & depth > 0); coverage: their share of the
        frame.  Torch ops on the device, one read-back."""
        if not (isinstance(rgb, torch.Tensor) and rgb.dim() == 3 and rgb.shape[2] == 3):
            raise ValueError(f"evaluate: rgb must be [H,W,3], got {tuple(getattr(rgb, 'shape', ()))}")
        H, W = int(rgb.shape[0]), int(rgb.shape[1])
        if not (isinstance(depth, torch.Tensor) and tuple(depth.shape) == (H, W)):
            raise ValueError(f"evaluate: depth must be [{H},{W}], got {tuple(getattr(depth, 'shape', ()))}")
        color, rdepth, mask = self.render(pose_c2w, K, W, H, seed=seed)
        gt_rgb = rgb.to(device=self.dev, dtype=torch.float32)
        gt_d = depth.to(device=self.dev, dtype=torch.float32)
        valid = mask & (gt_d > 0)
        n = valid.sum()
        mse = ((color - gt_rgb)[valid] ** 2).mean()
        l1 = (rdepth[..., 0] - gt_d)[valid].abs().mean()
        res = torch.stack([-10.0 * torch.log10(mse), l1, n.float() / float(H * W)]).cpu()
        return {"psnr": float(res[0]), "depth_l1": float(res[1]), "coverage": float(res[2])}

    def close(self):
        if getattr(self, "handle", None) is not None:
            L.lib().psvo_engine_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
