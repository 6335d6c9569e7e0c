"""Frames for the whole-frame renderer's tests (a helper module, no tests of
its own): surface_case's map and decoder seen from three poses, their rays
formed as frame.get_rays / render_debug_images form them, and the oracle's
render_rays in fp32 and fp64 on the same rays and sampler noise (computed once
per frame and shared — about a second each on the CPU)."""
import functools

import numpy as np
import torch

import surface_case as sc
from oracle import oracle as O

W, H = 40, 32
NEAR_TIE_CAP = 0.01  # rays whose fp32 and fp64 first crossings may differ (the project's near-tie cap)


def scene_K(scene):
    k = scene.intrinsics
    return np.array([[k["fx"], 0.0, k["cx"]], [0.0, k["fy"], k["cy"]], [0.0, 0.0, 1.0]]), (k["W"], k["H"])


def frame_rays(T, K, w, h, src_wh):
    """frame.get_rays(w, h) @ Rᵀ, origin t (tracking.py:178-185) → [h·w, 3] each, CPU."""
    from psvo.render import camera_dirs
    T = torch.as_tensor(np.asarray(T), dtype=torch.float32)
    dirs = camera_dirs(K, w, h, src_wh)
    rays_d = (dirs @ T[:3, :3].transpose(-1, -2)).reshape(-1, 3).contiguous()
    rays_o = T[:3, 3].reshape(1, 3).expand_as(rays_d).contiguous()
    return rays_o, rays_d


def poses():
    """name -> camera-to-world pose: seed-0 (every ray hits), "up" (whole image
    rows miss), "away" (nothing hit), seed-9 (the width-256 frame)."""
    from psvo import synthetic as syn
    scene = sc.surface_case()[0].scene
    room = [b for b in scene.boxes if b.inside][0]
    lo, hi = np.asarray(room.lo, np.float64), np.asarray(room.hi, np.float64)
    c = 0.5 * (lo + hi)
    eye = np.array([hi[0] + 1.5, c[1], c[2]])
    return {"seed0": syn.camera_poses(scene, 1, seed=0)[0],
            "up": syn.look_at(eye, np.array([hi[0], c[1], hi[2] + 1.0])),
            "away": syn.look_at(eye, eye + np.array([1.0, 0.0, 0.0])),
            "seed9": syn.camera_poses(scene, 1, seed=9)[0]}


def passthrough_params(width, seed):
    """oracle.decoder_params_init(width) plus surface_case's pass-through unit
    (embedding channel 0 → the sdf output), so the sdf is the scene's."""
    p = O.decoder_params_init(width, seed=seed)
    e0 = torch.zeros(16)
    e0[0] = 1.0
    u0 = torch.zeros(width)
    u0[0] = 1.0
    p["pts_linears.0.weight"][0], p["pts_linears.0.bias"][0] = e0, 8.0
    p["pts_linears.1.weight"][0], p["pts_linears.1.bias"][0] = u0, 0.0
    p["sdf_out.weight"][0], p["sdf_out.bias"][0] = u0, -8.0
    return p


def oracle_pair(rays_o, rays_d, params, noise):
    """The oracle in fp32 and fp64 plus what the tests compare: per dtype the
    first sign change, z_min, colour, depth [R_hit, …] and the hit mask."""
    ms = sc.surface_case()[4]
    res = {}
    for dt in (torch.float32, torch.float64):
        o = O.render_rays(rays_o[None], rays_d[None], ms, params, sc.STEP, sc.VOXEL, sc.TR, sc.MAX_DEPTH, noise=noise,
                          sum_order="sequential", dtype=dt)
        sdf = o["sdf"].detach().float()
        cross = (sdf[:, 1:] * sdf[:, :-1]) < 0
        first = torch.argmax(cross.float(), dim=1)
        z = o["z_vals"].float()
        valid = o["samples"]["sampled_point_voxel_idx"].ne(-1)
        res[dt] = dict(color=o["color"].detach(), depth=o["depth"].detach(), first=first, any_cross=cross.any(1),
                       z_min=z.gather(1, first[:, None])[:, 0], ns=valid.sum(-1), s_max=valid.shape[1],
                       mask=o["ray_mask"].view(-1), z=z, valid=valid, sdf=sdf)
    return res


@functools.lru_cache(maxsize=None)
def frame(name, w=W, h=H, noise_seed=17):
    """(rays_o, rays_d [w·h, 3] CPU, noise or None, oracle pair or None) of the named pose."""
    w_, _, _, params, ms = sc.surface_case()
    K, src = scene_K(w_.scene)
    ro, rd = frame_rays(poses()[name], K, w, h, src)
    _, hits = O.ray_intersect_vox(ro[None], rd[None], ms["voxel_center_xyz"], ms["voxel_structure"], sc.VOXEL, 10.0)
    if int(hits.sum()) == 0:
        return ro, rd, None, None
    noise = sc.sampler_noise(ro[None], rd[None], ms, seed=noise_seed)
    return ro, rd, noise, oracle_pair(ro, rd, params, noise)


def regimes(o32):
    """Shares of the hit rays whose first crossing lies inside the ray, at the
    padding (first = ns − 1), or that have none; and the composited share."""
    f, ns, anyc = o32["first"], o32["ns"], o32["any_cross"]
    frac = lambda t: float(t.float().mean())  # noqa: E731
    comp = (o32["z"] < o32["z_min"][:, None] + sc.TR) & o32["valid"]
    return dict(inside=frac(anyc & (f < ns - 1)), padding=frac(anyc & (f == ns - 1)), none=frac(~anyc),
                composited=int(comp.sum()), M=int(o32["valid"].sum()))


def fp64_bound(ref32, ref64):
    """max|gpu − ref64| ≤ max(8·max|ref32 − ref64|, 32·2⁻²⁴·max|ref64|)."""
    return max(8.0 * float((ref32.double() - ref64).abs().max()), 32.0 * 2.0 ** -24 * float(ref64.abs().max()))


def check_against_oracle(out, pair, label, rays_ok=None):
    """ray_mask and raw exact; colour / depth within the fp64 bound (on the
    hit rays rays_ok, default all).  Prints each figure before asserting."""
    o32, o64 = pair[torch.float32], pair[torch.float64]
    mask = out["ray_mask"].cpu()
    assert torch.equal(mask, o32["mask"]), f"{label}: ray_mask"
    raw = out["raw"].cpu()[mask]
    n_bad = int((raw != o32["z_min"]).sum())
    print(f"{label}: raw mismatches {n_bad} / {raw.numel()}")
    assert n_bad == 0, f"{label}: raw (z_min) differs from the oracle on {n_bad} rays"
    keep = torch.ones(raw.numel(), dtype=torch.bool) if rays_ok is None else rays_ok
    for k in ("color", "depth"):
        got = out[k].cpu()[mask].double()[keep]
        r32, r64 = o32[k][keep], o64[k][keep]
        err, bound = float((got - r64).abs().max()), fp64_bound(r32, r64)
        print(f"{label}: {k} err {err:.3e} bound {bound:.3e} (ref32 err {float((r32.double() - r64).abs().max()):.3e})")
        assert err <= bound, f"{label}: {k} error {err:.3e} > bound {bound:.3e}"
    miss = ~mask
    for k in ("color", "depth", "raw"):
        assert float(out[k].cpu()[miss].abs().sum()) == 0.0, f"{label}: {k} of missed rays not 0"
