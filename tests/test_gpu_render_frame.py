"""The whole-frame renderer (psvo.render.FrameRenderer, csrc/render.hip)
against the CPU oracle's render_rays on the whole ray batch with the same
sampler noise: tests/render_case.py's 40 x 32 frames of tests/surface_case.py's
map (a decoder whose sdf is the scene's, so first crossings lie inside the
ray, at the padding, or nowhere), tiled so that several tiles, partial tiles
and a single tile all occur.  Discrete results (hit mask, z_min) are exact,
colour and depth meet DESIGN §7g's fp64 bound."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _renderer(tile_rays, params=None, width=128):
    import surface_case as S
    from psvo.decoder import Decoder
    from psvo.octree import map_states
    from psvo.render import FrameRenderer
    _, tree, emb, p0, _ = S.surface_case()
    dec = Decoder(depth=2, width=width, in_dim=16, skips=[], embedder="none").to(DEV)
    dec.load_state_dict(p0 if params is None else params)
    ms = map_states(tree, emb.clone().to(DEV), S.VOXEL, device=DEV)
    return FrameRenderer(ms, dec, S.VOXEL, S.STEP, truncation=S.TR, max_distance=10.0, tile_rays=tile_rays), ms, dec


def _render(fr, ro, rd, noise=None, seed=None):
    out = fr.render_rays(ro.to(DEV), rd.to(DEV), noise=noise, seed=seed)
    torch.cuda.synchronize()
    return out


def _same(a, b, label):
    for k in ("color", "depth", "raw", "ray_mask"):
        assert torch.equal(a[k], b[k]), f"{label}: {k} differs"


def test_oracle_parity_all_regimes():
    import render_case as C
    ro, rd, noise, pair = C.frame("seed0")
    o32, o64 = pair[torch.float32], pair[torch.float64]
    reg = C.regimes(o32)
    print("regimes", reg)
    assert min(reg["inside"], reg["padding"], reg["none"]) >= 0.10, reg  # the fixture cannot silently degrade
    assert torch.equal(o32["first"], o64["first"])
    fr, _, _ = _renderer(256)
    out = _render(fr, ro, rd, noise)
    C.check_against_oracle(out, pair, "seed0 / tile 256")
    st = out["stats"]
    assert st["r_hit"] == 1280 and st["n_tiles"] == 5 and st["S_max"] == o32["s_max"]
    assert st["M"] == reg["M"] and st["M_composited"] == reg["composited"], (st, reg)
    fr.close()


def test_tile_invariance():
    import render_case as C
    import surface_case as S
    from psvo.render import tile_bytes
    from psvo.render_helpers import render_rays
    ro, rd, noise, _ = C.frame("seed0")
    outs = {}
    for tile, n_tiles in ((64, 20), (200, 7), (333, 4), (1 << 20, 1)):
        fr, ms, dec = _renderer(tile)
        a = _render(fr, ro, rd, noise)
        b = _render(fr, ro, rd, None, seed=7)
        for o in (a, b):
            st = o["stats"]
            assert st["n_tiles"] == n_tiles, (tile, st)
            assert st["tile_bytes"] == tile_bytes(tile, st["max_steps"], 128), (tile, st)
        outs[tile] = (a, b)
        fr.close()
    for tile in (200, 333, 1 << 20):
        _same(outs[tile][0], outs[64][0], f"noise, tile {tile} vs 64")
        _same(outs[tile][1], outs[64][1], f"seed 7, tile {tile} vs 64")
    # the autograd-shaped path on the whole batch with the same seed
    with torch.no_grad():
        ref = render_rays(ro.to(DEV)[None], rd.to(DEV)[None], ms, dec, None, S.STEP, S.VOXEL, S.TR, 10, 10.0, seed=7,
                          return_raw=True)
    got = outs[64][1]
    mask = ref["ray_mask"].view(-1)
    assert torch.equal(got["ray_mask"], mask)
    assert torch.equal(got["raw"][mask], ref["raw"].view(-1))
    torch.testing.assert_close(got["color"][mask], ref["color"], rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(got["depth"][mask], ref["depth"].view(-1), rtol=1e-4, atol=1e-5)


def test_frame_wide_s_max():
    """A decoder whose sdf is negative on every sample: a ray crosses into the
    padding (z_min = its last depth) unless its sample count is the FRAME's
    maximum (then z_min = its first depth) — a tile-local maximum gets every
    ray wrong that attains its own tile's."""
    import render_case as C
    from oracle import oracle as O
    ro, rd, noise, _ = C.frame("seed0")
    params = O.decoder_params_init(128, seed=1)
    params["sdf_out.bias"][0] -= 0.5
    pair = C.oracle_pair(ro, rd, params, noise)
    o32, o64 = pair[torch.float32], pair[torch.float64]
    assert float(o32["sdf"][o32["valid"]].max()) < 0.0
    ns, s_max = o32["ns"], o32["s_max"]
    attain = sum(int(((t == t.max()) & (t < s_max)).sum()) for t in ns.split(64))
    print("rays at their 64-row tile's maximum but below the frame's:", attain, "at the frame's:",
          int((ns == s_max).sum()))
    assert attain >= 3
    last = o32["z"].gather(1, (ns - 1)[:, None])[:, 0]
    assert torch.equal(o32["z_min"], torch.where(ns < s_max, last, o32["z"][:, 0]))
    ok = o32["first"] == o64["first"]  # near ties leave the continuous comparison (cap 1 %)
    assert int((~ok).sum()) <= C.NEAR_TIE_CAP * ok.numel()
    fr, _, _ = _renderer(64, params)
    out = _render(fr, ro, rd, noise)
    C.check_against_oracle(out, pair, "negative sdf / tile 64", ok)
    fr.close()


def test_partial_and_empty_views():
    import render_case as C
    ro, rd, noise, pair = C.frame("seed0")
    fr, _, _ = _renderer(64)
    first = _render(fr, ro, rd, noise)
    uo, ud, unoise, upair = C.frame("up")
    out = _render(fr, uo, ud, unoise)
    mask = out["ray_mask"].cpu()
    assert int(mask.sum()) == 520 and int((~mask.view(C.H, C.W)).all(1).sum()) >= 19  # whole image rows missing
    C.check_against_oracle(out, upair, "up / tile 64")
    ao, ad, anoise, apair = C.frame("away")
    assert apair is None
    out = _render(fr, ao, ad, None, seed=3)
    assert out["stats"]["r_hit"] == 0
    for k in ("color", "depth", "raw", "ray_mask"):
        assert float(out[k].float().abs().sum()) == 0.0, k
    # no state leaks from the partial and the empty frame
    again = _render(fr, ro, rd, noise)
    _same(again, first, "seed0 after up / away")
    C.check_against_oracle(again, pair, "seed0 again / tile 64")
    fr.close()


def test_width_256():
    import render_case as C
    ro, rd, noise, _ = C.frame("seed9", 24, 16)
    params = C.passthrough_params(256, seed=1)
    pair = C.oracle_pair(ro, rd, params, noise)
    o32, o64 = pair[torch.float32], pair[torch.float64]
    assert int(o32["mask"].sum()) == 384
    ok = o32["first"] == o64["first"]
    assert int((~ok).sum()) <= C.NEAR_TIE_CAP * ok.numel()
    fr, _, _ = _renderer(100, params, width=256)
    out = _render(fr, ro, rd, noise)
    assert out["stats"]["n_tiles"] == 4
    C.check_against_oracle(out, pair, "width 256 / tile 100", ok)
    fr.close()


def test_render_and_evaluate():
    import render_case as C
    import surface_case as S
    scene = S.surface_case()[0].scene
    K, src = C.scene_K(scene)
    T = np.asarray(C.poses()["seed0"])
    fr, _, _ = _renderer(256)
    w, h = C.W, C.H
    color, depth, mask = fr.render(T, K, w, h, src, seed=11)
    assert color.shape == (h, w, 3) and depth.shape == (h, w, 1) and mask.shape == (h, w)
    # the rays as frame.get_rays / render_debug_images form them, written out here
    fx, fy, cx, cy = K[0, 0] * w / src[0], K[1, 1] * h / src[1], K[0, 2] * w / src[0], K[1, 2] * h / src[1]
    ix, iy = torch.meshgrid(torch.arange(w, device=DEV), torch.arange(h, device=DEV), indexing="xy")
    d_cam = torch.stack([(ix - cx) / fx, (iy - cy) / fy, torch.ones_like(ix)], -1).float()
    Tt = torch.as_tensor(T, dtype=torch.float32).to(DEV)
    rays_d = (d_cam @ Tt[:3, :3].transpose(-1, -2)).reshape(-1, 3)
    rays_o = Tt[:3, 3].reshape(1, 3).expand_as(rays_d).contiguous()
    out = fr.render_rays(rays_o, rays_d, seed=11)
    assert torch.equal(color.reshape(-1, 3), out["color"]) and torch.equal(depth.reshape(-1), out["depth"])
    assert torch.equal(mask.reshape(-1), out["ray_mask"])
    # evaluate against images made from the oracle's own colour and depth
    _, _, _, pair = C.frame("seed0")
    o32 = pair[torch.float32]
    omask = o32["mask"]
    rgb = torch.zeros(h * w, 3)
    rgb[omask] = o32["color"]
    gt_d = torch.zeros(h * w)
    gt_d[omask] = o32["depth"]
    gt_d[::7] = 0.0  # pixels without a sensor depth leave the statistics
    K_img = K.copy()  # the 40 x 32 images' own intrinsics
    K_img[0] *= w / src[0]
    K_img[1] *= h / src[1]
    ev = fr.evaluate(T, K_img, rgb.view(h, w, 3), gt_d.view(h, w), seed=11)
    valid = mask.reshape(-1) & (gt_d.to(DEV) > 0)
    mse = ((out["color"] - rgb.to(DEV))[valid] ** 2).mean()
    psnr = float(-10.0 * torch.log10(mse))
    l1 = float((out["depth"] - gt_d.to(DEV))[valid].abs().mean())
    print("evaluate", ev, "torch", psnr, l1)
    assert ev["psnr"] == pytest.approx(psnr, rel=1e-5)
    assert ev["depth_l1"] == pytest.approx(l1, rel=1e-5)
    assert ev["coverage"] == pytest.approx(float(valid.float().mean()), rel=1e-6)
    fr.close()
