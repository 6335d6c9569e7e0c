"""A small mapping batch in the regime of a trained map (a helper module, no
tests of its own): room0, 2 frames × 256 rays, where the decoder's sdf is the
scene's signed distance, so that the first sign change of most rays lies
deep inside the ray — what the bench times and what the random decoders of
the small engine tests never produce (their crossing is at the padding, or
there is none).

Embedding channel 0 holds the exact box-union signed distance at each voxel
vertex ÷ truncation (the other channels randn·0.1); the decoder is
oracle.decoder_params_init(128, seed=4) plus one always-active pass-through
unit that hands channel 0 to the sdf output: W1[0] = e₀, b1[0] = 8; W2[0] =
unit(0), b2[0] = 0; sdf_out row 0 = unit(0), bias −8 (|channel 0| < 8, so
both ReLUs stay open — and no pre-activation is exactly zero, which a
relu(x) / relu(−x) pair would give every sample).  Every other unit stays
random."""
import functools

import numpy as np
import torch

from oracle import oracle as O

STEP, TR, VOXEL, MAX_DEPTH = 0.01, 0.1, 0.2, 10.0
FRAMES, RAYS = 2, 256


def _box_sdf(p, lo, hi):
    """Signed distance of points p [n,3] to the axis-aligned box (negative inside)."""
    c, h = 0.5 * (lo + hi), 0.5 * (hi - lo)
    q = np.abs(p - c) - h
    return np.linalg.norm(np.maximum(q, 0.0), axis=1) + np.minimum(q.max(axis=1), 0.0)


def scene_sdf(scene, p):
    """Signed distance to the union of the scene's solids: the furniture boxes
    and everything outside the `inside` shell (its box distance negated)."""
    d = np.full(p.shape[0], np.inf)
    for b in scene.boxes:
        s = _box_sdf(p, np.asarray(b.lo, np.float64), np.asarray(b.hi, np.float64))
        d = np.minimum(d, -s if b.inside else s)
    return d


@functools.lru_cache(maxsize=None)
def surface_case():
    """(workload, tree, embeddings [N,16] CPU, decoder params, oracle map
    states on the CPU)."""
    from psvo import synthetic as syn
    from psvo.octree import Octree, map_states
    w = syn.make_workload("room0", FRAMES, RAYS, seed=4)
    tree = Octree()
    tree.init(256, 16, VOXEL, 8)
    tree.insert(w.voxels)
    n = max(20000, tree.count_nodes())
    emb = torch.randn(n, 16, generator=torch.Generator().manual_seed(4)) * 0.1
    ms = map_states(tree, emb, VOXEL, device="cpu")
    vid = ms["voxel_vertex_idx"].long()                      # [N, 8]
    corners = O._CORNERS.double()                             # [8, 3]
    pos = ms["voxel_center_xyz"].double()[:, None, :] + (corners[None] - 0.5) * VOXEL
    ok = vid >= 0
    sd = scene_sdf(w.scene, pos[ok].numpy())
    emb[:, 0] = 0.0
    emb[vid[ok], 0] = torch.from_numpy(sd / TR).float()
    assert float(emb[:, 0].abs().max()) < 8.0
    params = O.decoder_params_init(128, seed=4)
    e0 = torch.zeros(16)
    e0[0] = 1.0
    u0 = torch.zeros(128)
    u0[0] = 1.0
    params["pts_linears.0.weight"][0], params["pts_linears.0.bias"][0] = e0, 8.0
    params["pts_linears.1.weight"][0], params["pts_linears.1.bias"][0] = u0, 0.0
    params["sdf_out.weight"][0], params["sdf_out.bias"][0] = u0, -8.0
    return w, tree, emb, params, ms


def sampler_noise(rays_o, rays_d, ms, step=STEP, seed=17):
    """Sampler noise for rays [1,R,3] in the layout the batch's sampler reads
    ([200, K', max ⌈Σ/step⌉ + P]), so that the engine and the oracle can be
    fed the same draws."""
    o_out, o_hits = O.ray_intersect_vox(rays_o, rays_d, ms["voxel_center_xyz"], ms["voxel_structure"], VOXEL, 10.0)
    hit = o_hits.view(-1)
    inter = {k: v[0][hit] for k, v in o_out.items()}
    dists = (inter["max_depth"] - inter["min_depth"]).masked_fill(inter["intersected_voxel_idx"].eq(-1), 0)
    p = dists.shape[-1]
    max_steps = int(torch.ceil(O.sequential_row_sums(dists) / np.float32(step)).max()) + p
    kp = (int(hit.sum()) + 199) // 200
    return torch.rand((200, kp, max_steps), generator=torch.Generator().manual_seed(seed)).clamp(0.001, 0.999)


def oracle_regime(rays_o=None, rays_d=None, noise=None):
    """The oracle's render + loss + backward of the case in fp32 and fp64 (on
    the workload's rays, or on the rays [1,R,3] the engine formed from its
    poses; `noise`: sampler_noise's draws, default: its own) and the regime it
    is in — whose conditions are asserted here:
      first crossing strictly inside (4 ≤ first < ns − 1)  ≥ 50 % of the hit rays
      first crossing into the padding (first = ns − 1)      ≥ 10 %
      no crossing                                           ≥ 1 %
      composited samples                                    25–60 % of M
      class B (kept, not composited)                        ≥ 20 % of M
      fp32 / fp64 first indices                             equal
    Returns ({dtype: render_and_backward's result}, regime dict with the
    composited / kept sample counts)."""
    w, tree, emb, params, ms = surface_case()
    rays_o = w.rays_o if rays_o is None else rays_o
    rays_d = w.rays_d if rays_d is None else rays_d
    noise = sampler_noise(rays_o, rays_d, ms) if noise is None else noise
    outs = {}
    for dt in (torch.float32, torch.float64):
        outs[dt] = O.render_and_backward(rays_o, rays_d, w.rgb.reshape(1, -1, 3), w.depth.reshape(1, -1), ms, params,
                                         STEP, VOXEL, TR, MAX_DEPTH, O.REPLICA_CRITERIA, noise=noise,
                                         sum_order="sequential", max_depth=MAX_DEPTH, dtype=dt)
    res = outs[torch.float32][0]
    mask = res["samples"]["sampled_point_voxel_idx"].ne(-1)
    ns, s_max = mask.sum(-1), mask.shape[1]
    first = {}
    for dt in outs:
        sdf = outs[dt][0]["sdf"].detach().float()
        cross = (sdf[:, 1:] * sdf[:, :-1]) < 0
        first[dt] = torch.argmax(cross.float(), dim=1)
    assert torch.equal(first[torch.float32], first[torch.float64])
    f, any_cross = first[torch.float32], cross.any(1)
    z = res["z_vals"]
    comp = (z < z.gather(1, f[:, None]) + TR) & mask
    d = w.depth.reshape(-1)[res["ray_mask"].view(-1)][:, None]
    kept = (comp | (z < d - TR) | (~(z > d + TR) & (d > 0.0) & (d < MAX_DEPTH))) & mask
    m = int(mask.sum())
    frac = lambda t: float(t.float().mean())  # noqa: E731
    reg = dict(hit=int(mask.shape[0]), M=m, s_max=s_max, inside=frac(any_cross & (f >= 4) & (f < ns - 1)),
               padding=frac(any_cross & (f == ns - 1)), none=frac(~any_cross), composited=int(comp.sum()),
               kept=int(kept.sum()))
    assert reg["inside"] >= 0.5 and reg["padding"] >= 0.1 and reg["none"] >= 0.01, reg
    assert 0.25 <= reg["composited"] / m <= 0.60 and (reg["kept"] - reg["composited"]) / m >= 0.20, reg
    return outs, reg
