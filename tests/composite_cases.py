"""Inputs and references of tests/test_gpu_composite.py and its CPU companion
(a helper module, no tests of its own).

One case = one launch: 70 hit rays out of 100, ragged sample counts, sorted z
with a padding of 10.0, per-sample sdf / colours of one profile family, and a
ground truth with a margin against the fp64 rendering.  The reference is
oracle.composite + oracle.criterion (torch, CPU) — in fp64 the truth, in fp32
the yardstick for what fp32 arithmetic costs on these inputs.  Everything is
cached per (family, S_max): built once, shared, never modified."""
import functools

import numpy as np
import torch

from oracle import oracle as O

R, R_HIT = 100, 70
TR, MAX_DEPTH = 0.1, 10.0
CRIT = O.REPLICA_CRITERIA
# the wave stride and each side of k_composite_loss's J = 2 / 4 / 8 / 0 variants (S_max = 1: argmax undefined)
S_MAXES = (2, 64, 65, 128, 129, 256, 257, 512, 513)
FAMILIES = ("surface", "none_pos", "none_neg", "first", "noise", "zeros", "ties", "depth_edges")
DEPTH_EDGES = (-0.3, 0.0, 0.005, 0.01, 9.95, 10.0, 10.5)
MARGIN = 1e-4


def _seed(family, s_max):
    return 1000 * FAMILIES.index(family) + s_max


def _profile(z, ns, k, g):
    """sdf ≈ clamp((d0 − z)/tr, ±1)·0.8 + noise with d0 between samples k and
    k + 1 of each ray (one crossing, at k; ns = 1: all positive)."""
    r_hit, s_max = z.shape
    k1 = torch.clamp(k + 1, max=s_max - 1)
    d0 = 0.5 * (z.gather(1, k[:, None]) + z.gather(1, k1[:, None]))
    d0 = torch.where((ns > 1)[:, None], d0, torch.full_like(d0, 20.0))
    return torch.clamp((d0 - z) / TR, -1.0, 1.0) * 0.8 + torch.randn(z.shape, generator=g) * 0.005


def _tie_depth(zk, sign):
    """An fp32 d with fl32(d − sign·tr) == zk bit for bit, or None (zk not
    reachable: d lies in a coarser binade)."""
    tr = np.float32(TR)
    zk = np.float32(zk)
    d = np.float32(zk + tr) if sign > 0 else np.float32(zk - tr)
    for _ in range(9):
        v = np.float32(d - tr) if sign > 0 else np.float32(d + tr)
        if v == zk:
            return float(d)
        d = np.nextafter(d, np.float32(np.inf) if v < zk else np.float32(-np.inf), dtype=np.float32)
    return None


@functools.lru_cache(maxsize=None)
def make_case(family, s_max):
    """The launch's inputs (fp32 / int32 CPU tensors) plus what the family
    constructed: "k" the intended first index per ray (−1: unspecified)."""
    g = torch.Generator().manual_seed(_seed(family, s_max))
    hit = torch.sort(torch.randperm(R, generator=g)[:R_HIT]).values
    ns = torch.randint(1, s_max + 1, (R_HIT,), generator=g)
    ns[0], ns[1], ns[2] = s_max, 1, min(2, s_max)
    # 0.02 spacing (0.0175 at S_max ≥ 512, so that every valid depth stays below the padding's 10.0)
    dz = min(0.02, 9.0 / s_max)
    col = torch.arange(s_max)[None, :]
    z0 = 0.3 + 0.5 * torch.rand(R_HIT, 1, generator=g)
    z = (z0 + dz * (col + 0.5 * (torch.rand(R_HIT, s_max, generator=g) - 0.5))).float()
    valid = col < ns[:, None]
    assert bool((z[:, 1:] > z[:, :-1]).all()) and float(z.max()) < 10.0
    # the crossing of the profile families: at 20–80 % of ns
    u = 0.2 + 0.6 * torch.rand(R_HIT, generator=g)
    k = torch.clamp((u * ns).long(), max=ns - 2).clamp(min=0)
    k_want = torch.full((R_HIT,), -1, dtype=torch.long)
    if family in ("surface", "ties", "depth_edges", "zeros"):
        sdf = _profile(z, ns, k, g)
        k_want = torch.where(ns > 1, k, torch.zeros_like(k))
    elif family == "none_pos":
        sdf = 0.05 + torch.randn(R_HIT, s_max, generator=g).abs() * 0.3
        k_want = torch.zeros(R_HIT, dtype=torch.long)
    elif family == "none_neg":
        sdf = -(0.05 + torch.randn(R_HIT, s_max, generator=g).abs() * 0.3)
        k_want = torch.where(ns < s_max, ns - 1, torch.zeros_like(ns))
    elif family == "first":
        sdf = -(0.05 + torch.randn(R_HIT, s_max, generator=g).abs() * 0.3)
        sdf[:, 0] = torch.where(ns > 1, sdf[:, 0].abs(), sdf[:, 0])
        k_want = torch.zeros(R_HIT, dtype=torch.long)
    elif family == "noise":
        sdf = torch.randn(R_HIT, s_max, generator=g) * 0.3
    if family == "zeros":
        # ±0 singles anywhere but at the crossing pair; before it, where they fit, the triple (1e-30, −1e-30, −0):
        # 1e-30·−1e-30 underflows to −0 in fp32 and −0·x is −0 — negative sign bits, none of them < 0; and, on
        # the rays with r % 4 == 3, the pair (1e-20, −1e-20) whose fp32 product −1e-40 is a denormal < 0:
        # a crossing, earlier than the profile's
        for r in range(R_HIT):
            n, kr = int(ns[r]), int(k[r])
            for s in torch.randperm(n, generator=g)[: max(1, n // 8)].tolist():
                if n > 1 and s in (kr, kr + 1):
                    continue
                sdf[r, s] = 0.0 if s % 2 else -0.0
            if kr >= 6:
                sdf[r, 1:5] = torch.tensor([0.3, 1e-30, -1e-30, -0.0])
                if r % 4 == 3:
                    sdf[r, 0:2] = torch.tensor([1e-20, -1e-20])
                    sdf[r, 2] = -0.0
                    k_want[r] = 0
    tie_zmin = torch.zeros(R_HIT, dtype=torch.bool)
    if family == "ties":
        # rays r % 3 == 0: the first sample beyond the window sits exactly on its edge fl32(z_min + tr): the
        # comparison is strict, it is not composited
        zmin = z.gather(1, k_want[:, None])[:, 0]
        edge = zmin + TR  # fp32 + python scalar: the fp32 sum the reference and the kernels form
        j = ((z < edge[:, None]) & valid).long().sum(1)  # the first sample at or beyond the edge
        for r in range(0, R_HIT, 3):
            jr = int(j[r])
            if int(ns[r]) > 1 and jr < int(ns[r]) and jr > int(k_want[r]):
                z[r, jr] = edge[r]
                tie_zmin[r] = True
        assert bool((z[:, 1:] > z[:, :-1]).all()) and int(tie_zmin.sum()) >= (10 if s_max >= 64 else 0)
    z = torch.where(valid, z, torch.full_like(z, MAX_DEPTH))
    sdf_s = sdf[valid].float().contiguous()
    rgb_s = torch.rand(int(ns.sum()), 3, generator=g)
    # ground truth: the fp64 rendering plus an offset of magnitude in [1e-3, 5e-2] and random sign
    c64 = O.composite(sdf_s.double(), rgb_s.double(), valid, z.double(), TR, torch.float64)

    def offset(shape):
        mag = 1e-3 * (50.0 ** torch.rand(shape, generator=g, dtype=torch.float64))
        return mag * (torch.randint(0, 2, shape, generator=g) * 2 - 1)

    gt_rgb, gt_depth = torch.rand(R, 3, generator=g), torch.rand(R, generator=g) * 6
    gt_rgb[hit] = (c64["color"] + offset((R_HIT, 3))).float()
    d_hit = (c64["depth"] + offset((R_HIT,))).float()
    depth_free = torch.ones(R_HIT, dtype=torch.bool)  # rays whose gt depth keeps the margin construction
    tie_front = torch.zeros(R_HIT, dtype=torch.bool)
    tie_back = torch.zeros(R_HIT, dtype=torch.bool)
    tie_k = torch.zeros(R_HIT, dtype=torch.long)
    if family == "depth_edges":
        d_hit = torch.tensor(DEPTH_EDGES)[torch.arange(R_HIT) % len(DEPTH_EDGES)]
        depth_free[:] = False
    if family == "ties":
        # rays r % 3 == 1: some z[k] == fl32(d − tr) (not in front: strict <); r % 3 == 2: z[k] == fl32(d + tr)
        # (not behind: strict >) — k beyond the composited window, so the sample's class hangs on the
        # comparison alone, and away from the rendered depth, so the depth margin holds
        for r in range(R_HIT):
            n, kr = int(ns[r]), int(k_want[r])
            cands = range(kr + 10, n) if r % 3 else ()  # beyond the composited window
            for kk in cands:
                d = _tie_depth(float(z[r, kk]), 1 if r % 3 == 1 else -1)
                if d is not None and d > 0.02:
                    d_hit[r] = d
                    (tie_front if r % 3 == 1 else tie_back)[r] = True
                    tie_k[r] = kk
                    break
    gt_depth[hit] = d_hit
    offsets = torch.zeros(R_HIT + 1, dtype=torch.int32)
    offsets[1:] = torch.cumsum(ns, 0)
    return dict(family=family, s_max=s_max, hit=hit, rank_ray=hit.to(torch.int32), ns=ns.to(torch.int32),
                offsets=offsets, z=z.contiguous(), valid=valid, sdf_s=sdf_s, rgb_s=rgb_s.contiguous(),
                gt_rgb=gt_rgb.contiguous(), gt_depth=gt_depth.contiguous(), k=k_want, depth_free=depth_free,
                tie_zmin=tie_zmin, tie_front=tie_front, tie_back=tie_back, tie_k=tie_k, M=int(ns.sum()))


def _outputs(c, comp, z):
    ray_mask = torch.zeros(1, R, dtype=torch.bool)
    ray_mask[0, c["hit"]] = True
    return {"color": comp["color"], "depth": comp["depth"], "sdf": comp["sdf"], "weights": comp["weights"],
            "z_vals": z, "ray_mask": ray_mask}


@functools.lru_cache(maxsize=None)
def reference(family, s_max, dtype):
    """oracle.composite + oracle.criterion + autograd in `dtype` on the
    case's fp32 inputs: weights, colour, depth, the loss and its parts, d loss
    / d sdf_s, d loss / d rgb_s, the padded sdf row, first and z_min."""
    c = make_case(family, s_max)
    sdf_s = c["sdf_s"].to(dtype).requires_grad_(True)
    rgb_s = c["rgb_s"].to(dtype).requires_grad_(True)
    z = c["z"].to(dtype)
    comp = O.composite(sdf_s, rgb_s, c["valid"], z, TR, dtype)
    loss, parts = O.criterion(_outputs(c, comp, z), c["gt_rgb"].to(dtype).view(1, R, 3),
                              c["gt_depth"].to(dtype).view(1, R), CRIT, TR, MAX_DEPTH)
    g_sdf_s, g_rgb_s = torch.autograd.grad(loss, [sdf_s, rgb_s])
    out = {k: v.detach() for k, v in comp.items()}
    out.update(loss=loss.detach(), g_sdf_s=g_sdf_s, g_rgb_s=g_rgb_s,
               **{k: v.detach() for k, v in parts.items()})
    return out


@functools.lru_cache(maxsize=None)
def cotangents(family, s_max):
    """Random cotangents for psvo_composite_bwd: colour, depth, weights, sdf."""
    g = torch.Generator().manual_seed(_seed(family, s_max) + 500000)
    return (torch.randn(R_HIT, 3, generator=g), torch.randn(R_HIT, generator=g),
            torch.randn(R_HIT, s_max, generator=g), torch.randn(R_HIT, s_max, generator=g))


@functools.lru_cache(maxsize=None)
def reference_bwd(family, s_max, dtype):
    """The vector-Jacobian product of oracle.composite for cotangents():
    (g_sdf_s [M], g_rgb_s [M,3])."""
    c = make_case(family, s_max)
    sdf_s = c["sdf_s"].to(dtype).requires_grad_(True)
    rgb_s = c["rgb_s"].to(dtype).requires_grad_(True)
    comp = O.composite(sdf_s, rgb_s, c["valid"], c["z"].to(dtype), TR, dtype)
    gs = [t.to(dtype) for t in cotangents(family, s_max)]
    return torch.autograd.grad([comp["color"], comp["depth"], comp["weights"], comp["sdf"]], [sdf_s, rgb_s],
                               grad_outputs=gs)


def bound(ref32, ref64):
    """max|gpu − ref64| may be 8 × the fp32 reference's own error (three bits
    for another summation order over ≤ 513 terms and a 1–2 ulp expf), and at
    least 32 ulp of the tensor's largest magnitude (where the fp32 reference
    happens to be exact)."""
    ref64 = ref64.double()
    err32 = float((ref32.double() - ref64).abs().max())
    return max(8.0 * err32, 32.0 * 2.0 ** -24 * float(ref64.abs().max()))


def masks(c):
    """The selection's classes from torch fp32 masks on the case's inputs:
    (composited, kept) [R_hit, S_max] bool, valid samples only."""
    ref = reference(c["family"], c["s_max"], torch.float32)
    z, valid = c["z"], c["valid"]
    d = c["gt_depth"][c["hit"]][:, None]
    comp = (z < ref["z_min"][:, None] + TR) & valid
    front = z < d - TR
    back = z > d + TR
    dm = (d > 0.0) & (d < MAX_DEPTH)
    return comp, (comp | front | (~back & dm)) & valid


def terms_live(c):
    """Both of the loss's balance weights 1 − n / (n_fs + n_sdf) are non-zero:
    the launch has samples in front and in the sdf band (the padding counts).
    Only then is every kept sample's reference gradient non-zero."""
    z = c["z"]
    d = c["gt_depth"][c["hit"]][:, None]
    front = z < d - TR
    band = ~front & ~(z > d + TR) & (d > 0.0) & (d < MAX_DEPTH)
    return bool(front.any()) and bool(band.any())
