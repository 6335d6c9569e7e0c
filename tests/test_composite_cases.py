"""The inputs of tests/test_gpu_composite.py have the properties their
families promise — from the reference alone (oracle.composite +
oracle.criterion on the CPU), so that a GPU failure there is the kernels'."""
import numpy as np
import pytest
import torch

import composite_cases as C


@pytest.mark.parametrize("family", C.FAMILIES)
def test_family_properties(family):
    for s_max in C.S_MAXES:
        c = C.make_case(family, s_max)
        r32, r64 = C.reference(family, s_max, torch.float32), C.reference(family, s_max, torch.float64)
        ns, first, k = c["ns"].long(), r32["first"], c["k"]
        tag = (family, s_max)
        # the launch's shape
        assert c["z"].shape == (C.R_HIT, s_max) and c["rank_ray"].shape == (C.R_HIT,)
        assert bool((c["rank_ray"][1:] > c["rank_ray"][:-1]).all()) and int(c["rank_ray"][-1]) < C.R
        assert not torch.equal(c["rank_ray"], torch.arange(C.R_HIT, dtype=torch.int32))  # a real indirection
        assert ns.tolist()[:3] == [s_max, 1, min(2, s_max)] and int(ns.min()) >= 1 and int(ns.max()) <= s_max
        assert bool((c["z"][~c["valid"]] == 10.0).all()) and float(c["z"][c["valid"]].max()) < 10.0
        zz = c["z"]
        assert bool((zz[:, 1:] >= zz[:, :-1]).all())
        # fp32 and fp64 make the same discrete decisions; the padded row is the fp32 values
        assert torch.equal(first, r64["first"]), tag
        assert torch.equal(r32["z_min"].double(), r64["z_min"]), tag
        assert torch.equal(r32["weights"] == 0, r64["weights"] == 0), tag
        assert torch.equal(r32["sdf"].double(), r64["sdf"]), tag
        # the family's first index
        spec = k >= 0
        assert torch.equal(first[spec], k[spec]), tag
        if family in ("surface", "ties", "depth_edges"):
            assert bool((first[ns >= 20] >= 4).all()), tag
            assert bool(((first >= 0.2 * ns - 1) & (first <= 0.8 * ns))[ns > 1].all()), tag
            if s_max >= 256:
                assert 10 * int((first >= 4).sum()) >= 9 * C.R_HIT, tag
        if family == "none_pos":
            assert bool((c["sdf_s"] > 0).all()) and bool((first == 0).all()), tag
        if family == "none_neg":
            assert bool((c["sdf_s"] < 0).all()), tag
            assert torch.equal(first, torch.where(ns < s_max, ns - 1, torch.zeros_like(ns))), tag
        if family == "first":
            assert bool((first == 0).all()), tag
            w_on = (r32["weights"] > 0).sum(1)
            assert bool((w_on >= 1).all()), tag
        if family == "noise" and s_max >= 64:
            assert float((first <= 1).float().mean()) > 0.6, tag  # today's regime: the crossing at the ray's start
        if family == "zeros":
            s = c["sdf_s"]
            assert int((s == 0).sum()) >= C.R_HIT // 2, tag
            if s_max >= 64:
                assert bool((torch.signbit(s) & (s == 0)).any()) and bool((~torch.signbit(s) & (s == 0)).any()), tag
                # a product with a negative sign bit that is not < 0: −0, and the underflowing 1e-30·−1e-30
                sd = r32["sdf"]
                prod = sd[:, 1:] * sd[:, :-1]
                before = torch.arange(s_max - 1)[None, :] < first[:, None]
                fake = torch.signbit(prod) & ~(prod < 0) & before
                assert int(fake.any(1).sum()) >= 10, tag
                assert int(((sd[:, 1:] == -1e-30) & (sd[:, :-1] == 1e-30) & before).any(1).sum()) >= 5, tag
                # and a denormal product that is < 0: the crossing
                den = (prod < 0) & (prod.abs() < 1.1754944e-38)
                assert int(den[:, 0].sum()) >= 3 and bool((first[den[:, 0]] == 0).all()), tag
        if family == "ties" and s_max >= 64:
            d = c["gt_depth"][c["hit"]]
            z = c["z"]
            edge = r32["z_min"] + C.TR
            on_edge = ((z == edge[:, None]) & c["valid"]).any(1)
            assert torch.equal(on_edge, c["tie_zmin"]) and int(on_edge.sum()) >= 10, tag
            assert bool((r32["weights"][z == edge[:, None]] == 0).all()), tag  # strict <: not composited
            zk = z.gather(1, c["tie_k"][:, None])[:, 0]
            assert int(c["tie_front"].sum()) >= 5 and int(c["tie_back"].sum()) >= 5, tag
            assert bool((zk == d - C.TR)[c["tie_front"]].all()) and bool((zk == d + C.TR)[c["tie_back"]].all()), tag
            comp, kept = C.masks(c)
            at = torch.zeros_like(comp)
            at[torch.arange(C.R_HIT), c["tie_k"]] = True
            ties = at & (c["tie_front"] | c["tie_back"])[:, None]
            assert bool(kept[ties].all()) and not bool(comp[ties].any()), tag  # in the sdf band by the strictness alone
        if family == "depth_edges":
            d = c["gt_depth"][c["hit"]]
            assert sorted(set(d.tolist())) == sorted(float(np.float32(v)) for v in C.DEPTH_EDGES), tag
            if s_max >= 64:
                # at 9.95 the padded samples lie in the sdf band and count in the loss value
                pad_band = (~c["valid"]) & (d == np.float32(9.95))[:, None]
                assert int(pad_band.sum()) > 0, tag
                zz, dd = c["z"][pad_band], d[:, None].expand_as(c["z"])[pad_band]
                assert bool(((zz >= dd - C.TR) & (zz <= dd + C.TR)).all()), tag
        # the ground truth's margins: sign(gt − rendered) cannot flip under fp32 rounding
        gt_c = c["gt_rgb"][c["hit"]].double()
        d_hit = c["gt_depth"][c["hit"]].double()
        assert float((gt_c - r64["color"]).abs().min()) >= C.MARGIN, tag
        assert float((gt_c - r32["color"].double()).abs().min()) >= 0.5 * C.MARGIN, tag
        dm = (d_hit - r64["depth"]).abs()
        if family == "depth_edges":
            valid_d = (d_hit > 0.01) & (d_hit < C.MAX_DEPTH)
            assert int(valid_d.sum()) >= 5 and float(dm[valid_d].min()) >= C.MARGIN, tag
        else:
            assert float(dm.min()) >= C.MARGIN, tag
            if family != "ties":
                assert float(dm.max()) <= 5.1e-2, tag
        # the loss terms are live.  Where no sample of the launch lies in front of its ray's depth (S_max = 2; no
        # crossing or a crossing at index 0: the window starts at the first sample and d − tr lies before it), the
        # sdf term's balance weight 1 − n_sdf / (n_fs + n_sdf) and with it every band sample's gradient is exactly 0
        live = C.terms_live(c)
        assert live or s_max < 64 or family in ("none_pos", "first"), tag
        for key in ("color_loss", "depth_loss") + (("fs_loss", "sdf_loss") if live else ()):
            assert np.isfinite(float(r64[key])) and float(r64[key]) > 0, (tag, key)
        # the selection's classes: non-trivial where the rays are long enough
        comp, kept = C.masks(c)
        assert bool((comp <= kept).all()) and bool((kept <= c["valid"]).all())
        assert torch.equal(comp, (r32["weights"] > 0)), tag  # u = σσ never underflows here
        # a dropped sample's reference gradients are exactly zero, a kept one's are not
        zero = (r64["g_sdf_s"] == 0) & (r64["g_rgb_s"] == 0).all(-1)
        assert bool(zero[~kept[c["valid"]]].all()), tag
        if live:
            assert torch.equal(zero, ~kept[c["valid"]]), tag


def test_fp32_reference_error_is_rounding_sized():
    """The fp32 formulation's own error on these inputs: ≤ 1e-6·max for
    colour, depth, weights and g_rgb, ≤ 2e-5·max for g_sdf (σ(a)σ(−a)(σ(−a) −
    σ(a)) cancels near sdf = 0), ≤ 1e-5 of the loss (|d − depth| cancels two
    numbers up to 1e4 × larger than itself).  The bound of the GPU test is 8 ×
    the measured figure per tensor, so this pins that the measured figures
    are of fp32 rounding size: no family sits at a discontinuity."""
    worst = {}
    for family in C.FAMILIES:
        for s_max in C.S_MAXES:
            r32, r64 = C.reference(family, s_max, torch.float32), C.reference(family, s_max, torch.float64)
            for key in ("loss", "color", "depth", "weights", "g_rgb_s", "g_sdf_s"):
                rel = float((r32[key].double() - r64[key]).abs().max() / r64[key].abs().max())
                worst[key] = max(worst.get(key, 0.0), rel)
    for key, v in worst.items():
        assert v <= {"g_sdf_s": 2e-5, "loss": 1e-5}.get(key, 1e-6), worst


def test_surface_case_regime():
    """tests/surface_case.py: the small engine batch is in the trained-map
    regime (oracle_regime asserts the conditions), from the oracle alone."""
    import surface_case as S
    outs, reg = S.oracle_regime()
    assert reg["hit"] == S.FRAMES * S.RAYS and reg["s_max"] > 128 and reg["M"] > 20000, reg
    g32, g64 = outs[torch.float32][3], outs[torch.float64][3]
    for k in ("embeddings", "rays_o", "rays_d", "sdf_out.weight"):  # the sdf path's gradients: fp32 rounding only
        assert float((g32[k].double() - g64[k]).abs().max()) <= 5e-5 * float(g64[k].abs().max()), k
