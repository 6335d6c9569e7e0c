"""The mapping step's device-sized sdf trunk with the interpolation in its
operand load (k_mlp_sdf2<true, true>: one launch leaves the sdf, the h2 rows
and the [M,16] feature rows) against the two kernels it replaces
(k_interp_fwd, then k_mlp_sdf2<false> reading the feature rows): the same
bits, on its own at the unit / tile / empty-workgroup edges and inside the
engine against the PATH_INTERP_PASS schedule."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

SENTINEL = 0x7FC0BEEF  # a quiet NaN's bit pattern: compared as int32, never as a float
M_CAP_MIN = 4096       # 16 workgroups of 256 samples: at m_dev = 1 fifteen of them own nothing


def _setup():
    from psvo import synthetic as syn
    from psvo.decoder import Decoder
    from psvo.octree import Octree
    w = syn.make_workload("room0", 2, 512, seed=4)
    tree = Octree()
    tree.init(256, 16, 0.2, 8)
    tree.insert(w.voxels)
    g = torch.Generator().manual_seed(0)
    emb0 = torch.randn(max(20000, tree.count_nodes()), 16, generator=g) * 0.1
    torch.manual_seed(0)
    dec = Decoder(depth=2, width=128, in_dim=16, skips=[], embedder="none").to(DEV)
    return w, tree, emb0, dec


def _frames_of(w, n):
    from oracle import oracle as O
    from psvo.pose import OptimizablePose
    poses, dirs = [], []
    rd = w.rays_d[0].double()
    for f, T in enumerate(w.poses):
        p = OptimizablePose.from_matrix(np.asarray(T)).data.detach().double()
        poses.append(p.float())
        dirs.append((rd[f * n:(f + 1) * n] @ O.se3_rotation(p)).float())
    return torch.stack(poses).contiguous().to(DEV), torch.cat(dirs).contiguous().to(DEV)


@pytest.fixture(scope="module")
def case():
    """64 rays of the small test octree queried once (shared, left unchanged):
    their samples, the map and a decoder."""
    from psvo import _lib as L
    from psvo.octree import map_states
    from psvo.render_helpers import query_samples
    w, tree, emb0, dec = _setup()
    ms = map_states(tree, emb0.clone().to(DEV), 0.2, device=DEV)
    ro = w.rays_o[:, :64].contiguous().to(DEV)
    rd = w.rays_d[:, :64].contiguous().to(DEV)
    smp = query_samples(ro, rd, ms, 0.01, 0.2, 10.0, seed=77)
    m = int(smp.m)
    assert m >= 2 * 256 + 5 + 1, m
    c = {
        "m": m, "m_cap": max(M_CAP_MIN, m),
        "leaf": smp.leaf, "t": smp.t, "ray_of": smp.ray_of_sample, "ray_index": smp.rank_ray32.contiguous(),
        "ro": ro.reshape(-1, 3).float().contiguous(), "rd": rd.reshape(-1, 3).float().contiguous(),
        "centres": ms["voxel_center_xyz"].float().contiguous(),
        "vertex_idx": ms["voxel_vertex_idx"].int().contiguous(),
        "emb": ms["voxel_vertex_emb"].detach().float().contiguous(),
        "dec": [p.detach().float().contiguous() for p in dec.fused_params()],
        "images": torch.empty(int(L.lib().psvo_mlp_image_floats()), dtype=torch.float32, device=DEV),
    }
    # the interpolation on its own (the host-sized pass) on every sample
    ref = torch.empty((m, 16), dtype=torch.float32, device=DEV)
    L.call("psvo_interp_fwd", L.stream_of(DEV), m, 16, 0.2, c["leaf"], c["t"], c["ray_of"], c["ray_index"], c["ro"],
           c["rd"], c["centres"], c["vertex_idx"], c["emb"], ref)
    torch.cuda.synchronize()
    c["feat_ref"] = ref.view(torch.int32).cpu()
    return c


def _run(c, fused, m_dev, m_cap):
    """One psvo_debug_trunk_interp call into sentinel-filled outputs of m_cap
    rows; returns (sdf [m_cap], h2 [m_cap,128], feat [m_cap,16]) as int32."""
    from psvo import _lib as L
    outs = [torch.full(shape, SENTINEL, dtype=torch.int32, device=DEV)
            for shape in ((m_cap,), (m_cap, 128), (m_cap, 16))]
    md = torch.tensor([m_dev], dtype=torch.int32, device=DEV)
    L.call("psvo_debug_trunk_interp", L.stream_of(DEV), int(fused), m_cap, md, c["leaf"], c["t"], c["ray_of"],
           c["ray_index"], c["ro"], c["rd"], c["centres"], c["vertex_idx"], c["emb"], 0.2, *c["dec"], c["images"],
           *outs)
    torch.cuda.synchronize()
    return [o.cpu() for o in outs]


@pytest.mark.parametrize("m_dev", [0, 1, 31, 32, 33, 255, 256, 257, 2 * 256 + 5, "all"])
def test_fused_trunk_matches_interp_pass_then_trunk(case, m_dev):
    """Rows < m_dev of sdf, h2 and feat: the fused launch and the two-kernel
    sequence give the same int32 bits, and feat is psvo_interp_fwd's; rows
    >= m_dev of all three outputs keep the sentinel (one m_cap >= 4096 for
    every m_dev: workgroups with empty unit ranges, partial units and tiles)."""
    c = case
    n = c["m"] if m_dev == "all" else m_dev
    two = _run(c, 0, n, c["m_cap"])
    one = _run(c, 1, n, c["m_cap"])
    for name, a, b in zip(("sdf", "h2", "feat"), one, two):
        assert torch.equal(a[:n], b[:n]), name
        assert bool((a[n:] == SENTINEL).all()), f"{name}: the fused launch wrote past m_dev"
        assert bool((b[n:] == SENTINEL).all()), f"{name}: the two-kernel sequence wrote past m_dev"
    assert torch.equal(one[2][:n], c["feat_ref"][:n])
    if n:
        assert not bool((one[0][:n] == SENTINEL).any())  # every row < m_dev was written


def test_fused_trunk_beyond_capacity_writes_nothing(case):
    """m_dev > m_cap (a batch beyond the device-sized forward's capacity):
    neither form writes anything; the host-sized launch runs later."""
    c = case
    m_cap = 256 + 7
    assert c["m"] > m_cap
    for fused in (1, 0):
        for name, a in zip(("sdf", "h2", "feat"), _run(c, fused, c["m"], m_cap)):
            assert bool((a == SENTINEL).all()), (fused, name)


def _engine_runs(paths):
    """The capacity test's sequence (tests/test_gpu_engine.py): a host-sized
    first step, a batch beyond the capacity, a device-sized step, a
    device-sized step far below the capacity."""
    from psvo.engine import MappingEngine
    from psvo.octree import map_states
    w, tree, emb0, dec = _setup()
    rgb, depth = w.rgb.reshape(-1, 3).to(DEV), w.depth.reshape(-1).to(DEV)
    crit = {"rgb_weight": 0.5, "depth_weight": 1.0, "sdf_weight": 5000.0, "fs_weight": 10.0}
    eng = MappingEngine(map_states(tree, emb0.clone().to(DEV), 0.2, device=DEV), dec, 0.2, 0.01, truncation=0.1,
                        max_distance=10.0, criteria=crit, max_depth=10.0)
    eng.set_paths(paths)
    out = []
    for it, n in enumerate([128, 512, 512, 128]):
        poses, dirs = _frames_of(w, n)
        pg = torch.zeros(poses.shape[0], 8, device=DEV)
        loss = eng.step_frames(dirs, n, poses.clone(), torch.zeros_like(poses), torch.zeros_like(poses), [0, 1],
                               1e-3, rgb, depth, seed=900 + it, apply_adam=False, pose_grad=pg, want_loss=True)
        torch.cuda.synchronize()
        out.append((float(loss), list(eng.last_stats), eng.grad_flat.cpu().clone(), pg.cpu().clone()))
    eng.close()
    return out, emb0.shape[0] * 16


def test_engine_fused_trunk_matches_interp_pass():
    """The engine's default schedule (the trunk interpolates) against
    PATH_INTERP_PASS (the separate k_interp_fwd), step by step: the query's
    statistics equal, the loss, the decoder gradients and the pose gradients
    bit for bit (all computed in fixed order), the embedding gradients within
    the capacity test's bound (rtol 1e-4, atol 1e-5 · max: their float
    atomics add in a different order every run).  The PATH_INTERP_PASS
    schedule run twice against itself reproduces its decoder and pose
    gradients bit for bit at these shapes, so exact equality is asked of the
    new schedule too."""
    from psvo.engine import MappingEngine
    ref, n_emb = _engine_runs(MappingEngine.PATH_INTERP_PASS)
    again, _ = _engine_runs(MappingEngine.PATH_INTERP_PASS)
    new, _ = _engine_runs(0)
    assert ref[1][1][4] > 1.25 * ref[0][1][4]  # the second batch is beyond the capacity
    for other, what in ((again, "the pass schedule repeated"), (new, "the fused schedule")):
        for it, ((la, sa, ga, pa), (lb, sb, gb, pb)) in enumerate(zip(ref, other)):
            assert sa[:13] == sb[:13], (what, it)
            assert la == lb, (what, it, la, lb)
            assert torch.equal(ga[n_emb:].view(torch.int32), gb[n_emb:].view(torch.int32)), (what, it, "decoder grads")
            assert torch.equal(pa.view(torch.int32), pb.view(torch.int32)), (what, it, "pose grads")
            torch.testing.assert_close(gb[:n_emb], ga[:n_emb], rtol=1e-4,
                                       atol=1e-5 * float(ga[:n_emb].abs().max()))
