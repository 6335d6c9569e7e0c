"""The sparse decoder's backward as ONE launch whose workgroups are divided
between the two sample classes (k_mlp_bwd3<W, H2>: class A, the composited
samples, on workgroups [0, nA); class B, the loss-only samples' trunk, on the
rest; one slab set) against the two launches it replaces
(PATH_BWD_TWO_LAUNCH: k_mlp_bwd3<true>, then k_mlp_trunk_fb, each over the
whole grid with slabs of its own).  The forward is the same kernels, so the
loss and the statistics are the same bits; the weight gradients are the same
sums in another order, the embedding gradients float atomics in any order:
test_sparse_decoder_matches_dense's bounds for a change of summation order
(tests/test_gpu_engine.py), whose engine set-up this is."""
from copy import deepcopy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
CRIT = {"rgb_weight": 0.5, "depth_weight": 1.0, "sdf_weight": 5000.0, "fs_weight": 10.0}


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
def random_case():
    """test_gpu_engine._setup: room0, 2 × 512 rays, a random decoder (its sdf
    negative nearly everywhere).  Shared, left unchanged."""
    from psvo import synthetic as syn
    from psvo.decoder import Decoder
    from psvo.octree import Octree
    w = syn.make_workload("room0", 2, 512, seed=4)
    tree = Octree()
    tree.init(256, 16, 0.2, 8)
    tree.insert(w.voxels)
    emb0 = torch.randn(max(20000, tree.count_nodes()), 16, generator=torch.Generator().manual_seed(0)) * 0.1
    torch.manual_seed(0)
    dec = Decoder(depth=2, width=128, in_dim=16, skips=[], embedder="none").to(DEV)
    return w, tree, emb0, dec


@pytest.fixture(scope="module")
def surface():
    """tests/surface_case.py: the decoder's sdf is the scene's signed distance,
    both classes populated as a trained map has them."""
    import surface_case as S
    from psvo.decoder import Decoder
    w, tree, emb0, params, _ = S.surface_case()
    dec = Decoder(depth=2, width=128, in_dim=16, skips=[], embedder="none").to(DEV)
    dec.load_state_dict(params)
    return w, tree, emb0, dec


def _shifted(dec, shift):
    dec = deepcopy(dec)
    with torch.no_grad():
        dec.sdf_out.bias[0] += shift
    return dec


def _engine(case, dec, paths, step=0.01):
    from psvo.engine import MappingEngine
    from psvo.octree import map_states
    w, tree, emb0, _ = case
    eng = MappingEngine(map_states(tree, emb0.clone().to(DEV), 0.2, device=DEV), dec, 0.2, step, truncation=0.1,
                        max_distance=10.0, criteria=CRIT, max_depth=10.0)
    eng.set_paths(paths)
    return eng


def _step(eng, case, n, seed, gt_depth=None):
    """One psvo_map_step_frames iteration of n rays per frame, stopped before
    Adam: (loss, statistics, gradients, pose gradient, class-A samples,
    class-B samples, workgroups of the decoder backward).  gt_depth: one
    measured depth for every ray in place of the workload's."""
    w = case[0]
    poses, dirs = _frames_of(w, n)
    rgb, depth = w.rgb.reshape(-1, 3).to(DEV), w.depth.reshape(-1).to(DEV)
    if gt_depth is not None:
        depth = torch.full_like(depth, gt_depth)
    pg = torch.zeros(poses.shape[0], 8, device=DEV)
    loss = eng.step_frames(dirs, n, poses.clone(), torch.zeros_like(poses), torch.zeros_like(poses), [0, 1], 1e-3,
                           rgb, depth, seed=seed, apply_adam=False, pose_grad=pg, want_loss=True)
    torch.cuda.synchronize()
    sel = eng.select_stats()
    stats = list(eng.last_stats)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    grid = max(1, min((stats[4] + 63) // 64, cus))  # mlp_bwd.hip bwd3_grid: one workgroup per round of 64 samples
    return dict(loss=float(loss), stats=stats, grads=eng.grad_flat.cpu().clone(), pose=pg.cpu().clone(),
                m_a=sel["composited"], m_b=sel["kept"] - sel["composited"], grid=grid)


def _runs(case, dec, paths, n, seeds=(700, 701), step=0.01, gt_depth=None):
    eng = _engine(case, dec, paths, step)
    out = [_step(eng, case, n, s, gt_depth) for s in seeds]
    eng.close()
    return out


def _n_a(r):
    from psvo import _lib as L
    return L.lib().psvo_debug_bwd_split((r["m_a"] + 15) // 16, (r["m_b"] + 15) // 16, r["grid"])


def _assert_same(new, ref, n_emb, what):
    """test_sparse_decoder_matches_dense's comparison."""
    assert new["stats"][:13] == ref["stats"][:13], what
    assert new["loss"] == ref["loss"], (what, new["loss"], ref["loss"])
    assert (new["m_a"], new["m_b"]) == (ref["m_a"], ref["m_b"]), what
    gd, gs = ref["grads"][n_emb:], new["grads"][n_emb:]
    ed, es = ref["grads"][:n_emb], new["grads"][:n_emb]
    print(f"{what}: M {new['stats'][4]} A {new['m_a']} B {new['m_b']} G {new['grid']} nA {_n_a(new)} "
          f"dec max|g| {float(gd.abs().max()):.4g} max|diff| {float((gs - gd).abs().max()):.4g} "
          f"emb max|g| {float(ed.abs().max()):.4g} max|diff| {float((es - ed).abs().max()):.4g}")
    torch.testing.assert_close(gs, gd, rtol=1e-4, atol=1e-5 * float(gd.abs().max()))
    torch.testing.assert_close(es, ed, rtol=1e-4, atol=1e-5 * float(ed.abs().max()))
    torch.testing.assert_close(new["pose"], ref["pose"], rtol=0, atol=1e-4 * float(ref["pose"].abs().max()))


def _compare(case, dec, n, step=0.01, gt_depth=None):
    from psvo.engine import MappingEngine
    n_emb = case[2].shape[0] * 16
    ref = _runs(case, dec, MappingEngine.PATH_BWD_TWO_LAUNCH, n, step=step, gt_depth=gt_depth)
    new = _runs(case, dec, 0, n, step=step, gt_depth=gt_depth)
    for it, (a, b) in enumerate(zip(new, ref)):
        _assert_same(a, b, n_emb, f"n {n} step {step} iteration {it}")
    return new


def test_one_launch_matches_two_both_classes(surface):
    """Both classes populated (the surface case, 256 rays per frame): the
    split is strictly inside the grid."""
    for r in _compare(surface, surface[3], 256):
        assert r["m_a"] > 0 and r["m_b"] > 0 and r["grid"] >= 10
        assert 1 <= _n_a(r) < r["grid"]


def test_one_launch_matches_two_class_b_nearly_empty(random_case):
    """The random decoder (sdf_shift 0): its sdf is negative nearly everywhere,
    the first sign change at the padding and nearly every sample composited —
    153 of 55 k kept samples are class B's, which gets the one workgroup a
    present class must have.  (No batch of this set-up leaves class B exactly
    empty: a constant measured depth in front of every ray still keeps 4
    loss-only samples.  nA = G is tests/test_bwd_split.py's.)"""
    for r in _compare(random_case, random_case[3], 512):
        assert 0 < r["m_b"] < 0.01 * r["m_a"]
        assert _n_a(r) == r["grid"] - 1


def test_one_launch_matches_two_class_a_small(random_case):
    """The decoder's sdf shifted positive: no sign change, z_min is the first
    sample, most samples dropped and few composited."""
    for r in _compare(random_case, _shifted(random_case[3], 0.5), 512):
        assert 0 < r["m_a"] < r["m_b"]
        assert 1 <= _n_a(r) < r["grid"]


@pytest.mark.parametrize("n,step", [(2, 0.01), (4, 0.01), (2, 0.1)])
def test_one_launch_matches_two_tiny_batch(surface, n, step):
    """A few rays per frame.  Sampler step 0.01 (141 and 267 samples: 3 and 5
    workgroups): some workgroups get fewer than four units (a partial first
    round, idle chain waves).  (2, 0.1): 22 samples, one workgroup — no split,
    the two launches run (the fallback) and the switch changes nothing: the
    decoder gradients are then the same bits."""
    new = _compare(surface, surface[3], n, step)
    for r in new:
        assert r["m_a"] > 0 and r["m_b"] > 0
        if step == 0.1:
            assert r["grid"] == 1
        else:
            assert 2 <= r["grid"] < 10
            units = ((r["m_a"] + 15) // 16, (r["m_b"] + 15) // 16)
            n_a = _n_a(r)
            assert min(units[0] // n_a, units[1] // (r["grid"] - n_a)) < 4
    if step == 0.1:
        from psvo.engine import MappingEngine
        n_emb = surface[2].shape[0] * 16
        ref = _runs(surface, surface[3], MappingEngine.PATH_BWD_TWO_LAUNCH, n, step=step)
        for a, b in zip(new, ref):
            assert torch.equal(a["grads"][n_emb:].view(torch.int32), b["grads"][n_emb:].view(torch.int32))


def test_stale_slab_elements_are_not_read(random_case):
    """Two consecutive steps on one engine whose class mixes differ: the
    random decoder (nearly every sample composited: all workgroups but the
    last class A's, every element of their slabs written), then shifted
    positive (class A small: most slabs are class B's now and keep the first
    step's values in the elements class B does not write).
    The second step's gradients against a fresh engine's given only that
    step."""
    n_emb = random_case[2].shape[0] * 16
    dec = deepcopy(random_case[3])
    eng = _engine(random_case, dec, 0)
    first = _step(eng, random_case, 512, 700)
    with torch.no_grad():
        dec.sdf_out.bias[0] += 0.5  # the engine reads the live parameters
    second = _step(eng, random_case, 512, 701)
    eng.close()
    fresh_eng = _engine(random_case, _shifted(random_case[3], 0.5), 0)
    fresh = _step(fresh_eng, random_case, 512, 701)
    fresh_eng.close()
    assert _n_a(first) >= first["grid"] - 1
    assert second["grid"] == first["grid"]
    assert _n_a(first) - _n_a(second) >= first["grid"] / 4, (_n_a(first), _n_a(second))
    _assert_same(second, fresh, n_emb, "second step against a fresh engine")


def test_one_launch_is_deterministic(surface):
    """The same step twice from the same state: the decoder gradients are the
    same bits (slabs in fixed order, quarters in order)."""
    n_emb = surface[2].shape[0] * 16
    a = _runs(surface, surface[3], 0, 256)
    b = _runs(surface, surface[3], 0, 256)
    for x, y in zip(a, b):
        assert x["loss"] == y["loss"]
        assert torch.equal(x["grads"][n_emb:].view(torch.int32), y["grads"][n_emb:].view(torch.int32))
