"""psvo_frames_visible / psvo_visibility_overlap (csrc/covis.hip)
and psvo/covis.py on the device against covis_case.py's CPU reference.  The
result is a set and t_in is the oracle's bit for bit: every comparison is
exact, word for word."""
import ctypes

import numpy as np
import pytest
import torch

import covis_case as V
import frame_insert_case as C
from psvo import _lib as L
from psvo import covis as K
from psvo.octree import DeviceOctree, map_states

pytestmark = pytest.mark.gpu
DEV = "cuda"
PSVO_E_INVALID = 1


def device_ms(ms):
    return {k: v.to(DEV).contiguous() for k, v in ms.items()}


def visible(frames, ms, voxel_size, px_step, packed=True, flags=None):
    bits = K.visible_voxels(frames, ms, voxel_size, V.TRUNCATION, V.MAX_DISTANCE, px_step, packed=packed, flags=flags)
    torch.cuda.synchronize()
    return bits.cpu().numpy().view(np.uint32)


def assert_words(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    bad = np.flatnonzero((got != want).reshape(-1))
    assert bad.size == 0, (bad[:8], got.reshape(-1)[bad[:8]], want.reshape(-1)[bad[:8]])


# ---- Case A ---------------------------------------------------------------------
@pytest.mark.parametrize("packed", [True, False], ids=["packed", "arrays"])
@pytest.mark.parametrize("px_step", [1, 3, 4])  # 3 divides neither 170 nor 300
def test_case_a_all_frames_and_one_at_a_time(px_step, packed):
    vs = C.scene().voxel_size
    ms = device_ms(V.case_a_tree())
    want = V.case_a_ref(px_step)
    frames = V.case_a_frames()
    print("|V| per frame", [V.popcount(w) for w in want])
    assert_words(visible(frames, ms, vs, px_step, packed), want)  # one call for the four frames
    for k, f in enumerate(frames):
        assert_words(visible([f], ms, vs, px_step, packed)[0], want[k])
    assert V.A_NODES % 32 != 0 and int(want[:, -1].max()) >> (V.A_NODES & 31) == 0  # the tail bits stay zero


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "arrays"])
def test_case_a_shifted_pose(packed):
    vs = C.scene().voxel_size
    want = V.case_a_ref(4, C.SHIFT)
    assert int(sum(V.popcount(w) for w in want)) > 0  # below zero most rays miss the root box; two frames still see voxels
    assert_words(visible(V.case_a_frames(C.SHIFT), device_ms(V.case_a_tree(C.SHIFT)), vs, 4, packed), want)


def test_zero_nan_and_inf_depth_pixels():
    vs = C.scene().voxel_size
    depth, rays_d, pose = V.case_a_frames()[1]
    depth = depth.clone()
    g = torch.Generator().manual_seed(5)
    pick = torch.randperm(depth.numel(), generator=g)
    flat = depth.view(-1)
    flat[pick[:4000]] = 0.0
    flat[pick[4000:8000]] = float("nan")
    flat[pick[8000:12000]] = float("inf")   # a ray with no depth bound: max_distance alone decides
    flat[pick[12000:13000]] = -1.0
    frame = (depth, rays_d, pose)
    ms_cpu = V.case_a_tree()
    want = V.visible_ref(frame, ms_cpu, vs, px_step=1)
    clean = V.case_a_ref(1)[1]
    assert V.popcount(want & ~clean) > 0  # the unbounded rays see past the walls
    for packed in (True, False):
        assert_words(visible([frame], device_ms(ms_cpu), vs, 1, packed)[0], want)
    none = (torch.full_like(depth, float("nan")), rays_d, pose)
    assert int(visible([none, frame], device_ms(ms_cpu), vs, 1)[0].max()) == 0


def raw_call(frames, ms, vs, px_step, bits, packed=None, flags=None, n_nodes=None, h=None, w=None):
    """psvo_frames_visible itself; returns its code."""
    depths = [f[0].to(DEV, torch.float32).contiguous() for f in frames]
    dirs = frames[0][1].to(DEV, torch.float32).contiguous()
    poses = torch.stack([f[2][:3].reshape(12) for f in frames]).to(DEV, torch.float32).contiguous()
    ptrs = (ctypes.c_void_p * len(depths))(*[d.data_ptr() for d in depths])
    hh, ww = depths[0].shape
    n = ms["voxel_center_xyz"].shape[0] if n_nodes is None else n_nodes
    rc = L.lib().psvo_frames_visible(L.stream_of(DEV), len(depths), hh if h is None else h, ww if w is None else w,
                                     px_step, ptrs, L.ptr(dirs), L.ptr(poses), n, L.ptr(packed),
                                     L.ptr(ms["voxel_center_xyz"]), L.ptr(ms["voxel_structure"]), vs, V.TRUNCATION,
                                     V.MAX_DISTANCE, L.ptr(bits), L.ptr(flags))
    torch.cuda.synchronize()
    return rc


def test_garbage_in_bits_and_repeat_calls():
    vs = C.scene().voxel_size
    ms = device_ms(V.case_a_tree())
    want = V.case_a_ref(4)
    frames = V.case_a_frames()
    bits = torch.full((4, want.shape[1]), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    assert raw_call(frames, ms, vs, 4, bits) == 0
    first = bits.cpu().numpy().view(np.uint32)
    assert_words(first, want)  # the call zeroes the words itself
    bits.fill_(-1)
    assert raw_call(frames, ms, vs, 4, bits) == 0
    assert_words(bits.cpu().numpy().view(np.uint32), first)  # back to back: identical words


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "arrays"])
def test_large_tree_sets_bits_in_global_memory(packed):
    """More than 65,536 nodes: the set no longer fits the workgroup's LDS
    copy.  The tree is Case A's with unreferenced nodes appended (the walk
    never reaches them): the same sets, zero-extended; 70,001 is no multiple
    of 32."""
    vs = C.scene().voxel_size
    ms_cpu = V.case_a_tree()
    n = 70001
    centres = torch.zeros(n, 3)
    structure = torch.full((n, 9), -1, dtype=torch.int32)
    structure[:, 8] = 1
    centres[:V.A_NODES] = ms_cpu["voxel_center_xyz"]
    structure[:V.A_NODES] = ms_cpu["voxel_structure"]
    ms = device_ms({"voxel_center_xyz": centres, "voxel_structure": structure})
    want = np.zeros((4, V.words_of(n)), np.uint32)
    want[:, :V.words_of(V.A_NODES)] = V.case_a_ref(4)
    assert_words(visible(V.case_a_frames(), ms, vs, 4, packed), want)


# ---- Case B ---------------------------------------------------------------------
@pytest.mark.parametrize("packed", [True, False], ids=["packed", "arrays"])
@pytest.mark.parametrize("reverse", [False, True], ids=["near_end", "far_end"])
@pytest.mark.parametrize("depth", sorted(V.B_COUNTS))
def test_case_b_row_has_no_cap(depth, reverse, packed):
    """The row from both ends: whichever order a walk visits children in, one
    of the two rays meets its 46 / 21 voxels last, where a leaf cap cuts."""
    ms_cpu, ids = V.case_b_tree()
    got = visible([V.case_b_frame(depth, reverse)], device_ms(ms_cpu), V.B_VOXEL, 1, packed)[0]
    n = V.B_COUNTS[depth]
    print("row voxels seen", V.popcount(got), "of", n)
    assert V.popcount(got) == n
    assert sorted(V.ids_of(got)) == sorted(ids[V.B_ROW - n:] if reverse else ids[:n])
    assert_words(got, V.case_b_ref(depth, reverse=reverse))


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "arrays"])
def test_case_b_depth_bound_is_inclusive(packed):
    """depth + truncation lands exactly on row voxel 10's t_in: that voxel is seen."""
    ms_cpu, ids = V.case_b_tree()
    depth = V.case_b_tie_depth()
    got = visible([V.case_b_frame(depth)], device_ms(ms_cpu), V.B_VOXEL, 1, packed)[0]
    assert sorted(V.ids_of(got)) == sorted(ids[:V.B_TIE_VOXEL + 1])
    assert_words(got, V.case_b_ref(depth))


# ---- a tree deeper than the level stack ---------------------------------------------
def chain_tree(depth_of_leaf):
    """A chain root → ... → leaf, one child each (slot 0), node i the box [0, side_i]^3."""
    n = depth_of_leaf + 1
    structure = np.full((n, 9), -1, np.int32)
    centres = np.zeros((n, 3), np.float32)
    for i in range(n):
        side = 1 << (depth_of_leaf - i)
        structure[i, 8] = side
        centres[i] = side / 2.0
        if i + 1 < n:
            structure[i, 0] = i + 1
    return {"voxel_center_xyz": torch.from_numpy(centres), "voxel_structure": torch.from_numpy(structure)}


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "arrays"])
def test_tree_deeper_than_the_level_stack_sets_the_flag(packed):
    frame = V.ray_frame((0.25, 0.3, -1.0), (0.001, 0.002, 1.0), 5.0)
    for leaf_depth, flag in ((16, 0), (17, 1)):  # 16 levels of children fit the stack; the 17th does not
        ms_cpu = chain_tree(leaf_depth)
        flags = torch.zeros(1, dtype=torch.int32, device=DEV)
        got = visible([frame], device_ms(ms_cpu), 1.0, 1, packed, flags=flags)[0]
        assert int(flags.item()) == flag
        if flag:
            assert int(got.max()) == 0  # the subtree below the stack is not descended
        else:
            o, d, z = V.frame_rays(*frame, 1)
            want = V.rays_visible_ref(o, d, z, ms_cpu["voxel_center_xyz"].numpy(), ms_cpu["voxel_structure"].numpy(),
                                      1.0, V.TRUNCATION, V.MAX_DISTANCE)[0]
            assert V.ids_of(want).tolist() == [leaf_depth]
            assert_words(got, want)


# ---- overlap counts --------------------------------------------------------------
def np_popcount_rows(a):
    return np.unpackbits(np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], -1), axis=1).sum(1)


def device_overlap(sets, query):
    n_sets, words = sets.shape
    s = torch.from_numpy(sets.view(np.int32).copy()).to(DEV)
    q = torch.from_numpy(query.view(np.int32).copy()).to(DEV)
    out = torch.full((n_sets + 1, 2), -7, dtype=torch.int32, device=DEV)
    L.call("psvo_visibility_overlap", L.stream_of(DEV), n_sets, words, s, q, out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("n_sets", [1, 9])
@pytest.mark.parametrize("words", [1, 63, 233])
def test_overlap_random_words(words, n_sets):
    rng = np.random.default_rng(100 * words + n_sets)
    sets = rng.integers(0, 1 << 32, (n_sets, words), dtype=np.uint64).astype(np.uint32)
    sets[0] &= rng.integers(0, 1 << 32, words, dtype=np.uint64).astype(np.uint32)  # a sparser one
    query = rng.integers(0, 1 << 32, words, dtype=np.uint64).astype(np.uint32)
    out = device_overlap(sets, query)
    assert out[:n_sets, 0].tolist() == np_popcount_rows(sets & query[None]).tolist()
    assert out[:n_sets, 1].tolist() == np_popcount_rows(sets).tolist()
    assert out[n_sets].tolist() == [V.popcount(query)] * 2


def test_overlap_case_a_sets():
    ref = np.array(V.case_a_ref(4))
    for q in range(4):
        out = device_overlap(ref, ref[q])
        assert out[:4, 1].tolist() == list(V.A_SIZES[4])
        assert out[4].tolist() == [V.A_SIZES[4][q]] * 2
        for k in range(4):
            want = V.A_SIZES[4][q] if k == q else V.A_INTER[4].get((min(k, q), max(k, q)), 0)
            assert out[k, 0] == want, (q, k)
    print("overlap matrix", [[int(device_overlap(ref, ref[q])[k, 0]) for k in range(4)] for q in range(4)])


# ---- Covisibility end to end ---------------------------------------------------------
def test_covisibility_on_a_growing_device_tree(monkeypatch):
    sc = C.scene()
    vs = sc.voxel_size
    tree = DeviceOctree(DEV)
    tree.init(sc.grid_dim, 16, vs, 8)
    emb = torch.zeros(1, device=DEV)
    cv = K.Covisibility(vs, V.TRUNCATION, V.MAX_DISTANCE, px_step=4)
    graph = [(d, r, p.clone()) for d, r, p in V.case_a_frames()]  # poses of our own: one is moved below
    counts = []
    for f in graph:  # the mapper's loop: integrate the frame, make it a keyframe
        tree.insert_frame(*f)
        ms = map_states(tree, emb, vs)
        cv.add_keyframe(f, ms)
        counts.append(K.n_nodes_of(ms))
    assert counts[-1] == V.A_NODES and sorted(set(counts)) == counts  # the tree grew with every frame
    final = np.array(V.case_a_ref(4))
    early = cv.bits.cpu().numpy().view(np.uint32)
    assert early.shape == final.shape                       # the early sets are zero-extended ...
    assert int((early & ~final).max()) == 0                 # ... and stay valid subsets of the fresh ones
    assert cv.stale(ms) == [0, 1, 2]                        # computed on smaller trees; the last one is current

    calls = []
    real = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    assert cv.refresh(graph, ms) == [0, 1, 2]
    assert calls.count("psvo_frames_visible") == 1          # the three stale keyframes in one call
    assert_words(cv.bits.cpu().numpy().view(np.uint32), final)
    assert cv.stale(ms) == [] and cv.refresh(None, ms) == []
    assert calls.count("psvo_frames_visible") == 1

    graph[2][2][0, 3] += 0.5                                # keyframe 2's pose moves (in place)
    try:
        assert cv.stale(ms) == [2]
    finally:
        graph[2][2][0, 3] -= 0.5
    assert cv.stale(ms) == []

    # the optimisation window: the keyframes that see what the tracked frame sees
    for q, want in ((0, [0, 2]), (3, [1, 3])):
        tracked = (graph[q][0], graph[q][1], graph[q][2].clone())  # a tracked frame at keyframe q's pose
        calls.clear()
        got = K.select_optimize_targets(graph, 2, tracked, graph[3], covis=cv, method="overlap", map_states=ms)
        assert [k for f in got[:-1] for k, g in enumerate(graph) if g is f] == want and got[-1] is tracked
        assert calls.count("psvo_visibility_overlap") == 1
        inter, size, n_query = cv.overlap(tracked, ms)
        assert size.tolist() == list(V.A_SIZES[4]) and n_query == V.A_SIZES[4][q]
        assert cv.is_new_keyframe(tracked, ms, 0.8, current=q) is False   # it sees what keyframe q sees
        assert cv.is_new_keyframe(tracked, ms, 0.8, current=(q + 1) % 4) is True


# ---- bad arguments -----------------------------------------------------------------
def test_invalid_arguments_launch_nothing():
    vs = C.scene().voxel_size
    ms = device_ms(V.case_a_tree())
    frames = V.case_a_frames()[:1]
    words = V.words_of(V.A_NODES)
    bits = torch.full((1, words), 0x13572468, dtype=torch.int32, device=DEV)
    untouched = lambda: bool((bits == 0x13572468).all().item())
    assert raw_call(frames, ms, vs, 0, bits) == PSVO_E_INVALID and untouched()         # px_step <= 0
    assert raw_call(frames, ms, vs, -4, bits) == PSVO_E_INVALID and untouched()
    assert raw_call(frames, ms, 0.0, 4, bits) == PSVO_E_INVALID and untouched()        # voxel_size <= 0
    assert raw_call(frames, ms, vs, 4, bits, n_nodes=0) == PSVO_E_INVALID and untouched()
    assert raw_call(frames, ms, vs, 4, bits, h=4097, w=4097) == PSVO_E_INVALID and untouched()  # h·w > 2^24
    assert b"2^24" in L.lib().psvo_last_error()
    lib = L.lib()
    null_img = (ctypes.c_void_p * 1)(None)
    d = frames[0][1].to(DEV).contiguous()
    p = torch.zeros(12, device=DEV)
    args = lambda img: (L.stream_of(DEV), 1, 170, 300, 4, img, L.ptr(d), L.ptr(p), V.A_NODES, None,
                        L.ptr(ms["voxel_center_xyz"]), L.ptr(ms["voxel_structure"]), vs, 0.1, 10.0, L.ptr(bits), None)
    assert lib.psvo_frames_visible(*args(null_img)) == PSVO_E_INVALID                    # a null image
    assert lib.psvo_frames_visible(*args(None)) == PSVO_E_INVALID                        # no image array
    torch.cuda.synchronize()
    assert untouched()
    out = torch.zeros((2, 2), dtype=torch.int32, device=DEV)
    assert lib.psvo_visibility_overlap(L.stream_of(DEV), 1, 0, L.ptr(bits), L.ptr(bits), L.ptr(out)) == PSVO_E_INVALID
    assert lib.psvo_visibility_overlap(L.stream_of(DEV), 1, words, L.ptr(bits), None, L.ptr(out)) == PSVO_E_INVALID
    assert lib.psvo_visibility_words(V.A_NODES) == words and lib.psvo_visibility_words(0) == 0
    assert raw_call(frames, ms, vs, 4, bits) == 0 and not untouched()                    # and the good call runs
