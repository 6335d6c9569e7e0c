"""Covisibility without a GPU: the reference of the device tests reproduces the
hand-derived counts (covis_case.py), and the policy layer of psvo/covis.py —
window selection, the overlap_th keyframe rule, staleness — on hand-made CPU
bitsets.  Every comparison is exact."""
import random

import numpy as np
import pytest
import torch

import covis_case as V
from psvo import covis as K


# ---- the reference ------------------------------------------------------------
@pytest.mark.parametrize("depth", sorted(V.B_COUNTS))
def test_reference_case_b(depth):
    ms, ids = V.case_b_tree()
    words = V.case_b_ref(depth)
    n = V.B_COUNTS[depth]
    assert V.popcount(words) == n
    assert sorted(V.ids_of(words)) == sorted(ids[:n])  # exactly the n nearest voxels of the row
    # the reference's 50-leaf cap keeps the farthest 50 of the row: the near ones are lost
    capped = V.case_b_ref(depth, n_max=50)
    assert V.popcount(capped) == V.B_CAPPED[depth]
    assert set(V.ids_of(capped)) <= set(ids[30:])


@pytest.mark.parametrize("depth", sorted(V.B_COUNTS))
def test_reference_case_b_from_the_far_end(depth):
    ms, ids = V.case_b_tree()
    words = V.case_b_ref(depth, reverse=True)
    n = V.B_COUNTS[depth]
    assert sorted(V.ids_of(words)) == sorted(ids[V.B_ROW - n:])  # the n voxels nearest to the far end


def test_reference_case_b_exact_tie():
    ms, ids = V.case_b_tree()
    words = V.case_b_ref(V.case_b_tie_depth())
    assert sorted(V.ids_of(words)) == sorted(ids[:V.B_TIE_VOXEL + 1])  # the voxel on the bound is in: t_in <= bound
    below = V.case_b_ref(float(np.nextafter(np.float32(V.case_b_tie_depth()), np.float32(0))))
    assert sorted(V.ids_of(below)) == sorted(ids[:V.B_TIE_VOXEL])      # one ulp less depth: out


@pytest.mark.parametrize("px_step", sorted(V.A_SIZES))
def test_reference_case_a(px_step):
    assert V.case_a_tree()["voxel_center_xyz"].shape[0] == V.A_NODES
    ref = V.case_a_ref(px_step)
    assert ref.shape == (4, V.words_of(V.A_NODES))
    assert tuple(V.popcount(r) for r in ref) == V.A_SIZES[px_step]
    for i in range(4):
        for j in range(i + 1, 4):
            assert V.popcount(ref[i] & ref[j]) == V.A_INTER[px_step].get((i, j), 0), (i, j)
    assert int(ref[:, -1].max()) >> (V.A_NODES & 31) == 0  # no bit at or beyond n_nodes


def test_reference_case_a_hits_per_ray():
    ms = V.case_a_tree()
    most = 0
    for frame in V.case_a_frames():
        o, d, z = V.frame_rays(*frame, 1)
        most = max(most, V.rays_visible_ref(o, d, z, ms["voxel_center_xyz"].numpy(), ms["voxel_structure"].numpy(),
                                            V.C.scene().voxel_size, V.TRUNCATION, V.MAX_DISTANCE)[1])
    assert most == V.A_MAX_HITS


# ---- hand-made sets -------------------------------------------------------------
def bits_of(ids, words=3):
    w = np.zeros(words, np.uint32)
    for v in ids:
        w[v >> 5] |= np.uint32(1) << np.uint32(v & 31)
    return torch.from_numpy(w.view(np.int32).copy())


class Frame:
    def __init__(self, name, pose=None):
        self.name = name
        self.pose = torch.eye(4) if pose is None else pose
        self.depth = self.rays_d = None

    def get_pose(self):
        return self.pose


def tree_of(n_nodes):
    return {"voxel_center_xyz": torch.zeros(n_nodes, 3), "voxel_structure": torch.zeros(n_nodes, 9, dtype=torch.int32)}


def graph_of(id_lists, n_nodes=90):
    cv = K.Covisibility(0.2, 0.1, 10.0)
    graph = [Frame(f"kf{k}") for k in range(len(id_lists))]
    for f, ids in zip(graph, id_lists):
        cv.add_keyframe(f, tree_of(n_nodes), bits=bits_of(ids))
    return cv, graph


def test_popcount_and_extend():
    t = bits_of([0, 31, 32, 70, 89])
    assert int(K.popcount(t)) == 5
    assert K.popcount(torch.stack([t, bits_of([]), bits_of(range(96))])).tolist() == [5, 0, 96]
    e = K.extend_words(t, 5)
    assert e.shape == (5,) and torch.equal(e[:3], t) and int(e[3:].abs().sum()) == 0
    assert K.words_of(7427) == 233 and K.words_of(64) == 2 and K.words_of(65) == 3


def test_overlap_counts_cpu():
    cv, _ = graph_of([[1, 2, 3, 40], [40, 41, 80], []])
    inter, size, n_query = cv.overlap(bits_of([2, 3, 40, 80, 81]))
    assert inter.tolist() == [3, 2, 0] and size.tolist() == [4, 3, 0] and n_query == 5
    inter, size, n_query = cv.overlap(bits_of([2, 40, 100], words=4))  # a query on a grown tree
    assert inter.tolist() == [2, 1, 0] and n_query == 3


def reference_random(graph, window, tracked, current):
    """mapping.py:220-234 as the reference runs it (selection_method = 'random')."""
    if len(graph) <= window:
        targets = graph[:]
    else:
        targets = random.sample(graph, window)
    if tracked is not None and tracked != current:
        targets += [tracked]
    return targets


@pytest.mark.parametrize("n,window", [(3, 4), (4, 4), (9, 4), (20, 5)])
def test_select_random_is_the_reference(n, window):
    graph = [Frame(f"kf{k}") for k in range(n)]
    tracked = Frame("tracked")
    for tr, cur in ((tracked, graph[-1]), (None, graph[-1]), (graph[-1], graph[-1])):
        random.seed(1234)
        want = reference_random(graph, window, tr, cur)
        random.seed(1234)
        got = K.select_optimize_targets(graph, window, tr, cur)
        assert [f.name for f in got] == [f.name for f in want]
        assert len(graph) == n  # the graph itself is not extended


def test_select_overlap_top_k_in_graph_order():
    cv, graph = graph_of([[1], [1, 2, 3], [9], [1, 2], [1, 2, 3, 4], [50]])
    tracked = Frame("tracked")
    cv_q = bits_of([1, 2, 3, 4, 5])
    state = random.getstate()
    # the query's set: through a stored keyframe (current) ...
    got = K.select_optimize_targets(graph, 3, None, graph[4], covis=cv, method="overlap")
    assert [f.name for f in got] == ["kf1", "kf3", "kf4"]  # 3, 2, 4 common voxels, ascending graph order
    # ... or through the tracked frame's own set
    inter, _, _ = cv.overlap(cv_q)
    assert inter.tolist() == [1, 3, 0, 2, 4, 0]
    assert random.getstate() == state  # no random numbers drawn


def test_select_overlap_tracked_frame_is_the_query_and_is_appended(monkeypatch):
    cv, graph = graph_of([[1, 2], [7, 8, 9], [7], [1]])
    tracked = Frame("tracked")
    monkeypatch.setattr(cv, "_visible", lambda frames, ms: bits_of([7, 8, 1]).reshape(1, -1))
    got = K.select_optimize_targets(graph, 2, tracked, graph[0], covis=cv, method="overlap", map_states=tree_of(90))
    assert [f.name for f in got] == ["kf1", "kf3", "tracked"]  # inter 1, 2, 1, 1: the tie goes to the higher index
    got = K.select_optimize_targets(graph, 2, graph[0], graph[0], covis=cv, method="overlap")
    assert [f.name for f in got] == ["kf0", "kf3"]  # the current keyframe as tracked frame: not appended


def test_select_overlap_ties_and_empty_intersections():
    # inter = [2, 0, 2, 0, 2, 0]: ties go to the higher index, empty ones fill up last (highest index first)
    cv, graph = graph_of([[1, 2], [60], [1, 2, 9], [61], [1, 2, 70], [62]])
    q = Frame("q")
    cv.add_keyframe(q, tree_of(90), bits=bits_of([1, 2]))
    graph.append(q)  # the query is the current keyframe, itself in the graph: inter 2
    names = lambda w: [f.name for f in K.select_optimize_targets(graph, w, None, q, covis=cv, method="overlap")]
    assert names(2) == ["kf4", "q"]
    assert names(3) == ["kf2", "kf4", "q"]
    assert names(4) == ["kf0", "kf2", "kf4", "q"]
    assert names(5) == ["kf0", "kf2", "kf4", "kf5", "q"]
    assert names(6) == ["kf0", "kf2", "kf3", "kf4", "kf5", "q"]


def test_select_overlap_graph_no_longer_than_the_window():
    cv, graph = graph_of([[1], [2], [3]])
    tracked = Frame("tracked")
    got = K.select_optimize_targets(graph, 3, tracked, graph[2], covis=None, method="overlap")  # no sets needed
    assert [f.name for f in got] == ["kf0", "kf1", "kf2", "tracked"]
    assert len(graph) == 3
    with pytest.raises(NotImplementedError):
        K.select_optimize_targets(graph, 2, tracked, graph[2], method="nearest")
    with pytest.raises(RuntimeError):
        K.select_optimize_targets(graph, 2, tracked, graph[2], covis=None, method="overlap")


def test_is_new_keyframe_threshold_and_empty_query():
    cv, _ = graph_of([[50], list(range(10))])  # current = the last keyframe: voxels 0..9
    q = bits_of(list(range(8)) + [20, 21])      # 8 of its 10 voxels are the current keyframe's
    assert cv.is_new_keyframe(q, None, 0.81) is True     # 0.8 < 0.81
    assert cv.is_new_keyframe(q, None, 0.8) is False     # 0.8 < 0.8 fails
    assert cv.is_new_keyframe(q, None, 0.79) is False
    assert cv.is_new_keyframe(q, None, 0.5, current=0) is True   # nothing in common with keyframe 0
    assert cv.is_new_keyframe(bits_of([]), None, 0.8) is False   # a frame that sees nothing is no keyframe
    empty = K.Covisibility(0.2, 0.1, 10.0)
    assert empty.is_new_keyframe(q, None, 0.8) is True           # the first frame that sees something


def test_stale_after_pose_and_node_count_changes():
    cv, graph = graph_of([[1], [2], [3]], n_nodes=90)
    assert cv.stale() == [] and cv.stale(tree_of(90)) == []
    graph[1].pose[0, 3] += 0.25                 # in place: the optimiser's update
    assert cv.stale() == [1]
    graph[2].pose = graph[2].pose.clone()       # another tensor, the same bytes: not stale
    assert cv.stale() == [1]
    graph[1].pose[0, 3] -= 0.25
    assert cv.stale() == []
    assert cv.stale(tree_of(91)) == [0, 1, 2]   # the tree grew: every set may miss new voxels
    late = Frame("late")
    cv.add_keyframe(late, tree_of(91), bits=bits_of([4]))
    assert cv.stale() == [0, 1, 2] and cv.stale(tree_of(90)) == [3]
    assert cv.bits.shape == (4, 3)
