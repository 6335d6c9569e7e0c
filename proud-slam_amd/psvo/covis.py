"""Keyframe covisibility (csrc/covis.hip): the set of leaf voxels
each depth frame sees, as a bitset over node ids, and what the mapper's
keyframe policy needs from such sets — overlap counts, the `overlap_th`
keyframe test the reference ships a config value for but never reads
(mapping.py:52, :136) and the `'overlap'` branch of select_optimize_targets
it leaves unimplemented (mapping.py:220-234).

The sets are computed on the GPU (psvo_frames_visible: no CPU or torch
fallback).  Everything after them — overlap counts, staleness, the two
policies — also takes sets held in CPU tensors through torch bit operations,
so the policy layer runs and is tested without a device.
"""
from __future__ import annotations

import ctypes
import random
import weakref

import torch

from . import _lib as L
from .octree import _frame_shapes, _pose34

__all__ = ["visible_voxels", "Covisibility", "select_optimize_targets", "popcount", "extend_words", "words_of"]


def words_of(n_nodes):
    """u32 words of a set over n_nodes node ids (psvo_visibility_words)."""
    return (int(n_nodes) + 31) // 32 if n_nodes > 0 else 0


def _frame_parts(frame):
    """(depth [H, W], rays_d [H, W, 3], pose) of a triple or an RGBDFrame-like object."""
    if isinstance(frame, (tuple, list)):
        depth, rays_d, pose = frame
        return depth, rays_d, pose
    return frame.depth, frame.rays_d, frame.get_pose()


def _tree_arrays(map_states):
    """(centres f32[N,3], structure i32[N,9], packed records or None) of a
    map_states dict (its optional "voxel_packed": the caller's psvo_pack_tree
    records) or of an object that holds them as .centres / .structure /
    .packed (MapEngine, the frame renderer)."""
    if isinstance(map_states, dict):
        return map_states["voxel_center_xyz"], map_states["voxel_structure"], map_states.get("voxel_packed")
    return map_states.centres, map_states.structure, getattr(map_states, "packed", None)


def n_nodes_of(map_states):
    return int(_tree_arrays(map_states)[0].shape[0])


def _packed_for(centres, structure):
    """psvo_pack_tree records of these arrays, packed once per identity: the
    records ride on the centres tensor itself (an attribute), with the versions
    of both arrays and a weak reference to the structure tensor, so they are
    reused while the caller hands over the same unwritten tensors (a
    DeviceOctree's map_states does, while its generation is unchanged) and are
    freed with the array — nothing here keeps a map alive.  A caller whose
    map_states are fresh tensors every time passes its own "voxel_packed"."""
    hit = getattr(centres, "_psvo_packed", None)
    if hit is not None and hit[0]() is structure and hit[1] == (centres._version, structure._version):
        return hit[2]
    n = centres.shape[0]
    packed = torch.empty(n * 32, dtype=torch.uint8, device=centres.device)
    ws = torch.empty(int(L.lib().psvo_pack_tree_workspace_ints(n)), dtype=torch.int32, device=centres.device)
    L.call("psvo_pack_tree", L.stream_of(centres.device), n, centres, structure, ws, packed)
    centres._psvo_packed = (weakref.ref(structure), (centres._version, structure._version), packed)
    return packed


def visible_voxels(frames, map_states, voxel_size, truncation, max_distance, px_step=4, packed=True, flags=None):
    """The visible sets of `frames` on the tree of `map_states`: int32
    [F, words] on the tree's device (bit v & 31 of word v >> 5 = node v), all
    frames in ONE psvo_frames_visible call.  frames: (depth, rays_d, pose)
    triples or objects with .depth, .rays_d and .get_pose(), all of one image
    size; rays_d is the camera's per-pixel direction table and is taken from
    the first frame.  packed=False walks the reference arrays instead of the
    packed records (the same sets).  flags: an int32 device tensor of one
    word that receives the DFS-overflow bit, or None."""
    frames = list(frames)
    centres, structure, pk = _tree_arrays(map_states)
    if not centres.is_cuda:
        raise L.PsvoError("visible_voxels runs on the GPU: map_states must hold device tensors")
    dev = centres.device
    L.require_device_tensor(centres, "voxel_center_xyz", torch.float32)
    L.require_device_tensor(structure, "voxel_structure", torch.int32)
    n = int(centres.shape[0])
    words = words_of(n)
    bits = torch.empty((len(frames), words), dtype=torch.int32, device=dev)
    if not frames:
        return bits
    parts = [_frame_parts(f) for f in frames]
    h, w = (int(s) for s in parts[0][0].shape)
    for depth, rays_d, _ in parts:
        _frame_shapes(depth, rays_d)
        if tuple(depth.shape) != (h, w):
            raise RuntimeError(f"frames of one call share one image size (got {tuple(depth.shape)} and {(h, w)})")
    depths = [d.to(device=dev, dtype=torch.float32).contiguous() for d, _, _ in parts]
    dirs = parts[0][1].to(device=dev, dtype=torch.float32).contiguous()
    poses = torch.stack([_pose34(p).detach().to(dev).contiguous().reshape(12) for _, _, p in parts]).contiguous()
    if not packed:
        pk = None
    elif pk is None:
        pk = _packed_for(centres, structure)
    ptrs = (ctypes.c_void_p * len(depths))(*[d.data_ptr() for d in depths])
    L.call("psvo_frames_visible", L.stream_of(dev), len(depths), h, w, int(px_step), ptrs, dirs, poses, n, pk, centres,
           structure, float(voxel_size), float(truncation), float(max_distance), bits, flags)
    return bits


# ---- sets as tensors: CPU (torch bit operations) or device -----------------
_POP8 = torch.tensor([bin(i).count("1") for i in range(256)], dtype=torch.int64)


def popcount(t):
    """Set bits per row of an int32 [..., words] CPU tensor."""
    t = t.contiguous()
    return _POP8[t.view(torch.uint8).reshape(*t.shape, 4).long()].sum((-1, -2))


def extend_words(t, words):
    """`t` [..., w] zero-extended to [..., words]: a set computed on a smaller
    tree, valid on the grown one (node ids are never renumbered)."""
    if t.shape[-1] == words:
        return t
    if t.shape[-1] > words:
        raise RuntimeError(f"a set of {t.shape[-1]} words does not fit a tree of {words}")
    out = torch.zeros((*t.shape[:-1], words), dtype=t.dtype, device=t.device)
    out[..., :t.shape[-1]] = t
    return out


def _poses_bytes(frames):
    """The 48 bytes of each frame's pose34, all poses in ONE host copy (device
    poses are stacked on their device first: one synchronisation, not one per
    keyframe)."""
    poses = [_pose34(_frame_parts(f)[2]).detach() for f in frames]
    if not poses:
        return []
    dev = next((p.device for p in poses if p.is_cuda), poses[0].device)
    rows = torch.stack([p.to(dev).contiguous().reshape(12) for p in poses]).cpu().numpy()
    return [r.tobytes() for r in rows]


class Covisibility:
    """The keyframes' visible sets, kept current as poses are optimised and
    the map grows.  With each set go the node count and the pose's bytes at
    the time it was computed; a set whose keyframe has another pose now, or
    whose tree has grown since, is stale (a grown tree can put new voxels in
    view; until refreshed the old set stays a valid subset, zero-extended)."""

    def __init__(self, voxel_size, truncation, max_distance, px_step=4):
        self.voxel_size, self.truncation, self.max_distance = float(voxel_size), float(truncation), float(max_distance)
        self.px_step = int(px_step)
        self.frames = []   # the keyframes, in graph order
        self.bits = None   # int32 [K, words]
        self.meta = []     # per keyframe: (node count, pose bytes) of its set
        self._n_nodes = 0  # of the map seen last

    def __len__(self):
        return len(self.frames)

    def _visible(self, frames, map_states):
        return visible_voxels(frames, map_states, self.voxel_size, self.truncation, self.max_distance, self.px_step)

    def _grow(self, words):
        if self.bits is not None and self.bits.shape[1] < words:
            self.bits = extend_words(self.bits, words)

    def add_keyframe(self, frame, map_states, bits=None):
        """Store `frame`'s set on the current tree (computed here, or `bits`:
        the set already computed for it, e.g. by the keyframe test).  Returns
        the keyframe's index."""
        n = n_nodes_of(map_states)
        if bits is None:
            bits = self._visible([frame], map_states)[0]
        bits = bits.reshape(1, -1)
        words = max(words_of(n), bits.shape[1], 0 if self.bits is None else self.bits.shape[1])
        self._grow(words)
        bits = extend_words(bits, words)
        self.bits = bits.clone() if self.bits is None else torch.cat([self.bits, bits.to(self.bits.device)])
        self.frames.append(frame)
        self.meta.append((n, _poses_bytes([frame])[0]))
        self._n_nodes = n
        return len(self.frames) - 1

    def _stale(self, n):
        now = _poses_bytes(self.frames)  # one host copy for all keyframes
        return [k for k, ((nk, pb), cur) in enumerate(zip(self.meta, now)) if nk != n or pb != cur], now

    def stale(self, map_states=None):
        """Indices of the keyframes whose pose bytes or node count differ from now."""
        return self._stale(self._n_nodes if map_states is None else n_nodes_of(map_states))[0]

    def refresh(self, frames, map_states):
        """Recompute exactly the stale keyframes' sets, all in one
        psvo_frames_visible call, and zero-extend the others to the current
        tree.  frames: the keyframes in graph order (they replace the stored
        references), or None: the stored ones.  Returns the refreshed indices."""
        if frames is not None:
            frames = list(frames)
            if len(frames) != len(self.frames):
                raise RuntimeError(f"refresh: {len(frames)} frames for {len(self.frames)} keyframes")
            self.frames = frames
        n = n_nodes_of(map_states)
        self._n_nodes = n
        todo, now = self._stale(n)
        self._grow(words_of(n))
        if todo:
            fresh = self._visible([self.frames[k] for k in todo], map_states)
            self.bits[torch.as_tensor(todo, device=self.bits.device)] = fresh.to(self.bits.device)
            for k in todo:
                self.meta[k] = (n, now[k])
        return todo

    def overlap(self, frame_or_bits, map_states=None):
        """(inter i64[K], size i64[K], n_query): |V_k ∩ V_q|, |V_k| of every
        keyframe and |V_q|, from one psvo_visibility_overlap call (sets on the
        CPU: torch bit operations).  The query is a frame (its set is computed
        on map_states' tree) or a set."""
        if isinstance(frame_or_bits, torch.Tensor):
            q = frame_or_bits.reshape(-1)
        else:
            q = self._visible([frame_or_bits], map_states)[0]
        k = len(self.frames)
        words = max(q.shape[0], 0 if self.bits is None else self.bits.shape[1])
        self._grow(words)
        q = extend_words(q, words)
        sets = self.bits if self.bits is not None else torch.zeros((0, words), dtype=torch.int32, device=q.device)
        if not q.is_cuda:
            sets = sets.cpu()
            return popcount(sets & q[None]).reshape(k), popcount(sets).reshape(k), int(popcount(q))
        sets = sets.to(q.device).contiguous()
        out = torch.empty((k + 1, 2), dtype=torch.int32, device=q.device)
        L.call("psvo_visibility_overlap", L.stream_of(q.device), k, words, sets if k else None, q.contiguous(), out)
        out = out.cpu().long()
        return out[:k, 0], out[:k, 1], int(out[k, 0])

    def is_new_keyframe(self, frame_or_bits, map_states, overlap_th, current=-1):
        """The `overlap_th` keyframe rule: the frame sees something, and less
        than overlap_th of it is what keyframe `current` sees."""
        inter, _, n_query = self.overlap(frame_or_bits, map_states)
        if n_query <= 0:
            return False
        if not len(self.frames):
            return True
        return int(inter[current]) / n_query < overlap_th


def select_optimize_targets(keyframe_graph, window_size, tracked_frame=None, current_keyframe=None, covis=None,
                            method="random", map_states=None):
    """Mapping.select_optimize_targets (mapping.py:220-234) with its
    'overlap' branch filled in.  'random' is the reference's rule: the whole
    graph while it fits the window, else random.sample of it.  'overlap'
    (covis: the Covisibility holding the graph's sets, in graph order): the
    window_size keyframes with the largest |V_k ∩ V_q|, q = tracked_frame if
    given else current_keyframe, in ascending graph order; ties go to the
    higher index, keyframes with an empty intersection fill up only after all
    others (by that order they do anyway).  No random numbers are drawn.
    map_states (beyond the reference's arguments): the tree on which a tracked
    frame that is no keyframe gets its set; a keyframe as query uses its stored set.
    Either way tracked_frame, if given and not the current keyframe, is
    appended."""
    if len(keyframe_graph) <= window_size:
        targets = keyframe_graph[:]
    elif method == "random":
        targets = random.sample(keyframe_graph, window_size)
    elif method == "overlap":
        if covis is None or len(covis) != len(keyframe_graph):
            raise RuntimeError("select_optimize_targets('overlap') needs the graph's Covisibility (one set per keyframe)")
        query = tracked_frame if tracked_frame is not None else current_keyframe
        if query is None:
            raise RuntimeError("select_optimize_targets('overlap') needs a tracked frame or the current keyframe")
        for k, f in enumerate(covis.frames):  # a keyframe as the query: its stored set
            if f is query:
                query = covis.bits[k]
                break
        inter, _, _ = covis.overlap(query, map_states)
        inter = [int(v) for v in inter]
        order = sorted(range(len(inter)), key=lambda k: (inter[k], k), reverse=True)
        targets = [keyframe_graph[k] for k in sorted(order[:window_size])]
    else:
        raise NotImplementedError(f"selection method {method} unknown")
    if tracked_frame is not None and tracked_frame is not current_keyframe:
        targets += [tracked_frame]
    return targets
