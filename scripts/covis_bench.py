"""Covisibility benchmark: psvo_frames_visible (csrc/covis.hip) against the path
composed from the entry points the query stage already had —
psvo_ray_intersect_sorted_packed on the same rays plus a mark pass over its
hit rows — in one process, the two alternating repetition by repetition.

  python scripts/covis_bench.py [--frames 10] [--reps 5] [--out profiles/covis_bench.json]

room0: the tree bench.py's config B builds (scripts/render_bench.py trains on
it; training moves embeddings, not nodes), --frames synthetic 1200 x 680
depth frames, px_step 1 and 4.  multiroom (config E, 2.7 M nodes): one frame.
Times are device-event spans around the C calls alone (inputs made before);
the composed path's rays are formed beforehand and not charged to it, and its
two parts are reported separately.  The composed path keeps at most 50 leaves
per ray (the reference's cap), so its set is a subset of the fused one; the
JSON records whether they are equal on these frames.  The CPU oracle
(covis_case.visible_ref's arithmetic) is timed on one room0 frame and must
give the fused kernel's words.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "proud-slam_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench as B  # noqa: E402

TRUNCATION, MAX_DISTANCE = 0.1, 10.0


def popcount_rows(bits):
    from psvo import covis as K
    return K.popcount(bits.cpu()).tolist()


class Case:
    """One tree and its frames on the device, with both paths' buffers."""

    def __init__(self, scene, ms, frames, device):
        from psvo import _lib as L
        from psvo import covis as K
        self.L, self.K, self.dev, self.vs = L, K, device, float(scene.voxel_size)
        self.centres = ms["voxel_center_xyz"].detach().contiguous()
        self.structure = ms["voxel_structure"].contiguous()
        self.n = int(self.centres.shape[0])
        self.words = K.words_of(self.n)
        self.packed = K._packed_for(self.centres, self.structure)
        self.depths = [f.depth.to(device, torch.float32).contiguous() for f in frames]
        self.dirs = frames[0].rays_d.to(device, torch.float32).contiguous()
        self.poses = torch.stack([torch.as_tensor(f.get_pose()).detach()[:3].reshape(12) for f in frames]).to(
            device, torch.float32).contiguous()
        self.h, self.w = (int(s) for s in self.depths[0].shape)
        self.ptrs = (ctypes.c_void_p * len(frames))(*[d.data_ptr() for d in self.depths])
        self.bits = torch.empty((len(frames), self.words), dtype=torch.int32, device=device)

    def fused(self, px_step):
        self.L.call("psvo_frames_visible", self.L.stream_of(self.dev), len(self.depths), self.h, self.w, px_step,
                    self.ptrs, self.dirs, self.poses, self.n, self.packed, self.centres, self.structure, self.vs,
                    TRUNCATION, MAX_DISTANCE, self.bits, None)
        return self.bits

    def rays(self, f, px_step):
        """(o, d, bound) of frame f's contributing pixels, the pinned arithmetic in torch on the device."""
        c = self.dirs[::px_step, ::px_step].reshape(-1, 3)
        z = self.depths[f][::px_step, ::px_step].reshape(-1)
        P = self.poses[f].reshape(3, 4)
        d = torch.stack([(c[:, 0] * P[j, 0] + c[:, 1] * P[j, 1]) + c[:, 2] * P[j, 2] for j in range(3)], -1)
        keep = z > 0
        d, z = d[keep].contiguous(), z[keep]
        return P[:, 3][None].expand(d.shape[0], 3).contiguous(), d, (z + TRUNCATION).contiguous()

    def composed_setup(self, px_step):
        self.ray_sets = [self.rays(f, px_step) for f in range(len(self.depths))]
        r = max(o.shape[0] for o, _, _ in self.ray_sets)
        dev = self.dev
        self.hit_idx = torch.empty((r, 50), dtype=torch.int32, device=dev)
        self.hit_t0 = torch.empty((r, 50), dtype=torch.float32, device=dev)
        self.hit_t1 = torch.empty((r, 50), dtype=torch.float32, device=dev)
        self.ray_nv = torch.empty(r, dtype=torch.int32, device=dev)
        self.ray_dsum = torch.empty(r, dtype=torch.float32, device=dev)
        self.stats = torch.zeros(16, dtype=torch.int32, device=dev)
        self.cbits = torch.empty((len(self.depths), self.words), dtype=torch.int32, device=dev)
        self.weights = (1 << torch.arange(32, device=dev, dtype=torch.int64))

    def composed_intersect(self, f):
        o, d, _ = self.ray_sets[f]
        self.stats.zero_()
        self.L.call("psvo_ray_intersect_sorted_packed", self.L.stream_of(self.dev), o.shape[0], o, d, self.packed,
                    self.centres, self.structure, self.vs, MAX_DISTANCE, 0.05, self.hit_idx, self.hit_t0, self.hit_t1,
                    self.ray_nv, self.ray_dsum, self.stats)

    def composed_mark(self, f):
        """The mark pass over the hit rows (rows are already trimmed at max_distance)."""
        r = self.ray_sets[f][0].shape[0]
        idx, t0 = self.hit_idx[:r], self.hit_t0[:r]
        keep = (idx >= 0) & (t0 <= self.ray_sets[f][2][:, None])
        flags = torch.zeros(self.words * 32, dtype=torch.bool, device=self.dev)
        flags[idx[keep].long()] = True
        w = (flags.reshape(self.words, 32).long() * self.weights).sum(1)
        self.cbits[f] = torch.where(w >= (1 << 31), w - (1 << 32), w).to(torch.int32)


def span(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def measure(case, px_step, reps):
    n_f = len(case.depths)
    case.composed_setup(px_step)
    case.fused(px_step)  # warm-up of both paths
    for f in range(n_f):
        case.composed_intersect(f)
        case.composed_mark(f)
    torch.cuda.synchronize()
    fused_bits = case.bits.clone()
    subset = bool(((case.cbits & ~fused_bits) == 0).all().item())
    equal = bool((case.cbits == fused_bits).all().item())
    t_f, t_i, t_m = [], [], []
    for _ in range(reps):  # alternating
        t_f.append(span(lambda: case.fused(px_step)))
        t_i.append(span(lambda: [case.composed_intersect(f) for f in range(n_f)]))
        # the hit rows hold the last frame only: the mark pass is timed on it, once per frame
        t_m.append(span(lambda: [case.composed_mark(n_f - 1) for _ in range(n_f)]))
    med = lambda v: float(np.median(v))  # noqa: E731
    sizes = popcount_rows(fused_bits)
    return {"px_step": px_step, "frames": n_f, "rays": int(sum(o.shape[0] for o, _, _ in case.ray_sets)),
            "fused_ms": med(t_f), "fused_ms_all": [round(x, 4) for x in t_f],
            "composed_intersect_ms": med(t_i), "composed_intersect_ms_all": [round(x, 4) for x in t_i],
            "composed_mark_ms": med(t_m), "composed_mark_ms_all": [round(x, 4) for x in t_m],
            "composed_ms": med([a + b for a, b in zip(t_i, t_m)]),
            "composed_hit_row_bytes_per_ray": 600,
            "composed_set_is_subset_of_fused": subset, "composed_set_equals_fused": equal,
            "V_per_frame": sizes, "V_composed_per_frame": popcount_rows(case.cbits)}, fused_bits


def cpu_oracle(case, f, px_step):
    """The tests' reference on frame f; -> (seconds, u32 words)."""
    from oracle import oracle as O
    o, d, bound = (t.cpu().numpy() for t in case.rays(f, px_step))
    centres, structure = case.centres.cpu().numpy(), case.structure.cpu().numpy()
    t0 = time.perf_counter()
    idx, tin, _, _ = O.svo_intersect_flat(o, d, centres, structure, case.vs, n_max=256)
    assert int((idx != -1).sum(1).max()) < 256
    ok = (idx != -1) & (tin <= bound[:, None]) & ~(tin > np.float32(MAX_DISTANCE))
    v = np.unique(idx[ok]).astype(np.int64)
    words = np.zeros(case.words, np.uint32)
    np.bitwise_or.at(words, v >> 5, np.uint32(1) << (v & 31).astype(np.uint32))
    return time.perf_counter() - t0, words


def build(scene_name, n_frames, device):
    from psvo.synthetic import SyntheticFrame, camera_poses
    args = types.SimpleNamespace(scene=scene_name, width=128)
    scene, tree, ms, emb, dec = B.build_scene(args, device, 0)
    frames = []
    for f, T in enumerate(camera_poses(scene, n_frames, seed=77)):
        fr = SyntheticFrame(scene, T, scale=1.0, seed=7 * f + 1, device=device)
        pose = torch.from_numpy(np.asarray(T, np.float32))
        fr.get_pose = lambda pose=pose: pose
        frames.append(fr)
    return scene, ms, frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-multiroom", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "covis_bench.json"))
    a = ap.parse_args()
    from psvo import _lib as L
    L.lib()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    res = {"truncation": TRUNCATION, "max_distance": MAX_DISTANCE, "reps": a.reps, "cases": {}}
    for name, n_frames in (("room0", a.frames),) + (() if a.skip_multiroom else (("multiroom", 1),)):
        B.log(f"{name}: scene, tree, {n_frames} frames")
        scene, ms, frames = build(name, n_frames, device)
        case = Case(scene, ms, frames, device)
        out = {"n_nodes": case.n, "words": case.words, "set_bytes": case.words * 4, "view": [case.w, case.h], "steps": {}}
        bits = {}
        for px_step in (1, 4):
            B.log(f"{name}: px_step {px_step}")
            out["steps"][str(px_step)], bits[px_step] = measure(case, px_step, a.reps)
        s1, s4 = out["steps"]["1"]["V_per_frame"], out["steps"]["4"]["V_per_frame"]
        out["V_step4_over_step1"] = [round(b / max(a_, 1), 4) for a_, b in zip(s1, s4)]
        k = len(frames)
        ov = torch.empty((k + 1, 2), dtype=torch.int32, device=device)
        matrix = []
        for q in range(k):  # the keyframe-to-keyframe overlap matrix |V_k ∩ V_q| at px_step 4
            L.call("psvo_visibility_overlap", L.stream_of(device), k, case.words, bits[4], bits[4][q].contiguous(), ov)
            matrix.append(ov[:k, 0].cpu().tolist())
        out["overlap_matrix_step4"] = matrix
        t_ov = [span(lambda: L.call("psvo_visibility_overlap", L.stream_of(device), k, case.words, bits[4],
                                    bits[4][0].contiguous(), ov)) for _ in range(a.reps + 1)][1:]
        out["overlap_call_ms"] = float(np.median(t_ov))
        secs, words = cpu_oracle(case, 0, 4)
        same = bool((torch.from_numpy(words.view(np.int32).copy()) == bits[4][0].cpu()).all().item())
        out["cpu_oracle"] = {"frame": 0, "px_step": 4, "seconds": secs, "omp_num_threads": int(os.environ.get("OMP_NUM_THREADS", 0)),
                             "equals_fused_words": same}
        assert same, "the fused kernel's words differ from the CPU oracle's"
        res["cases"][name] = out
        del case, ms, frames
        torch.cuda.empty_cache()
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
