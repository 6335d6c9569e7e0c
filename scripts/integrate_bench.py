"""Integrating depth frames into the device octree, two ways, on a fresh tree:

(a) what a caller did before insert_frame — mask, multiply, `@`, torch.div and
    .int() in torch (frame.py:69-71, mapping.py:263-264), DeviceOctree.insert
    of every point, then render_arrays;
(b) DeviceOctree.insert_frame plus map_states.

Frames: SyntheticFrame(room0, scale=1.0) from camera_poses.  One repeat is the
whole sequence on a rebuilt tree, every frame timed on the host between device
synchronisations; the legs alternate.  Reported per leg: the median over the
repeats of the first frame's milliseconds and of the later frames' mean, the
spread of the repeats, and the device-memory high-water mark (a pass of its
own; torch.cuda.mem_get_info deltas, sampled after every frame while the tree
and torch's cached blocks are alive — the library allocates with hipMalloc).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "proud-slam_amd"))
from psvo import synthetic as syn  # noqa: E402
from psvo.octree import DeviceOctree, map_states  # noqa: E402

DEV = "cuda"


def leg_a(tree, frame, pose, vs, emb):
    vmap = frame.rays_d * frame.depth[..., None]
    points = vmap[frame.depth > 0].reshape(-1, 3)
    points = points @ pose[:3, :3].transpose(-1, -2) + pose[:3, 3]
    voxels = torch.div(points, vs, rounding_mode="floor")
    tree.insert(voxels.int())
    return tree.render_arrays(vs)


def leg_b(tree, frame, pose, vs, emb):
    tree.insert_frame(frame.depth, frame.rays_d, pose)
    return map_states(tree, emb, vs)


def run_sequence(leg, scene, frames, poses, emb, after_frame=None):
    """Per-frame milliseconds of one pass over the frames on a fresh tree."""
    tree = DeviceOctree(DEV)
    tree.init(scene.grid_dim, 16, scene.voxel_size, 8)
    ms = []
    for frame, pose in zip(frames, poses):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        leg(tree, frame, pose, scene.voxel_size, emb)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        if after_frame:
            after_frame()
    nodes = tree.count_nodes()
    tree.close()
    return ms, nodes


def high_water(leg, scene, frames, poses, emb):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free0 = torch.cuda.mem_get_info()[0]
    low = [free0]
    run_sequence(leg, scene, frames, poses, emb, after_frame=lambda: low.append(torch.cuda.mem_get_info()[0]))
    torch.cuda.empty_cache()
    return free0 - min(low)


def summary(rows):
    first = [r[0] for r in rows]
    later = [statistics.fmean(r[1:]) for r in rows]
    q = lambda xs: {"median": statistics.median(xs), "min": min(xs), "max": max(xs),
                    "p25": float(np.percentile(xs, 25)), "p75": float(np.percentile(xs, 75))}
    return {"first_frame_ms": q(first), "later_frame_ms": q(later)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "integrate_bench.json"))
    a = ap.parse_args()
    assert a.frames >= 2 and a.repeats >= 1
    assert torch.cuda.is_available(), "integrate_bench needs the GPU"
    scene = syn.room0()
    T = syn.camera_poses(scene, a.frames, seed=0)
    frames = [syn.SyntheticFrame(scene, t, scale=a.scale, device=DEV) for t in T]
    poses = [torch.from_numpy(np.asarray(t, np.float32)).to(DEV) for t in T]
    emb = torch.zeros(1, device=DEV)
    legs = {"a_torch_keys_raw_insert": leg_a, "b_insert_frame": leg_b}
    for _ in range(a.warmup):
        for leg in legs.values():
            run_sequence(leg, scene, frames, poses, emb)
    rows = {k: [] for k in legs}
    nodes = {}
    for _ in range(a.repeats):
        for k, leg in legs.items():  # alternate the legs
            ms, nodes[k] = run_sequence(leg, scene, frames, poses, emb)
            rows[k].append(ms)
    out = {"scene": "room0", "frames": a.frames, "h": frames[0].h, "w": frames[0].w, "repeats": a.repeats,
           "warmup": a.warmup, "valid_pixels": [int((f.depth > 0).sum()) for f in frames], "nodes": nodes,
           "device": torch.cuda.get_device_name(0)}
    for k, leg in legs.items():
        out[k] = summary(rows[k])
        out[k]["high_water_bytes"] = int(high_water(leg, scene, frames, poses, emb))
    sa, sb = out["a_torch_keys_raw_insert"], out["b_insert_frame"]
    for part in ("first_frame_ms", "later_frame_ms"):
        out[part + "_ratio_a_over_b"] = sa[part]["median"] / sb[part]["median"]
        # (b) counts as faster when its median lies below (a)'s by more than (a)'s own repeats spread
        out[part + "_b_faster_beyond_a_spread"] = bool(sa[part]["median"] - sb[part]["median"] > sa[part]["max"] - sa[part]["min"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
