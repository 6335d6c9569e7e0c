"""Whole-frame render benchmark: psvo.render.FrameRenderer (csrc/render.hip)
against render_helpers.render_rays under no_grad on the same rays, in one
process, the two paths alternating frame by frame.

  python scripts/render_bench.py [--frames 10] [--train-iters 300] [--out profiles/render_frame_bench.json]

Scene: bench.py's config B (room0, 4 keyframes x 1024 rays, width 128, step
size calibrated to 64 samples per hit ray) after --train-iters untimed
bundle_adjust_frames iterations, one 1200 x 680 view, a warm-up of each path.
Per path: ms/frame from device events around each frame, rays/s, the sample
counts and torch's peak allocated bytes; the native path also at tile_rays
4096 / 16384 / 65536 with its own workspace (tile_bytes, ray_bytes: allocated
by the library, not seen by torch's allocator).

render_rays runs the decoder on every sample of its batch in one launch, which
the fused forward bounds at 4,194,272 samples: a full-resolution frame
(≈ 52 M samples) does not fit one call, so its rays go through render_rays in
chunks of --ref-chunk rays (the 200 x 160 debug render's proven size); the
whole-frame attempt and its error are recorded.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "proud-slam_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench as B  # noqa: E402  (config B's set-up, shared with the headline benchmark)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10, help="timed frames per path (>= 10 for a record)")
    ap.add_argument("--train-iters", type=int, default=300)
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--height", type=int, default=680)
    ap.add_argument("--ref-chunk", type=int, default=32768, help="rays per render_rays call")
    ap.add_argument("--tiles", type=int, nargs="*", default=[4096, 16384, 65536])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "render_frame_bench.json"))
    a = ap.parse_args()
    from psvo import _lib
    from psvo import render_helpers as RH
    from psvo import synthetic as syn
    from psvo.criterion import Criterion
    from psvo.point_feature import PointsResNet
    from psvo.render import DEFAULT_TILE_RAYS, FrameRenderer
    _lib.lib()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    args = types.SimpleNamespace(scene="room0", frames=4, rays_per_frame=1024, width=128, samples_per_ray=64.0, pool=8)
    B.log("config B: scene, keyframes, step size")
    scene, tree, ms, emb, dec = B.build_scene(args, device, 0)
    kfs = B.build_keyframes(args, scene, device, 0)
    step, spr = B.calibrate_step(ms, B.keyframe_batches(kfs, args.rays_per_frame, args.pool), args.samples_per_ray,
                                 scene.voxel_size)
    crit_cfg, max_depth = B.DEFAULT_CRITERIA
    criterion = Criterion(types.SimpleNamespace(criteria=dict(crit_cfg), data_specs={"max_depth": max_depth}))
    enc = PointsResNet(16).to(device)
    opt = [torch.optim.Adam([emb], lr=5e-3), torch.optim.Adam(dec.parameters(), lr=5e-3),
           torch.optim.Adam(enc.parameters(), lr=5e-3)]
    B.log(f"step {step:.5f} m ({spr:.1f} samples / hit ray); {a.train_iters} untimed training iterations")
    if a.train_iters > 0:
        RH.bundle_adjust_frames(kfs, ms, dec, enc, criterion, scene.voxel_size, step, args.rays_per_frame,
                                a.train_iters, 0.1, 10, max_depth, learning_rate=[1e-2, 1e-3], embed_optim=opt[0],
                                model_optim=opt[1], resnet_optim=opt[2], update_pose=True)
    torch.cuda.synchronize()
    for eng in list(getattr(RH, "_ENGINES", {}).values()):  # the mapping engine's look-ahead is not ours to keep
        eng.discard_queued()
    k = scene.intrinsics
    K = np.array([[k["fx"], 0.0, k["cx"]], [0.0, k["fy"], k["cy"]], [0.0, 0.0, 1.0]])
    T = np.asarray(syn.camera_poses(scene, 1, seed=5)[0])
    w, h = a.width, a.height
    src = (k["W"], k["H"])
    ms_r = {key: (v.detach() if torch.is_tensor(v) else v) for key, v in ms.items()}
    renderers = {t: FrameRenderer(ms_r, dec, scene.voxel_size, step, truncation=0.1, max_distance=max_depth,
                                  tile_rays=t) for t in sorted(set(a.tiles) | {DEFAULT_TILE_RAYS})}
    rays_o, rays_d = renderers[DEFAULT_TILE_RAYS].rays_of(T, K, w, h, src)
    n_rays = rays_o.shape[0]

    def native(t, seed):
        return renderers[t].render_rays(rays_o, rays_d, seed=seed)

    ref_info = {}

    def reference(seed):
        """render_rays under no_grad over the frame; -> (hit rays, samples)."""
        hit = m = 0
        with torch.no_grad():
            for c0 in range(0, n_rays, a.ref_chunk):
                ro, rd = rays_o[c0:c0 + a.ref_chunk][None], rays_d[c0:c0 + a.ref_chunk][None]
                try:
                    out = RH.render_rays(ro, rd, ms_r, dec, None, step, scene.voxel_size, 0.1, 10, max_depth,
                                         chunk_size=5000, return_raw=True, seed=seed, return_samples=True)
                except AssertionError:  # a chunk that sees nothing of the map
                    continue
                if not isinstance(out, dict):  # hit rays without a sample
                    continue
                hit += out["samples"].r_hit
                m += out["samples"].m
        return hit, m

    # the whole frame in one render_rays call: recorded, not timed
    try:
        with torch.no_grad():
            RH.render_rays(rays_o[None], rays_d[None], ms_r, dec, None, step, scene.voxel_size, 0.1, 10, max_depth,
                           chunk_size=5000, return_raw=True, seed=1)
        ref_info["whole_frame_call"] = "ok"
    except Exception as e:  # noqa: BLE001
        ref_info["whole_frame_call"] = f"{type(e).__name__}: {e}"[:300]
    torch.cuda.synchronize()
    torch.cuda.empty_cache()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.reset_peak_memory_stats()
        e0.record()
        res = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), res, torch.cuda.max_memory_allocated()

    B.log(f"{w} x {h} = {n_rays} rays; warm-up")
    warm = {t: native(t, 1) for t in renderers}
    same = all(torch.equal(warm[t][k], warm[DEFAULT_TILE_RAYS][k]) for t in renderers
               for k in ("color", "depth", "raw", "ray_mask"))
    ref_info["native_variants_bit_identical"] = bool(same)
    del warm
    reference(1)
    torch.cuda.synchronize()
    ms_nat = {t: [] for t in renderers}
    peak_nat = {t: 0 for t in renderers}
    stats_nat = {}
    ms_ref, peak_ref, ref_counts = [], 0, None
    for f in range(a.frames):  # alternating, one process
        for t in renderers:
            dt, out, peak = timed(lambda: native(t, 100 + f))
            ms_nat[t].append(dt)
            peak_nat[t] = max(peak_nat[t], peak)
            stats_nat[t] = out["stats"]
        dt, ref_counts, peak = timed(lambda: reference(100 + f))
        ms_ref.append(dt)
        peak_ref = max(peak_ref, peak)
    med = lambda v: float(np.median(v))  # noqa: E731
    res = {"scene": "room0 config B", "train_iters": a.train_iters, "step_size": step, "samples_per_hit_ray": spr,
           "view": [w, h], "n_rays": n_rays, "frames_timed": a.frames, "default_tile_rays": DEFAULT_TILE_RAYS,
           "native": {}, "render_rays": {
               "ms_per_frame": med(ms_ref), "ms_all": [round(x, 3) for x in ms_ref],
               "rays_per_s": n_rays / med(ms_ref) * 1e3, "chunk_rays": a.ref_chunk, "r_hit": ref_counts[0],
               "M": ref_counts[1], "torch_peak_allocated_bytes": peak_ref, **ref_info}}
    for t in renderers:
        st = stats_nat[t]
        res["native"][str(t)] = {
            "ms_per_frame": med(ms_nat[t]), "ms_all": [round(x, 3) for x in ms_nat[t]],
            "rays_per_s": n_rays / med(ms_nat[t]) * 1e3, "torch_peak_allocated_bytes": peak_nat[t],
            "composited_share": st["M_composited"] / max(st["M"], 1), **st}
    d = res["native"][str(DEFAULT_TILE_RAYS)]
    res["speedup_default_tile"] = res["render_rays"]["ms_per_frame"] / d["ms_per_frame"]
    for r in renderers.values():
        r.close()
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
