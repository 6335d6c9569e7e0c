"""Mesh extraction throughput (Mapping.extract_mesh →
MeshExtractor.create_mesh, res 8, require_color) on the synthetic room0 map:
SURFACE voxels per second for the device pipeline and its stages, and the
oracle's CPU restatement (torch-CPU get_scores + numpy marching cubes) on a
bounded voxel sample beside it.  --clean: the clean_mseh branch instead
(clean_bench below), written to profiles/mesh_clean_bench.json."""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "proud-slam_amd"))
from psvo import synthetic as syn  # noqa: E402
from psvo.decoder import Decoder  # noqa: E402
from psvo.mesh import (MeshExtractor, _vertex_normals, lattice_scores, marching_cubes_device,  # noqa: E402
                       surface_states)
from psvo.octree import Octree  # noqa: E402


def _timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps, out


def _ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def clean_bench(scene, dec, sv, states, reps, n_frames, out_path):
    """create_mesh's clean_mseh branch (csrc/mesh_clean.hip) on full-size depth
    frames (SyntheticFrame at scale 1.0 from camera_poses, as integrate_bench):
    DepthPointSet.add_frame on call 1 and call n, the ball query, and
    create_mesh(clean_mseh=True) on the device and on the host path, each from
    the same n − 1 frame state.  Medians over `reps` (host: over 2)."""
    from psvo.mesh import DepthPointSet, ball_any_device
    vs = scene.voxel_size
    T = syn.camera_poses(scene, n_frames, seed=0)
    frames = [syn.SyntheticFrame(scene, t, scale=1.0, device="cuda") for t in T]
    poses = [torch.from_numpy(np.asarray(t, np.float32)).cuda() for t in T]
    rays = frames[0].rays_d
    med = lambda xs: float(np.median(xs))
    first, last, sizes = [], [], []
    for rep in range(reps + 1):  # the first pass warms up
        s = DepthPointSet("cuda")
        per = [_ms(lambda: s.add_frame(poses[i], frames[i].depth, rays))[0] for i in range(n_frames)]
        if rep:
            first.append(per[0])
            last.append(per[-1])
        sizes = int(s.points.shape[0])
    # the state before the last frame, for the create_mesh legs
    s = DepthPointSet("cuda")
    for i in range(n_frames - 1):
        s.add_frame(poses[i], frames[i].depth, rays)
    before = s.numpy()
    s.add_frame(poses[-1], frames[-1].depth, rays)
    mx = MeshExtractor(types.SimpleNamespace(mapper_specs={"voxel_size": vs}))
    mx.rays_d = rays.cpu()
    c = states["voxel_center_xyz"]
    _, sdf = lattice_scores(dec, states, vs, 8, with_rgb=False)
    verts, faces = marching_cubes_device(c, sdf, vs, 8)
    t_ball = med([_ms(lambda: ball_any_device(s.points, verts, vs * 0.5))[0] for _ in range(reps + 1)][1:])
    depth_host = frames[-1].depth.cpu()

    # the vertex normals' ordered sum (psvo.mesh._vertex_normals) beside the atomic one it replaced
    def normals_atomic():
        f = faces.long()
        p0, p1, p2 = verts[f[:, 0]], verts[f[:, 1]], verts[f[:, 2]]
        fn = torch.cross(p1 - p0, p2 - p0, dim=-1)
        vn = torch.zeros_like(verts)
        for k in range(3):
            vn.index_add_(0, f[:, k], fn)
        return vn / vn.norm(dim=-1, keepdim=True).clamp_min(1e-12)

    t_nrm = {"ordered_index_put": med([_ms(lambda: _vertex_normals(verts, faces))[0] for _ in range(reps + 1)][1:]),
             "atomic_index_add": med([_ms(normals_atomic)[0] for _ in range(reps + 1)][1:])}
    n1, n2 = _vertex_normals(verts, faces), _vertex_normals(verts, faces)
    t_nrm["ordered_repeatable"] = bool(torch.equal(n1, n2))
    t_nrm["max_abs_diff_to_atomic"] = float((n1 - normals_atomic()).abs().max())

    def leg(clean):
        mx.depth_points = before  # not timed: every repeat starts from the same state
        depth = frames[-1].depth if clean == "device" else depth_host
        pose = poses[-1] if clean == "device" else poses[-1].cpu()
        return _ms(lambda: mx.create_mesh(dec, states, vs, sv, pose, depth, clean_mseh=True, require_color=True,
                                          offset=-10, res=8, clean=clean))

    t_plain = med([_ms(lambda: mx.create_mesh(dec, states, vs, sv, require_color=True, offset=-10, res=8))[0]
                   for _ in range(reps + 1)][1:])
    dev = [leg("device") for _ in range(reps + 1)][1:]
    host = [leg("host") for _ in range(3)][1:]
    f_dev, f_host = dev[-1][1].triangles.shape[0], host[-1][1].triangles.shape[0]
    out = {"scene": scene.name, "h": frames[0].h, "w": frames[0].w, "frames": n_frames, "reps": reps,
           "device": torch.cuda.get_device_name(0), "host_threads": os.cpu_count(),
           "depth_points_after_last_frame": sizes, "depth_points_before_last_frame": int(before.shape[0]),
           "vertices": int(verts.shape[0]), "triangles": int(faces.shape[0]),
           "kept_face_share": {"device": f_dev / faces.shape[0], "host": f_host / faces.shape[0]},
           "ms": {"add_frame_call_1": med(first), f"add_frame_call_{n_frames}": med(last), "ball_query": t_ball,
                  "create_mesh_no_clean": t_plain, "vertex_normals": t_nrm,
                  "create_mesh_clean_device": med([t for t, _ in dev]),
                  "create_mesh_clean_host": med([t for t, _ in host])}}
    out["host_over_device"] = out["ms"]["create_mesh_clean_host"] / out["ms"]["create_mesh_clean_device"]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reps", nargs="?", type=int, default=10)
    ap.add_argument("--clean", action="store_true", help="time the clean_mseh branch (device and host paths)")
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_clean_bench.json"))
    a = ap.parse_args()
    reps = a.reps
    scene = syn.room0()
    tree = Octree()
    tree.init(scene.grid_dim, 16, scene.voxel_size, 8)
    tree.insert(syn.surface_voxels(scene, seed=0))
    voxels, _, features = tree.export_arrays()
    gen = torch.Generator().manual_seed(0)
    emb = (torch.randn(voxels.shape[0], 16, generator=gen) * 0.3).cuda()
    torch.manual_seed(0)
    dec = Decoder(depth=2, width=128, in_dim=16, skips=[], embedder="none").cuda()
    sv, states = surface_states(torch.from_numpy(voxels), torch.from_numpy(features), emb, scene.voxel_size)
    n = sv.shape[0]
    vs = scene.voxel_size
    if a.clean:
        return clean_bench(scene, dec, sv, states, reps, a.frames, a.out)
    mx = MeshExtractor(types.SimpleNamespace(mapper_specs={"voxel_size": vs}))
    t_scores, _ = _timed(lambda: lattice_scores(dec, states, vs, 8), reps)
    t_sdf, (_, sdf) = _timed(lambda: lattice_scores(dec, states, vs, 8, with_rgb=False), reps)
    c = states["voxel_center_xyz"]
    t_mc, (v, f) = _timed(lambda: marching_cubes_device(c, sdf, vs, 8), reps)
    t_all, mesh = _timed(lambda: mx.create_mesh(dec, states, vs, sv, require_color=True, offset=-10, res=8), reps)
    out = {"surface_voxels": n, "lattice_points": n * 512, "vertices": int(v.shape[0]), "triangles": int(f.shape[0]),
           "ms": {"lattice_scores_rgb_sdf": 1e3 * t_scores, "lattice_sdf": 1e3 * t_sdf,
                  "marching_cubes": 1e3 * t_mc,
                  "create_mesh_with_colour": 1e3 * t_all},
           "voxels_per_s": n / t_all}
    # CPU oracle on a bounded sample
    from oracle import mesh_oracle as MO
    k = min(n, 256)
    params = {kk: vv.cpu() for kk, vv in dec.state_dict().items()}
    cc = c[:k].cpu()
    t0 = time.perf_counter()
    sc = MO.get_scores(params, cc, states["voxel_vertex_idx"][:k].cpu(), emb.cpu(), vs, 8)
    MO.marching_cubes(cc.numpy(), sc[..., 3].numpy(), vs)
    el = time.perf_counter() - t0
    out["cpu_oracle"] = {"voxels": k, "s": el, "voxels_per_s": k / el, "threads": torch.get_num_threads()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
