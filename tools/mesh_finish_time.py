"""What finishing the exported mesh costs next to the mesher that produced it (run on the GPU box):

    python tools/mesh_finish_time.py [--runs 10] [--warmup 3] [--resolution 256] [--log profiles/current/mesh_finish_time.log]

The two meshes of tools/mesh_time.py: the benchmark's scene (3 source views of 512 x 640), the maps rendered at the K = 3 source poses
and at the first K = 16 poses of the video path, fused into a cube of ``resolution``^3 voxels and meshed by ``hip.tsdf_mesh`` (random
weights: the thresholds are opened as there; about 15 k and 280 k vertices).  On each mesh, from one process: the five stages of
include/mnerf.h "MESH FINISHING" on preallocated buffers - ``hip.mesh_adjacency`` (eight launches), ``hip.mesh_components`` (six),
``hip.mesh_compact`` with the keep bytes of ``min_fraction = 0.01`` (eight), ``hip.mesh_smooth`` with 10 rounds (twenty) and
``hip.mesh_normals`` (one) - and ``fusion.finish(min_component_fraction=0.01, smooth=10)`` as a whole, which adds the allocations, the
copy of the two counts and the adjacency of the result.  Prints one JSON line per mesh and writes them to ``--log``."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from fusion_time import timed  # noqa: E402
from matchnerf_amd import fusion, hip  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--log", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "current",
                                                  "mesh_finish_time.log"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    opt, model, _ = bench.build_model(dev)
    _, batch = bench.make_batch(dev, 0)
    legacy = bool(opt.nerf.legacy_coord)
    loose = dict(px_tol=64.0, rel_tol=0.5, min_opacity=0.01, min_consistent=1)
    lines = ["# python tools/mesh_finish_time.py   (one MI355X, one session)"]
    with torch.no_grad():
        opt.nerf.video_n_frames = 18  # (the interpolated path has n // 3 poses per leg)
        for k, which in ((3, "sources"), (16, "path")):
            clouds, maps = model.export_points(batch, views=which, return_maps=True, **loose)
            h, w = maps.hw
            views = maps.views[0][:k]
            depth, opacity, rgb = maps.depth[0, :k].contiguous(), maps.opacity[0, :k].contiguous(), maps.rgb[0, :k].contiguous()
            cloud = clouds[0][:, :3]
            lo, hi = cloud.amin(0).double().cpu().numpy(), cloud.amax(0).double().cpu().numpy()
            voxel = float((hi - lo).max()) / (args.resolution - 8)  # the cube of tools/mesh_time.py
            bounds = (tuple(0.5 * (lo + hi) - 0.5 * args.resolution * voxel), tuple(0.5 * (lo + hi) + 0.5 * args.resolution * voxel))
            vertices, faces = fusion.mesh(views, depth, opacity, rgb, (h, w), legacy, bounds=bounds, voxel=voxel, **loose)
            n_vertices, n_faces = vertices.shape[0], faces.shape[0]
            ws = torch.empty(hip.mesh_finish_workspace_bytes(n_vertices, n_faces), dtype=torch.uint8, device=dev)
            adj = hip.mesh_adjacency(faces, n_vertices, workspace=ws)
            adjacency_ms, _ = timed(lambda: hip.mesh_adjacency(faces, n_vertices, out=adj, workspace=ws), args.runs, args.warmup)
            parts = hip.mesh_components(faces, n_vertices, 0, 0.01, workspace=ws)
            components_ms, _ = timed(lambda: hip.mesh_components(faces, n_vertices, 0, 0.01, out=parts, workspace=ws), args.runs, args.warmup)
            kept = hip.mesh_compact(vertices, faces, parts[1], workspace=ws)
            compact_ms, _ = timed(lambda: hip.mesh_compact(vertices, faces, parts[1], *kept, workspace=ws), args.runs, args.warmup)
            smoothed = torch.empty_like(vertices)
            smooth_ms, _ = timed(lambda: hip.mesh_smooth(vertices, faces, adj, 10, out=smoothed, workspace=ws), args.runs, args.warmup)
            normals = hip.mesh_normals(vertices, faces, adj)
            normals_ms, _ = timed(lambda: hip.mesh_normals(vertices, faces, adj, out=normals), args.runs, args.warmup)
            finish_ms, _ = timed(lambda: fusion.finish(vertices, faces, min_component_fraction=0.01, smooth=10), args.runs, args.warmup)
            kept_vertices, kept_faces = (int(c) for c in kept[2].cpu())
            lines.append(json.dumps(dict(
                workload=f"the mesh of {k} maps of {h}x{w} ({which}) in {args.resolution}^3 voxels", runs=args.runs, vertices=n_vertices,
                faces=n_faces, components=int(torch.unique(parts[0]).numel()), kept_vertices=kept_vertices, kept_faces=kept_faces,
                interior_vertices=int(adj[2].sum()), adjacency_ms=round(adjacency_ms, 4), components_ms=round(components_ms, 4),
                compact_ms=round(compact_ms, 4), smooth_10_rounds_ms=round(smooth_ms, 4), normals_ms=round(normals_ms, 4),
                fusion_finish_ms=round(finish_ms, 3), workspace_mib=round(ws.numel() / 2 ** 20, 2))))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
