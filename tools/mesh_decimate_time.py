"""What decimating the exported mesh costs next to the mesher that produced it (run on the GPU box):

    python tools/mesh_decimate_time.py [--runs 10] [--warmup 3] [--resolution 256] [--log profiles/current/mesh_decimate_time.log]

The two meshes of tools/mesh_finish_time.py (the benchmark's scene, the maps at the K = 3 source poses and at the first K = 16 poses
of the video path, a cube of ``resolution``^3 voxels; about 15 k and 280 k vertices).  On each mesh and for cells of 2 and 4 voxels
on the grid of the volume, from one process: ``hip.mesh_decimate`` on preallocated buffers with the adjacency given (23 launches; no
vertex_map) and ``fusion.finish(decimate_cell=...)`` as a whole, which adds the adjacency of the mesh, the allocations and the copy
of the two counts.  Prints one JSON line per mesh and cell - with the triangle counts before and after - and writes them to
``--log``."""
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
                                                  "mesh_decimate_time.log"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    opt, model, _ = bench.build_model(dev)
    _, batch = bench.make_batch(dev, 0)
    legacy = bool(opt.nerf.legacy_coord)
    loose = dict(px_tol=64.0, rel_tol=0.5, min_opacity=0.01, min_consistent=1)
    lines = ["# python tools/mesh_decimate_time.py   (one MI355X, one session)"]
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
            adj = hip.mesh_adjacency(faces, n_vertices)
            origin = tuple(float(x) for x in bounds[0])
            for cells in (2, 4):
                dims = (-(-args.resolution // cells),) * 3
                ws = torch.empty(hip.mesh_decimate_workspace_bytes(n_vertices, n_faces, dims), dtype=torch.uint8, device=dev)
                out = hip.mesh_decimate(vertices, faces, adj, origin, cells * voxel, dims, workspace=ws)
                decimate_ms, _ = timed(lambda: hip.mesh_decimate(vertices, faces, adj, origin, cells * voxel, dims, out[0], out[1], counts=out[2],
                                                                workspace=ws),
                                       args.runs, args.warmup)
                finish_ms, _ = timed(lambda: fusion.finish(vertices, faces, decimate_cell=cells * voxel, decimate_origin=origin,
                                                           decimate_dims=dims), args.runs, args.warmup)
                new_vertices, new_faces = (int(c) for c in out[2].cpu())
                lines.append(json.dumps(dict(
                    workload=f"the mesh of {k} maps of {h}x{w} ({which}) in {args.resolution}^3 voxels", runs=args.runs, cell_voxels=cells,
                    grid=list(dims), vertices=n_vertices, faces=n_faces, new_vertices=new_vertices, new_faces=new_faces,
                    faces_ratio=round(n_faces / max(new_faces, 1), 2), decimate_ms=round(decimate_ms, 4),
                    fusion_finish_decimate_ms=round(finish_ms, 3), workspace_mib=round(ws.numel() / 2 ** 20, 2))))
                print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
