"""What looking at the exported mesh costs (run on the GPU box):

    python tools/mesh_raster_time.py [--runs 9] [--inner 20] [--warmup 3] [--resolution 256] [--log profiles/current/mesh_raster_time.log]

The meshes of tools/mesh_texture_time.py (the benchmark's scene, the maps at the K = 3 source poses and at the first K = 16 poses of
the video path, a cube of ``resolution``^3 voxels), each as meshed and decimated with cells of 4 voxels, seen from their own first
fusion view.  Per mesh, from one process: the device time of ``hip.mesh_raster`` (clear + raster + resolve), of ``hip.mesh_shade``
from the vertex colours and from an atlas of blocks of 8 texels, and of ``fusion.texture`` with both visibility tests (K views) -
every figure the MEDIAN over ``runs`` windows of ``inner`` calls between two device events, with the smallest and largest window
beside it -, the pixels hit and the share of texels either test sees.  Two more lines per frame size measure what the design
leaves open: ONE triangle larger than the frame (one wave walks every 8 x 8 block of the frame), and 4096 copies of it, each nearer
than the one before (every pixel takes 4096 atomic minima, h w each time at once: the rate of 8-byte integer atomics under the
worst contention, after the time of clear + resolve alone is taken off).  Random weights: the depth maps are not a surface, so
the thresholds are opened as in the other export tools.  One JSON line per measurement, written to ``--log``."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import bench  # noqa: E402
from matchnerf_amd import fusion, hip  # noqa: E402
from mesh_texture_time import windows  # noqa: E402


def frame_filling(view, h, w, copies, dev):
    """``copies`` triangles, each larger than the frame of ``view``, at camera-z 1, 1 + 2^-10, ... (the nearest is the last one) ->
    (vertices [3 copies, 8], faces [copies, 3]): lifted through the view's own matrices on the host"""
    import numpy as np
    extr = np.asarray(list(view.extr), np.float64).reshape(3, 4)
    intr = np.asarray(list(view.intr), np.float64).reshape(3, 3)
    pixels = np.array([[-2.0 * w, -2.0 * h, 1.0], [4.0 * w, -2.0 * h, 1.0], [-2.0 * w, 4.0 * h, 1.0]])
    rows = []
    for c in range(copies):
        z = 1.0 + (copies - 1 - c) / 1024.0
        cam = (np.linalg.inv(intr) @ pixels.T).T * z
        world = (np.linalg.inv(extr[:, :3]) @ (cam - extr[:, 3]).T).T
        rows.append(np.concatenate([world, np.ones((3, 1)), np.full((3, 3), 0.5), np.zeros((3, 1))], 1))
    vertices = torch.from_numpy(np.concatenate(rows).astype(np.float32)).to(dev)
    return vertices, torch.arange(3 * copies, dtype=torch.int32, device=dev).view(copies, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--block", type=int, default=8)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "current", "mesh_raster_time.log"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    opt, model, _ = bench.build_model(dev)
    _, batch = bench.make_batch(dev, 0)
    legacy = bool(opt.nerf.legacy_coord)
    loose = dict(px_tol=64.0, rel_tol=0.5, min_opacity=0.01, min_consistent=1)
    block = args.block
    timed = lambda fn: windows(fn, args.runs, args.inner, args.warmup)
    lines = ["# python tools/mesh_raster_time.py   (one MI355X, one session; ms per call: median, min, max over the windows)"]
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
            view = fusion._open_views(views)[0]
            face, z, bary = (torch.empty(h, w, dtype=torch.int32, device=dev), torch.empty(h, w, device=dev), torch.empty(h, w, 2, device=dev))
            rgba = torch.empty(h, w, 4, device=dev)
            workspace = torch.empty(hip.mesh_raster_workspace_bytes(h, w), dtype=torch.uint8, device=dev)
            for cells in (0, 4):
                vertices, faces, uv, atlas = fusion.mesh(views, depth, opacity, rgb, (h, w), legacy, bounds=bounds, voxel=voxel, decimate=cells,
                                                         texture=block, **loose)
                vertices, faces = vertices.contiguous(), faces.contiguous()
                raster = lambda: hip.mesh_raster(vertices, faces, view, (h, w), legacy=legacy, out=(face, z, bary), workspace=workspace)
                raster_ms = timed(raster)
                flat_ms = timed(lambda: hip.mesh_shade(vertices, faces, face, bary, view, out=rgba))
                atlas_ms = timed(lambda: hip.mesh_shade(vertices, faces, face, bary, view, atlas=atlas, block=block, out=rgba))
                bake = dict(block=block, **loose)
                by_views = timed(lambda: fusion.texture(vertices, faces, views, depth, opacity, rgb, (h, w), legacy, **bake))
                by_mesh = timed(lambda: fusion.texture(vertices, faces, views, depth, opacity, rgb, (h, w), legacy, visibility="mesh", **bake))
                seen = {mode: float((fusion.texture(vertices, faces, views, depth, opacity, rgb, (h, w), legacy, visibility=mode,
                                                    **bake)[1][..., 3] == 1).float().mean()) for mode in ("views", "mesh")}
                lines.append(json.dumps(dict(
                    workload=f"the mesh of {k} maps of {h}x{w} ({which}) in {args.resolution}^3 voxels, seen from its first view",
                    decimate_voxels=cells, faces=faces.shape[0], vertices=vertices.shape[0], frame=[h, w], runs=args.runs, inner=args.inner,
                    raster_resolve_ms=raster_ms, shade_vertex_colours_ms=flat_ms, shade_atlas_ms=atlas_ms, block=block,
                    pixels_hit=round(float((face >= 0).float().mean()), 4), texture_views_ms=by_views, texture_mesh_ms=by_mesh,
                    texels_seen={m: round(s, 4) for m, s in seen.items()})))
                print(lines[-1], flush=True)
            for copies in (1, 4096):  # what one wave per triangle costs on a frame-sized triangle; the atomics' rate under contention
                vertices, faces = frame_filling(view, h, w, copies, dev)
                empty = timed(lambda: hip.mesh_raster(vertices, faces[:0], view, (h, w), legacy=legacy, out=(face, z, bary), workspace=workspace))
                ms = timed(lambda: hip.mesh_raster(vertices, faces, view, (h, w), legacy=legacy, out=(face, z, bary), workspace=workspace))
                atomics = copies * h * w
                lines.append(json.dumps(dict(
                    workload=f"{copies} triangle(s) larger than the frame of {h}x{w}: {(h + 7) // 8 * ((w + 7) // 8)} blocks per wave, "
                             f"{atomics} 64-bit atomic minima, {copies} per pixel", raster_resolve_ms=ms, clear_resolve_alone_ms=empty,
                    pixels_hit=round(float((face >= 0).float().mean()), 4), winner=int(face.max()),
                    atomics_per_s=round(atomics / max(ms[0] - empty[0], 1e-6) * 1e3))))
                print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
