"""What texturing the exported mesh costs (run on the GPU box):

    python tools/mesh_texture_time.py [--runs 9] [--inner 20] [--warmup 3] [--resolution 256] [--log profiles/current/mesh_texture_time.log]

The meshes of tools/mesh_decimate_time.py (the benchmark's scene, the maps at the K = 3 source poses and at the first K = 16 poses of
the video path, a cube of ``resolution``^3 voxels), each as meshed and decimated with cells of 4 voxels, textured with blocks of 8
texels from the same K maps.  Per mesh, from one process: the atlas size, the device time of ``hip.mesh_texture_uv``,
``hip.mesh_texture_accumulate`` (one launch, K views) and ``hip.mesh_texture_resolve`` (in place) on preallocated buffers - every
figure the MEDIAN over ``runs`` windows of ``inner`` calls between two device events, with the smallest and largest window beside it
-, resolve's achieved bytes/s (it reads and writes 16 bytes per texel) beside a device copy of the same byte count timed the same
way, and the share of texels with a = 1.  Random weights: the depth maps are not a surface, so the thresholds are opened as in the
other export tools; what the kernels do per texel does not depend on it, the share of seen texels does.  The last line is the
purpose test of tests/test_mesh_texture_gpu.py on the analytic scene: the RMS colour error of the atlas and of the vertex colours
against the colour field.  One JSON line per mesh, written to ``--log``."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import bench  # noqa: E402
from matchnerf_amd import fusion, hip  # noqa: E402


def windows(fn, runs, inner, warmup):
    """-> (median, min, max) ms per call over ``runs`` windows of ``inner`` calls"""
    for _ in range(warmup * inner):
        fn()
    torch.cuda.synchronize()
    per_call = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        per_call.append(e0.elapsed_time(e1) / inner)
    return [round(x, 5) for x in (statistics.median(per_call), min(per_call), max(per_call))]


def purpose(dev):
    """fusion.mesh(texture=8, decimate=3) on the analytic scene of the tests -> the two RMS colour errors"""
    import fusion_helpers as F
    import mesh_helpers as M
    import mesh_texture_helpers as X
    k, h, w, legacy = 16, 37, 53, False
    s = F.scene(k, h, w, legacy)
    origin, voxel, dims, _ = M.grid_of(k)
    rgb = torch.from_numpy(X.view_colours(s["cams"], h, w, legacy, s["depth"], None, voxel)).to(dev)
    views = [hip.make_view(c["extr"], c["intr"], c["near"], c["far"]) for c in s["cams"]]
    bounds = (origin, tuple(origin[a] + dims[a] * voxel for a in range(3)))
    out = {}
    for cells in (0, 3):
        vertices, faces, _, atlas = fusion.mesh(views, torch.from_numpy(s["depth"]).to(dev), None, rgb, (h, w), legacy, bounds=bounds, voxel=voxel,
                                                decimate=cells, texture=8)
        textured, vertex, seen = X.colour_errors(vertices.cpu().numpy(), faces.cpu().numpy(), 8, atlas.cpu().numpy(), voxel)
        out[f"decimate_{cells}"] = dict(faces=faces.shape[0], rms_atlas=round(textured, 4), rms_vertex_colours=round(vertex, 4),
                                        samples_seen=round(seen, 3))
    return dict(workload=f"the analytic scene of the tests, {k} views of {h}x{w}, a colour field of period 2 voxels, block 8", **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--block", type=int, default=8)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "current", "mesh_texture_time.log"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    opt, model, _ = bench.build_model(dev)
    _, batch = bench.make_batch(dev, 0)
    legacy = bool(opt.nerf.legacy_coord)
    loose = dict(px_tol=64.0, rel_tol=0.5, min_opacity=0.01, min_consistent=1)
    block = args.block
    lines = ["# python tools/mesh_texture_time.py   (one MI355X, one session; ms per call: median, min, max over the windows)"]
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
            fused, counts = fusion._consistent_maps(views, depth, opacity, legacy, loose["px_tol"], loose["rel_tol"], loose["min_opacity"])
            for cells in (0, 4):
                vertices, faces = fusion.mesh(views, depth, opacity, rgb, (h, w), legacy, bounds=bounds, voxel=voxel, decimate=cells, **loose)
                vertices, faces = vertices.contiguous(), faces.contiguous()
                n_faces = faces.shape[0]
                width, height = hip.mesh_texture_atlas(n_faces, block)
                uv = torch.empty(n_faces, 3, 2, device=dev)
                accum = torch.zeros(height, width, 4, device=dev)
                spare = torch.empty_like(accum)
                bake = dict(n_consistent=counts, min_consistent=loose["min_consistent"], legacy=legacy, vis_rel_tol=0.02, power=2)
                uv_ms = windows(lambda: hip.mesh_texture_uv(n_faces, block, out=uv), args.runs, args.inner, args.warmup)
                acc_ms = windows(lambda: hip.mesh_texture_accumulate(vertices, faces, block, views, fused, rgb, accum, **bake), args.runs,
                                 args.inner, args.warmup)
                accum.zero_()
                hip.mesh_texture_accumulate(vertices, faces, block, views, fused, rgb, accum, **bake)
                atlas = hip.mesh_texture_resolve(vertices, faces, block, accum)
                seen = float((atlas[..., 3] == 1).float().mean())
                owned = 0.5 * n_faces * block * block / max(width * height, 1)
                # (resolving a resolved atlas in place again does the same reads and writes: w = 1 or 0 per texel)
                res_ms = windows(lambda: hip.mesh_texture_resolve(vertices, faces, block, atlas, out=atlas), args.runs, args.inner, args.warmup)
                copy_ms = windows(lambda: spare.copy_(atlas), args.runs, args.inner, args.warmup)
                moved = 2 * atlas.numel() * 4
                lines.append(json.dumps(dict(
                    workload=f"the mesh of {k} maps of {h}x{w} ({which}) in {args.resolution}^3 voxels", decimate_voxels=cells, faces=n_faces,
                    vertices=vertices.shape[0], block=block, atlas=[width, height], atlas_mib=round(atlas.numel() * 4 / 2 ** 20, 2),
                    runs=args.runs, inner=args.inner, uv_ms=uv_ms, accumulate_ms=acc_ms, resolve_ms=res_ms, copy_ms=copy_ms,
                    resolve_gb_per_s=round(moved / res_ms[0] / 1e6, 1), copy_gb_per_s=round(moved / copy_ms[0] / 1e6, 1),
                    texels_owned=round(owned, 4), texels_seen=round(seen, 4))))
                print(lines[-1], flush=True)
                del uv, accum, spare, atlas
        lines.append(json.dumps(purpose(dev)))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
