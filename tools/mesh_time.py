"""What the mesh export costs next to the renders it consumes (run on the GPU box):

    python tools/mesh_time.py [--runs 10] [--warmup 3] [--resolution 256] [--log profiles/current/mesh_time.log]

The benchmark's scene (3 source views of 512 x 640).  K = 3: the maps rendered at the source views' own poses; K = 16: at the first
16 poses of the video path.  From the same process and the same maps: the render time of one frame (``MatchNeRF.render``, encoder
excluded), ``hip.tsdf_integrate`` of the K fused maps into a cube of ``resolution``^3 voxels around the cloud's box (trunc = 4 voxels,
the box padded by it, min_weight = 2), ``hip.tsdf_mesh`` on that volume (nine launches), and ``fusion.mesh`` as a whole at that
resolution along the box's longest side (its default grid follows the box, so it has fewer voxels than the cube) - which adds the K
consistency launches, the box (K compactions, a min / max and the copy) and the copy of the two counts.  Random weights: the depth
maps are not a surface, so the thresholds are opened as in tools/fusion_time.py; the integrator's work does not depend on what
survives, the mesher's scatter does - the vertex and face counts are printed with the times.  Prints one JSON line per K and writes
them to ``--log``.

``--sparse`` adds, per K and for every cube of ``--sparse-resolutions`` (default: the dense resolution, 512 and 1024), the brick-sparse
volume on the same maps: ``hip.tsdf_bricks_mark``, ``tsdf_bricks_table``, ``tsdf_integrate_sparse``, ``tsdf_mesh_sparse`` and
``fusion.mesh(sparse=True)`` as a whole, with the bricks allocated, their bytes and the distance to the bound of 349 525 bricks (a
resolution whose surface exceeds it is reported with its count and not meshed); the default log is then
``profiles/current/tsdf_sparse_time.log``."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from fusion_time import timed  # noqa: E402
from matchnerf_amd import fusion, hip  # noqa: E402


def sparse_times(args, k, which, views, fused, counts, depth, opacity, rgb, hw, legacy, loose, lo, hi, resolution):
    """the stages of the sparse volume on a cube of resolution^3 voxels laid as the dense one -> the log's dict"""
    dev = fused.device
    voxel = float((hi - lo).max()) / (resolution - 8)
    trunc = 4.0 * voxel
    origin = tuple(float(x) for x in 0.5 * (lo + hi) - 0.5 * resolution * voxel)
    dims = (resolution,) * 3
    bdims = hip.brick_dims(dims)
    maps = dict(n_consistent=counts, min_consistent=loose["min_consistent"], legacy=legacy)
    marks = torch.zeros(bdims[::-1], dtype=torch.uint8, device=dev)
    mark_ms, _ = timed(lambda: (marks.zero_(), hip.tsdf_bricks_mark(views, fused, origin, voxel, dims, trunc, marks, **maps)), args.runs,
                       args.warmup)
    table, bricks, count = hip.tsdf_bricks_table(marks, bdims)
    ws = torch.empty(max(16, hip.tsdf_bricks_table_workspace_bytes(bdims)), dtype=torch.uint8, device=dev)
    table_ms, _ = timed(lambda: hip.tsdf_bricks_table(marks, bdims, table, bricks, count, workspace=ws), args.runs, args.warmup)
    n_bricks = int(count.cpu())
    out = dict(workload=f"sparse: {k} maps of {hw[0]}x{hw[1]} ({which}) into a virtual grid of {resolution}^3 voxels", runs=args.runs,
               bricks=n_bricks, bricks_of=bdims[0] * bdims[1] * bdims[2], bricks_bound=hip.MAX_BRICKS,
               share_of_bound=round(n_bricks / hip.MAX_BRICKS, 4), mark_ms=round(mark_ms, 4), table_ms=round(table_ms, 4),
               volume_mib=round(20 * 512 * n_bricks / 2 ** 20, 1), tables_mib=round(9 * marks.numel() / 2 ** 20, 1),
               dense_volume_mib=round(20 * resolution ** 3 / 2 ** 20, 1))
    if n_bricks > hip.MAX_BRICKS or n_bricks == 0:
        return dict(out, note="beyond the bound of the sparse mesher: not integrated or meshed" if n_bricks else "no brick")
    sums, weight = torch.zeros(n_bricks, 512, 4, device=dev), torch.zeros(n_bricks, 512, device=dev)
    zero_ms, _ = timed(lambda: (sums.zero_(), weight.zero_()), args.runs, args.warmup)
    integrate_ms, _ = timed(lambda: (sums.zero_(), weight.zero_(),
                                     hip.tsdf_integrate_sparse(views, fused, rgb, origin, voxel, dims, trunc, bricks, n_bricks, sums, weight,
                                                               **maps)), args.runs, args.warmup)
    mesh_ws = torch.empty(hip.tsdf_mesh_sparse_workspace_bytes(n_bricks, bdims), dtype=torch.uint8, device=dev)
    totals = torch.zeros(2, dtype=torch.int64, device=dev)
    run = lambda v, f: hip.tsdf_mesh_sparse(sums, weight, table, bricks, n_bricks, origin, voxel, dims, 2.0, v, f, counts=totals, workspace=mesh_ws)
    run(torch.empty(0, 8, device=dev), torch.empty(0, 3, dtype=torch.int32, device=dev))
    n_vertices, n_faces = (int(c) for c in totals.cpu())
    vertices, faces = torch.empty(n_vertices, hip.VERTEX_FLOATS, device=dev), torch.empty(n_faces, 3, dtype=torch.int32, device=dev)
    mesh_ms, _ = timed(lambda: run(vertices, faces), args.runs, args.warmup)
    whole_ms, _ = timed(lambda: fusion.mesh(views, depth, opacity, rgb, hw, legacy, resolution=resolution, sparse=True, **loose), args.runs,
                        args.warmup)
    return dict(out, integrate_ms=round(integrate_ms - zero_ms, 4), mesh_ms=round(mesh_ms, 4), fusion_mesh_sparse_ms=round(whole_ms, 3),
                vertices=n_vertices, faces=n_faces, workspace_mib=round(mesh_ws.numel() / 2 ** 20, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--sparse", action="store_true")
    ap.add_argument("--sparse-resolutions", type=int, nargs="*", default=None)
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    if args.log is None:
        args.log = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "current",
                                "tsdf_sparse_time.log" if args.sparse else "mesh_time.log")
    if args.sparse_resolutions is None:
        args.sparse_resolutions = sorted({args.resolution, 512, 1024})
    dev = torch.device("cuda:0")
    opt, model, _ = bench.build_model(dev)
    _, batch = bench.make_batch(dev, 0)
    legacy = bool(opt.nerf.legacy_coord)
    loose = dict(px_tol=64.0, rel_tol=0.5, min_opacity=0.01, min_consistent=1)
    lines = ["# python tools/mesh_time.py   (one MI355X, one session)"]
    with torch.no_grad():
        _, ref = model.extract_poses(batch)
        k_src = model.n_src_views
        ref_images = batch.images[:, :k_src]
        feats = model.get_img_feat(ref_images, cur_n_src_views=k_src)
        pose = dict(extrinsics=ref["extrinsics"][:, 0], intrinsics=ref["intrinsics"][:, 0], near_fars=ref["near_fars"][:, 0])
        frame_ms, _ = timed(lambda: model.render(opt, pose, mode="test", ref_poses=ref, ref_images=ref_images, ref_feats_list=feats),
                            args.runs, args.warmup)
        opt.nerf.video_n_frames = 18  # (the interpolated path has n // 3 poses per leg)
        for k, which in ((3, "sources"), (16, "path")):
            clouds, maps = model.export_points(batch, views=which, return_maps=True, **loose)
            h, w = maps.hw
            views = maps.views[0][:k]
            depth, opacity, rgb = maps.depth[0, :k].contiguous(), maps.opacity[0, :k].contiguous(), maps.rgb[0, :k].contiguous()
            assert len(views) == k, (which, len(views))
            fused = torch.empty(k, h, w, device=dev)
            counts = torch.empty(k, h, w, dtype=torch.int32, device=dev)
            arr = hip.view_array(views)
            for r in range(k):
                hip.depth_consistency(arr, r, depth, opacity, legacy=legacy, out=(fused[r], counts[r]),
                                      **{a: loose[a] for a in ("px_tol", "rel_tol", "min_opacity")})
            cloud = fusion.fuse(views, depth, opacity, rgb, (h, w), legacy, **loose)
            lo, hi = cloud[:, :3].amin(0).double().cpu().numpy(), cloud[:, :3].amax(0).double().cpu().numpy()
            # a CUBE of resolution^3 voxels around the box's centre that holds the box padded by trunc = 4 voxels
            voxel = float((hi - lo).max()) / (args.resolution - 8)
            trunc = 4.0 * voxel
            origin = tuple(float(x) for x in 0.5 * (lo + hi) - 0.5 * args.resolution * voxel)
            dims = (args.resolution,) * 3
            nx, ny, nz = dims
            sums, weight = torch.zeros(nz, ny, nx, 4, device=dev), torch.zeros(nz, ny, nx, device=dev)

            def integrate():
                sums.zero_(), weight.zero_()
                return hip.tsdf_integrate(views, fused, rgb, origin, voxel, dims, trunc, sums, weight, n_consistent=counts,
                                          min_consistent=loose["min_consistent"], legacy=legacy)

            zero_ms, _ = timed(lambda: (sums.zero_(), weight.zero_()), args.runs, args.warmup)
            integrate_ms, _ = timed(integrate, args.runs, args.warmup)
            integrate_ms -= zero_ms
            ws = torch.empty(hip.tsdf_mesh_workspace_bytes(dims), dtype=torch.uint8, device=dev)
            totals = torch.zeros(2, dtype=torch.int64, device=dev)
            hip.tsdf_mesh(sums, weight, origin, voxel, dims, 2.0, torch.empty(0, 8, device=dev),
                          torch.empty(0, 3, dtype=torch.int32, device=dev), counts=totals, workspace=ws)
            n_vertices, n_faces = (int(c) for c in totals.cpu())
            vertices = torch.empty(n_vertices, hip.VERTEX_FLOATS, device=dev)
            faces = torch.empty(n_faces, 3, dtype=torch.int32, device=dev)
            mesh_ms, _ = timed(lambda: hip.tsdf_mesh(sums, weight, origin, voxel, dims, 2.0, vertices, faces, counts=totals, workspace=ws),
                               args.runs, args.warmup)
            whole_ms, _ = timed(lambda: fusion.mesh(views, depth, opacity, rgb, (h, w), legacy, resolution=args.resolution, **loose),
                                args.runs, args.warmup)
            lines.append(json.dumps(dict(
                workload=f"{k} maps of {h}x{w} ({which}) into {nx}x{ny}x{nz} voxels, {int(opt.nerf.sample_intvs)} samples per ray",
                runs=args.runs, render_ms_per_frame=round(frame_ms, 3), integrate_ms=round(integrate_ms, 4), mesh_ms=round(mesh_ms, 4),
                fusion_mesh_ms=round(whole_ms, 3), vertices=n_vertices, faces=n_faces, voxels=nx * ny * nz,
                updated_voxels=int((weight > 0).sum()), integrate_over_one_frame=round(integrate_ms / frame_ms, 4),
                mesh_over_one_frame=round(mesh_ms / frame_ms, 4), volume_mib=round(20 * nx * ny * nz / 2 ** 20, 1),
                workspace_mib=round(ws.numel() / 2 ** 20, 1))))
            print(lines[-1], flush=True)
            for resolution in (args.sparse_resolutions if args.sparse else ()):
                lines.append(json.dumps(sparse_times(args, k, which, views, fused, counts, depth, opacity, rgb, (h, w), legacy, loose, lo, hi,
                                                     resolution)))
                print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
