"""What the geometry export costs next to the renders it consumes (run on the GPU box):

    python tools/fusion_time.py [--runs 10] [--warmup 3]

The benchmark's scene (3 source views of 512 x 640) exported from the source views' own poses, K = 3 fusion frames: from the same
process and the same maps, the render time of the K frames (``MatchNeRF.render`` at each pose, encoder excluded), the K
consistency launches, the K compactions (four launches each), the K colour maps, and ``fusion.fuse`` as a whole - which adds the
one device->host copy of the counts and the joining of the segments.  Random weights: the depth maps are not a surface, so the
thresholds are opened until about half of the pixels survive - the kernels' work does not depend on what survives, the joining's
does.  Prints one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from matchnerf_amd import fusion, hip  # noqa: E402


def timed(fn, runs, warmup):
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(runs):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / runs, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    opt, model, _ = bench.build_model(dev)
    _, batch = bench.make_batch(dev, 0)
    h, w = batch.images.shape[-2:]
    n, k = h * w, model.n_src_views
    legacy = bool(opt.nerf.legacy_coord)
    loose = dict(px_tol=64.0, rel_tol=0.5, min_opacity=0.01, min_consistent=1)
    with torch.no_grad():
        _, ref = model.extract_poses(batch)
        ref_images = batch.images[:, :k]
        feats = model.get_img_feat(ref_images, cur_n_src_views=k)
        kw = dict(ref_poses=ref, ref_images=ref_images, ref_feats_list=feats)
        poses = [dict(extrinsics=ref["extrinsics"][:, v], intrinsics=ref["intrinsics"][:, v], near_fars=ref["near_fars"][:, v])
                 for v in range(k)]
        hosts = [model._tgt_host(p) for p in poses]
        views = [hip.make_view(ex[0], it[0], nf[0, 0], nf[0, 1]) for ex, it, nf in hosts]

        render_ms, rets = timed(lambda: [model.render(opt, p, mode="test", **kw) for p in poses], args.runs, args.warmup)
        depth = torch.stack([r.depth[0, :, 0] for r in rets]).reshape(k, h, w).contiguous()
        opacity = torch.stack([r.opacity[0, :, 0] for r in rets]).reshape(k, h, w).contiguous()
        rgb = torch.stack([r.rgb[0] for r in rets]).contiguous()
        out = [(torch.empty(h, w, device=dev), torch.empty(h, w, dtype=torch.int32, device=dev)) for _ in range(k)]
        arr = hip.view_array(views)
        short = (20 * args.runs, args.warmup)  # launches of tens of microseconds: a window of 200 repetitions
        consistency_ms, _ = timed(lambda: [hip.depth_consistency(arr, r, depth, opacity, legacy=legacy, out=out[r], **{
            a: loose[a] for a in ("px_tol", "rel_tol", "min_opacity")}) for r in range(k)], *short)
        points = torch.empty(k * n, hip.POINT_FLOATS, device=dev)
        counts = torch.zeros(k, dtype=torch.int64, device=dev)
        ws = torch.empty(hip.point_cloud_workspace_bytes(n), dtype=torch.uint8, device=dev)
        compaction_ms, _ = timed(lambda: [hip.point_cloud(views[r], (h, w), out[r][0], rgb[r], out[r][1], loose["min_consistent"],
                                                          legacy=legacy, points=points[r * n:(r + 1) * n], count=counts[r:r + 1],
                                                          workspace=ws) for r in range(k)], *short)
        panel = torch.empty(h, w, 3, dtype=torch.uint8, device=dev)
        near, far = float(hosts[0][2][0, 0]), float(hosts[0][2][0, 1])
        colormap_ms, _ = timed(lambda: [hip.depth_colormap(depth[r], near, far, out=panel) for r in range(k)], *short)
        fuse_ms, cloud = timed(lambda: fusion.fuse(views, depth, opacity, rgb, (h, w), legacy, **loose), *short)
    print(json.dumps(dict(workload=f"{k} fusion frames of {h}x{w} from {k} views, {int(opt.nerf.sample_intvs)} samples, encoder excluded",
                          runs=args.runs, render_ms=round(render_ms, 3), render_ms_per_frame=round(render_ms / k, 3),
                          consistency_ms=round(consistency_ms, 4), compaction_ms=round(compaction_ms, 4),
                          colormap_ms=round(colormap_ms, 4), fuse_ms=round(fuse_ms, 4), points=int(cloud.shape[0]), pixels=k * n,
                          fusion_launches_over_one_frame=round((consistency_ms + compaction_ms) / (render_ms / k), 5),
                          host_syncs_per_scene=1)))


if __name__ == "__main__":
    main()
