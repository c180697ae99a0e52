"""What a frame of caller-supplied rays costs next to the ray-list path of the same number of rays (run on the GPU box):

    python tools/free_ray_time.py [--frames 10] [--warmup 3] [--profile]

One 512 x 640 sphere frame (equirectangular window around the target pose) at 64 samples per ray from 3 source views through
``MatchNeRF.render_rays`` - camera_rays + per chunk: walk over the bundle, per-sample geometry, decoder on caller-supplied
geometry, compositing -, and in the same process the same number of rays through ``render(ray_idx=arange)``: the ray-list path,
i.e. the same walk and decoder kernels fed from pixel indices.  Both exclude the encoder pass (shared, computed once).  Prints one
JSON line.  ``--profile``: only the two timed loops, once each after a warm-up, for a kernel trace

    rocprofv3 --kernel-trace --stats -d <dir> -o trace -- python tools/free_ray_time.py --profile
    python tools/rocpd_stats.py <dir>/.../trace_results.db 20

(a run of its own: no counters in the same pass)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from matchnerf_amd import camera, hip  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    if args.profile:
        args.frames, args.warmup = 2, 1
    dev = torch.device("cuda:0")
    opt, model, _ = bench.build_model(dev)
    _, batch = bench.make_batch(dev, 0)
    h, w = batch.images.shape[-2:]
    n = h * w
    legacy = bool(opt.nerf.legacy_coord)
    with torch.no_grad():
        tgt, ref = model.extract_poses(batch)
        ref_images = batch.images[:, :model.n_src_views]
        feats = model.get_img_feat(ref_images, cur_n_src_views=model.n_src_views)
        kw = dict(ref_poses=ref, ref_images=ref_images, ref_feats_list=feats)
        half_lon = float(np.arctan(0.5 * w / float(batch.intrinsics[0, -1, 0, 0])))  # the window the pinhole target sees
        cam = camera.camera_model("sphere", h, w, batch.extrinsics[0, -1, :3].cpu(), legacy=legacy, fov_deg=float(np.rad2deg(2 * half_lon)))
        idx = torch.arange(n, device=dev)

        def bundle_frame():
            rows = hip.camera_rays(cam, device=dev)
            return model.render_rays(opt, rows[:, 0:3], rows[:, 4:7], batch.near_fars[:, -1], mode="test", **kw)

        def bundle_frame_packed():  # without the [N,3] + [N,3] -> rows repacking of the public signature
            rows = hip.camera_rays(cam, device=dev)
            return model._render_bundles(opt, [rows], model._host(batch.near_fars[:, -1]).reshape(1, 2), ref, ref_images, feats)

        def ray_list_frame():
            return model.render(opt, tgt, ray_idx=idx, mode="test", **kw)

        times = {}
        for name, fn in (("bundle", bundle_frame), ("bundle_packed", bundle_frame_packed), ("ray_list", ray_list_frame)):
            for _ in range(args.warmup):
                out = fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.frames):
                out = fn()
            e1.record()
            torch.cuda.synchronize()
            times[name] = e0.elapsed_time(e1) / args.frames
            assert bool(torch.isfinite(out.rgb).all())
    print(json.dumps(dict(workload=f"{h}x{w} frame, {model.n_src_views} views, {int(opt.nerf.sample_intvs)} samples, encoder excluded",
                          rays=n, frames=args.frames, bundle_ms=round(times["bundle"], 3),
                          bundle_packed_ms=round(times["bundle_packed"], 3), ray_list_ms=round(times["ray_list"], 3),
                          ratio=round(times["bundle_packed"] / times["ray_list"], 4),
                          staging_floats_per_sample=11)))


if __name__ == "__main__":
    main()
