#!/usr/bin/env python
"""Inference entry point on the MI355X hot path (counterpart of the reference's test.py:10-33).

    python test.py --yaml=test --name=run --nerf.rand_rays_test=4096 --nerf.sample_intvs=64
    python test.py --yaml=test --name=run --gpu_ids=0,1,2,3        # sharded: one process per listed GPU

Options use the reference's ``--a.b.c=value`` grammar and YAML inheritance; the configured
test sets are served by seeded synthetic scenes when no dataset is on disk.

PSNR and SSIM are computed on the device (csrc/metrics.hip; ``MNERF_DEVICE_METRICS=0``: on the host, as the reference does).

Several GPUs: in a process without ``WORLD_SIZE``, ``--gpu_ids`` longer than one starts one fresh child process per listed GPU
through train.py's launcher (the launching process never touches a GPU); under ``torchrun`` the ranks it is given are used as they
are.  Batch ``bi`` of every test set is rendered and scored by rank ``bi % W``; rank 0 assembles the report of a one-process run and
alone writes ``0results_<set>.txt``; every rank writes the images of its own share.  ``MNERF_FORCE_DEVICE=0
MNERF_DIST_BACKEND=gloo`` runs all ranks on one GPU (dry runs, tests).  Video paths (``nerf.render_video``) are not sharded.

Video frames may come from another camera model than the batch's pinhole camera (``MatchNeRF.target_camera``):

    python test.py --yaml=demo_own --nerf.render_camera=sphere --nerf.render_fov=60 --nerf.render_hw=128,256

``--nerf.render_camera=pinhole|fisheye|sphere|ortho``, ``--nerf.render_fov=<degrees>`` (fisheye / sphere),
``--nerf.render_ortho_width=<world units>`` (ortho).  Scored evaluation refuses them: its ground truth is a pinhole image.

Geometry instead of images: ``--nerf.export_geometry=sources|path`` writes one coloured point cloud per test batch under
``<output_path>/geometry/<set>/`` (``Coach.export_geometry``: depth maps rendered at the source views' poses, or along the video
path, kept where the other poses confirm them), with ``--vis_depth`` also the colour-mapped depth maps.  Thresholds:
``--nerf.fuse_px_tol=<pixels>`` (1), ``--nerf.fuse_rel_tol=<relative depth>`` (0.01), ``--nerf.fuse_min_opacity`` (0.5),
``--nerf.fuse_min_views=<confirming views>`` (min(2, K - 1)).  With ``--nerf.export_mesh`` also a coloured triangle mesh of the same
maps, ``<stem>_mesh.ply`` (TSDF fusion, marching tetrahedra): ``--nerf.mesh_resolution=<voxels along the longest side>`` (256),
``--nerf.mesh_voxel=<world units>`` (instead of the resolution), ``--nerf.mesh_trunc=<world units>`` (4 voxels),
``--nerf.mesh_min_weight=<views per lattice point>`` (min(2, K - 1)); ``--nerf.mesh_sparse`` stores the volume in bricks of 8^3
voxels only where a surface can be - the same mesh in another row order, for resolutions (512, 1024) past the dense grid's limit of
about 560 voxels a side.  The mesh is cleaned up by
``--nerf.mesh_min_component=<triangles>`` / ``--nerf.mesh_min_component_fraction=<of the largest component>`` (smaller connected
components are dropped), ``--nerf.mesh_smooth=<rounds of Taubin smoothing>``, then reduced by ``--nerf.mesh_decimate=<cell in voxels>``
(quadric vertex clustering: one vertex per occupied cell), and ``--nerf.mesh_normals`` adds ``nx ny nz`` per vertex.
``--nerf.mesh_texture=<block in texels, 4..64>`` also writes the finished mesh with a texture atlas baked from the views,
``<stem>_mesh.obj`` / ``.mtl`` / ``.png`` next to ``<stem>_mesh.ply``: ``--nerf.mesh_texture_power=<0..8>`` (2: a view weighs
cos^power of its angle to the surface normal), ``--nerf.mesh_texture_best`` (the single best view per texel instead of the
weighted mean), ``--nerf.mesh_texture_rel_tol=<relative depth>`` (0.02: how closely a view's depth map must agree with a surface
point to count as seeing it), ``--nerf.mesh_texture_from=render|images`` (``images``: the source photographs instead of their
re-renderings; with ``--nerf.export_geometry=sources`` only), ``--nerf.mesh_texture_visibility=views|mesh`` (``mesh``: a texel's
visibility is tested against the mesh's own depth, rasterized at each view - what a decimated mesh wants).
``--nerf.mesh_report`` writes ``<stem>_mesh_report.json`` (the mesh rendered at the fusion views against the field's maps: coverage,
spurious pixels, relative depth error, PSNR, per view and pooled) and ``--nerf.mesh_preview`` writes ``<stem>_mesh_preview_<k>.png``
per fusion view, the shaded mesh next to the field's frame.

    python test.py --yaml=demo_own --nerf.export_geometry=sources
    python test.py --yaml=demo_own --nerf.export_geometry=sources --nerf.export_mesh --nerf.mesh_resolution=192
    python test.py --yaml=demo_own --nerf.export_geometry=sources --nerf.export_mesh --nerf.mesh_decimate=4 --nerf.mesh_texture=8
    python test.py --yaml=demo_own --nerf.export_geometry=sources --nerf.export_mesh --nerf.mesh_sparse --nerf.mesh_resolution=1024"""
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def run(argv):
    from matchnerf_amd import dist, options
    from matchnerf_amd.coach import Coach

    rank, world, device = 0, 1, None
    if "WORLD_SIZE" in os.environ:
        rank, world, device = dist.init_from_env()
    opt = options.set(opt_cmd=options.parse_arguments(argv), make_output_dir=rank == 0, verbose=rank == 0)
    if device is not None and not opt.cpu:
        opt.device = str(device)  # the rank's device is init_from_env's (MNERF_FORCE_DEVICE)
    cam = getattr(opt.nerf, "render_camera", None)
    if cam not in (None, "", "pinhole") and not opt.nerf.render_video:  # (before anything is built)
        raise SystemExit(f"test.py: nerf.render_camera={cam} renders video frames (nerf.render_video); scored evaluation compares "
                         "with pinhole ground truth")
    if rank == 0:
        options.save_options_file(opt)
    dist.barrier()  # the output directory exists before any rank goes on
    coach = Coach(opt)
    coach.build_networks()
    coach.restore_checkpoint()
    coach.load_dataset(splits=["test"])
    if getattr(opt.nerf, "export_geometry", None):
        if world > 1:
            raise SystemExit("test.py: nerf.export_geometry is not sharded; run it with one GPU")
        return coach.export_geometry()
    if opt.nerf.render_video:
        if world > 1:
            raise SystemExit("test.py: nerf.render_video is not sharded; run it with one GPU")
        return coach.test_model_video()
    report = coach.test_model(save_images=bool(getattr(opt, "separate_save", False)))
    if world > 1:
        import torch
        dist.barrier(always=True)
        torch.distributed.destroy_process_group()
    return report


def main(argv):
    if "WORLD_SIZE" not in os.environ:
        import train
        gpu_ids = train.requested_gpu_ids(argv)
        if len(gpu_ids) > 1:
            return train.launch(argv, gpu_ids, script=os.path.abspath(__file__))
    run(argv)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
