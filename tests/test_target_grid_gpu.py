"""Target views at a frame size of their own (mnerf_rays.tgt_height / tgt_width) on the GPU: every entry point that takes the rays
against the CPU oracle's building blocks composed for the target grid (target_grid_helpers.oracle_frame, pinned to O.render_rays by
tests/test_target_grid_cpu.py; its target rays and its projections into the source views run in the reference's k-ordered FMA
chain, so that the expected values do not depend on how the host's BLAS rounds a 3- or 4-term sum:
target_grid_helpers.target_rays_chain / project_to_view_chain), the two forms of the cost volume against each other, launch
cutting, crops, the box filter and the host paths.

ORDER: the cases run in the file's order and every parametrisation lists the grids SMALLER than the source views first
("half", "tiny", "zoom"), then the ones with more pixels ("plus": H+3 x W+5 - tile tails in both directions, "tall": 2H x W).  A
kernel that took the target size for the source's then shows as wrong numbers inside the buffers before it can read outside one.

Tolerances are the project's (tests/test_hip_kernels.py): conditioning rows 2e-5, per-sample rgb / sigma 5e-5, rendered rgb and
opacity 1e-4, depth 3e-4; matrix form within 5e-6 of the walk."""
import numpy as np
import pytest
import torch

from gpu_helpers import make_decoder_struct
from helpers import linf
from oracle import matchnerf_oracle as O
from target_grid_helpers import (SCENES, box_downsample_f32, case, expected, rays_struct, scene_on_gpu, sizes, target_intrinsics)

pytestmark = pytest.mark.gpu

TAGS = ("half", "tiny", "zoom", "plus", "tall")
GRID = [(name, tag) for tag in TAGS for name in SCENES]  # all scenes at the small grids first


@pytest.fixture(scope="module")
def hip():
    from matchnerf_amd import hip as h
    h.load()
    assert torch.cuda.is_available(), "the gpu-marked tests need a GPU"
    return h


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def _view0(hip, batch):
    return hip.make_view(batch["extrinsics"][0, 0, :3].numpy(), batch["intrinsics"][0, 0].numpy(),
                         float(batch["near_fars"][0, 0, 0]), float(batch["near_fars"][0, 0, 1]))


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("h,w", [(5, 7), (33, 21)])
@pytest.mark.parametrize("c", [1, 3])
def test_box_downsample_is_the_float32_restatement(hip, k, h, w, c):
    """width and channel tails (w * c is never a multiple of 64), one block and several; bit for bit"""
    rng = np.random.default_rng(100 * k + 10 * h + c)
    src = (rng.random((k * h, k * w, c), dtype=np.float32) - 0.25) * 3
    got = hip.box_downsample(torch.from_numpy(src).cuda(), h, w, k)
    assert got.shape == (h, w, c)
    assert np.array_equal(_bits(got), box_downsample_f32(src, k).view(np.int32))
    flat = hip.box_downsample(torch.from_numpy(src).cuda().reshape(-1, c), h, w, k)  # the layout render returns: [k h k w, C]
    assert torch.equal(flat, got)
    with pytest.raises(hip.MnerfError):
        hip.box_downsample(torch.from_numpy(src).cuda(), h, w + 1, k)


@pytest.mark.parametrize("name,tag", GRID)
def test_ray_samples_bit_exact(hip, name, tag):
    """world points, depths and view-0 coordinates of every pixel of the target grid: the oracle's bits (as the views'-size test)"""
    g, cfg, sd, batch, _, _ = case(name)
    want = expected(name, tag)
    idx = want["idx"]
    pts, ndc, depth = (t.cpu() for t in hip.ray_samples(rays_struct(name, tag), _view0(hip, batch)))
    assert pts.shape[0] == sizes(name)[tag][0] * sizes(name)[tag][1]
    assert np.array_equal(_bits(pts[idx]), _bits(want["pts"]))
    assert np.array_equal(_bits(ndc[idx]), _bits(want["x_ref"]))
    assert np.array_equal(_bits(depth[idx]), _bits(want["depth_samples"]))
    # a ray_idx list decodes with the target width too
    some = idx[::7].int().cuda()
    p2, n2, d2 = hip.ray_samples(rays_struct(name, tag, n_rays=some.numel(), ray_idx_gpu=some), _view0(hip, batch))
    assert torch.equal(p2.cpu(), pts[idx[::7]]) and torch.equal(n2.cpu(), ndc[idx[::7]])


def _cond_rows(hip, name, tag, sc, cs, **kw):
    """-> (matrix form [n, S, cs], walk [n, S, cs]) of all target pixels"""
    _, cfg, _, _, _, _ = case(name)
    th, tw = kw.get("tgt_hw") or sizes(name)[tag]
    n = th * tw
    with hip.knob("cv_mm", 1):
        mm = hip.cost_volume(sc, rays_struct(name, tag, **kw), cs).reshape(n, cfg.sample_intvs, cs)
    every = torch.arange(n, dtype=torch.int32, device="cuda")
    walk = hip.cost_volume(sc, rays_struct(name, tag, ray_idx_gpu=every, **kw), cs).reshape(n, cfg.sample_intvs, cs)
    return mm, walk


@pytest.mark.parametrize("name,tag", GRID)
def test_cost_volume_both_forms(hip, name, tag):
    g, cfg, sd, batch, _, _ = case(name)
    want = expected(name, tag)
    idx = want["idx"]
    sc, keep = scene_on_gpu(name)
    keep_op = hip.cost_volume_operands(sc)  # noqa: F841 - the operand image of the matrix form
    assert sc.feat_op
    dc = want["cond"].shape[-1]
    cs = ((dc + 1 + 7) // 8) * 8
    sum_g = sum(cfg.cos_n_group)
    mm, walk = _cond_rows(hip, name, tag, sc, cs)
    print(f"\n[{name} {tag}] rows vs oracle: walk {linf(walk[idx][..., :dc], want['cond']):.2e} matrix form "
          f"{linf(mm[idx][..., :dc], want['cond']):.2e}; matrix form vs walk {linf(mm[..., :sum_g], walk[..., :sum_g]):.2e}")
    assert linf(walk[idx][..., :dc], want["cond"]) < 2e-5
    assert linf(mm[idx][..., :dc], want["cond"]) < 2e-5
    assert linf(mm[..., :sum_g], walk[..., :sum_g]) < 5e-6
    assert torch.equal(mm[..., sum_g:], walk[..., sum_g:])  # colours, masks, the constant 1 and the padding: the same bits
    m = walk[..., dc - cfg.n_src_views:dc]
    assert bool(((m == 0) | (m == 1)).all()) and float((walk[..., dc] - 1).abs().max()) == 0.0


@pytest.mark.parametrize("name,tag", GRID)
def test_render_chunk_and_decoder_chunk(hip, name, tag):
    g, cfg, sd, batch, _, _ = case(name)
    want = expected(name, tag)
    idx = want["idx"]
    sc, keep = scene_on_gpu(name)
    keep_op = hip.cost_volume_operands(sc)  # noqa: F841
    dec, keep_dec = make_decoder_struct(cfg, sd, setbg_opaque=g["meta"]["setbg_opaque"])
    th, tw = sizes(name)[tag]
    n, s = th * tw, cfg.sample_intvs
    rgb, depth, opacity = (torch.full((n, c), -1.0, device="cuda") for c in (3, 1, 1))
    ws = torch.empty(hip.render_workspace_bytes(n, s, dec.cond_stride) // 4, device="cuda")
    hip.render_chunk(sc, dec, rays_struct(name, tag), ws, rgb, depth, opacity)
    print(f"\n[{name} {tag}] frame vs oracle: rgb {linf(rgb[idx], want['rgb']):.2e} opacity {linf(opacity[idx], want['opacity']):.2e} "
          f"depth {linf(depth[idx], want['depth']):.2e}")
    assert linf(rgb[idx], want["rgb"]) < 1e-4
    assert linf(opacity[idx], want["opacity"]) < 1e-4
    assert linf(depth[idx], want["depth"]) < 3e-4
    # the decoder on its own, from the walk's rows of the oracle's pixels: per-sample outputs
    some = idx.int().cuda()
    rays = rays_struct(name, tag, n_rays=some.numel(), ray_idx_gpu=some)
    cond = hip.cost_volume(sc, rays, dec.cond_stride)
    r2, d2, o2, rgb_s, sigma = hip.decoder_chunk(dec, sc.views[0], rays, cond, want_samples=True)
    assert linf(rgb_s, want["rgb_samples"]) < 5e-5
    assert linf(sigma, want["sigma"]) < 5e-5
    assert linf(r2, want["rgb"]) < 1e-4 and linf(o2, want["opacity"][:, 0]) < 1e-4 and linf(d2, want["depth"][:, 0]) < 3e-4


# ------------------------------------------------------------------------------------------------ the module


def _model(name):
    """the drop-in module with the golden's weights, fed the SAME source maps as the oracle (the encoder is not under test here, and
    library convolutions are not what the render's gates are about)"""
    from test_model_gpu import build_model, to_batch
    g, cfg, sd, batch, feats_pm, _ = case(name)
    opt, model = build_model(g["meta"])
    feats = [f[None].cuda().contiguous() for f in feats_pm]
    model.get_img_feat = lambda *a, **k: feats
    return opt, model, to_batch(g)


def _with_grid(batch, name, tag, **extra):
    from matchnerf_amd.edict import EasyDict
    out = EasyDict({k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()})
    out.intrinsics[0, -1] = target_intrinsics(name, tag).to(out.intrinsics.device)
    out.tgt_hw = sizes(name)[tag]
    for k, v in extra.items():
        out[k] = v
    return out


@pytest.mark.parametrize("name,tag", GRID)
def test_forward_with_batch_tgt_hw(name, tag):
    opt, model, batch = _model(name)
    want = expected(name, tag)
    idx = want["idx"]
    th, tw = sizes(name)[tag]
    with torch.no_grad():
        out = model(_with_grid(batch, name, tag), mode="test")
    assert out.rgb.shape == (1, th * tw, 3) and out.depth.shape == (1, th * tw, 1) and out.opacity.shape == (1, th * tw, 1)
    assert linf(out.rgb[0, idx], want["rgb"]) < 1e-4
    assert linf(out.opacity[0, idx], want["opacity"]) < 1e-4
    assert linf(out.depth[0, idx], want["depth"]) < 3e-4


@pytest.mark.parametrize("name", SCENES)
def test_same_size_grid_is_bit_identical_to_none(hip, name):
    from matchnerf_amd.edict import EasyDict
    opt, model, batch = _model(name)
    h, w = batch.images.shape[-2:]
    with torch.no_grad():
        plain = model(EasyDict(dict(batch)), mode="test")
        same = model(EasyDict(dict(batch), tgt_hw=(h, w)), mode="test")
    for k in ("rgb", "depth", "opacity"):
        assert torch.equal(plain[k], same[k]), k
    # and on the C ABI: 0, 0 is the views' size
    g, cfg, sd, _, _, _ = case(name)
    sc, keep = scene_on_gpu(name)
    cs = ((g["cond"].shape[-1] + 1 + 7) // 8) * 8
    r0 = rays_struct(name, "half", tgt_hw=(h, w), intr=case(name)[3]["intrinsics"][0, -1])
    r1 = rays_struct(name, "half", tgt_hw=(h, w), intr=case(name)[3]["intrinsics"][0, -1])
    r1.tgt_height = r1.tgt_width = 0
    assert torch.equal(hip.cost_volume(sc, r0, cs), hip.cost_volume(sc, r1, cs))


@pytest.mark.parametrize("name", SCENES)
def test_ray_ranges_concatenate_to_the_frame(name):
    """render(ray_range=...) on the H+3 x W+5 grid: three runs, the cuts in the middle of a row and of a 4-row tile band"""
    opt, model, batch = _model(name)
    b = _with_grid(batch, name, "plus")
    th, tw = sizes(name)["plus"]
    n = th * tw
    cut0, cut1 = 5 * tw + 13, 18 * tw + tw // 2 + 1
    assert cut0 % tw and (cut0 // tw) % 4 and cut1 % tw and (cut1 // tw) % 4 and cut1 < n
    with torch.no_grad():
        feats = model.get_img_feat()
        tgt, ref = model.extract_poses(b)
        kw = dict(mode="test", ref_poses=ref, ref_images=b.images[:, :model.n_src_views], ref_feats_list=feats, tgt_hw=(th, tw))
        whole = model.render(opt, tgt, **kw)
        parts = [model.render(opt, tgt, ray_range=(a, e - a), **kw) for a, e in ((0, cut0), (cut0, cut1), (cut1, n))]
    for k in ("rgb", "depth", "opacity"):
        assert torch.equal(torch.cat([p[k] for p in parts], 1), whole[k]), k


@pytest.mark.parametrize("name", SCENES)
def test_pose_table_at_half_size_equals_pose_by_pose(hip, name):
    """two poses of the H/2 x W/2 grid in one launch (rays_per_pose = its pixel count).  cv_mm = 0: a pose table travels with the
    segment walk, so the pose-by-pose side is pinned to the walk as well (as in tests/test_pose_table_gpu.py)"""
    opt, model, batch = _model(name)
    b = _with_grid(batch, name, "half")
    th, tw = sizes(name)["half"]
    assert (th * tw) % 64 == 0
    with torch.no_grad(), hip.knob("cv_mm", 0):
        feats = model.get_img_feat()
        tgt, ref = model.extract_poses(b)
        poses = model.get_video_rendering_path(tgt, ref, "interpolate", n_frames=6)[1:3]
        kw = dict(ref_poses=ref, ref_images=b.images[:, :model.n_src_views], ref_feats_list=feats, tgt_hw=(th, tw))
        table = model.render_poses(opt, poses, **kw)
        assert table is not None, "the shipped shape takes a pose table"
        for i, pose in enumerate(poses):
            one = model.render(opt, pose, mode="test", **kw)
            for k in ("rgb", "depth", "opacity"):
                assert torch.equal(table[k][i], one[k]), (i, k)
        assert not torch.equal(table.rgb[0], table.rgb[1])


@pytest.mark.parametrize("name", SCENES)
def test_ssaa_is_the_double_size_frame_box_filtered(name):
    from matchnerf_amd import camera
    opt, model, batch = _model(name)
    _, cfg, _, _, _, _ = case(name)
    th, tw = sizes(name)["half"]
    b = _with_grid(batch, name, "half", ssaa=2)
    hi = _with_grid(batch, name, "half")
    hi.tgt_hw = (2 * th, 2 * tw)
    hi.intrinsics[0, -1] = camera.resize_intrinsics(hi.intrinsics[0, -1], (th, tw), (2 * th, 2 * tw), cfg.legacy_coord)
    with torch.no_grad():
        got = model(b, mode="test")
        big = model(hi, mode="test")
    for k, c in (("rgb", 3), ("depth", 1), ("opacity", 1)):
        assert got[k].shape == (1, th * tw, c)
        want = box_downsample_f32(big[k][0].cpu().numpy().reshape(2 * th, 2 * tw, c), 2).reshape(th * tw, c)
        assert np.array_equal(_bits(got[k][0]), want.view(np.int32)), k


def test_training_at_another_grid_is_refused_before_any_launch(hip):
    name = "c1_default"
    g, cfg, sd, batch, _, _ = case(name)
    sc, keep = scene_on_gpu(name)
    cs = ((g["cond"].shape[-1] + 1 + 7) // 8) * 8
    idx = torch.arange(16, dtype=torch.int32, device="cuda")
    rays = rays_struct(name, "tiny", n_rays=16, ray_idx_gpu=idx)
    g_feats = [torch.zeros_like(f) for f in keep[0]]
    with pytest.raises(hip.MnerfError, match=f"rc={hip.MNERF_E_UNSUPPORTED}"):
        hip.cost_volume_backward(sc, rays, cs, torch.ones(16 * cfg.sample_intvs, cs, device="cuda"), g_feats)
    assert all(float(f.abs().max()) == 0.0 for f in g_feats)  # nothing was launched
    opt, model, b = _model(name)
    with pytest.raises(NotImplementedError):
        model(_with_grid(b, name, "tiny"), mode="train")
    tgt, ref = model.extract_poses(b)
    for p in model.parameters():
        p.requires_grad_(True)
    with pytest.raises(NotImplementedError):  # gradients through render itself, whatever the mode says
        model.render(opt, tgt, mode="test", ref_poses=ref, ref_images=b.images[:, :3], ref_feats_list=model.get_img_feat(), tgt_hw=(5, 7))


# ------------------------------------------------------------------------------------------------ crops


def _crop_case(hip, x0, y0):
    """c1_default (legacy pixel centres) seen through a camera with a power-of-two focal length and an integer principal point on
    the views' own 64 x 64 grid, and the 24 x 32 crop at (x0, y0) of it as a camera of its own: K' = K with (cx - x0, cy - y0)"""
    name = "c1_default"
    g, cfg, sd, batch, _, _ = case(name)
    h, w = batch["images"].shape[-2:]
    ch, cw = 24, 32
    K = torch.tensor([[64.0, 0.0, 32.0], [0.0, 64.0, 32.0], [0.0, 0.0, 1.0]])
    Kc = K.clone()
    Kc[0, 2], Kc[1, 2] = K[0, 2] - x0, K[1, 2] - y0
    te = batch["extrinsics"][0, -1, :3]
    _, full_ray = O.target_rays(h, w, te, K, True)
    _, crop_ray = O.target_rays(ch, cw, te, Kc, True)
    pix = ((torch.arange(ch)[:, None] + y0) * w + torch.arange(cw)[None, :] + x0).reshape(-1)
    # the precondition: the crop camera's rays ARE the full camera's at the cropped pixels, bit for bit
    assert np.array_equal(_bits(crop_ray), _bits(full_ray[pix]))
    sc, keep = scene_on_gpu(name)
    keep_op = hip.cost_volume_operands(sc)
    dec, keep_dec = make_decoder_struct(cfg, sd, setbg_opaque=g["meta"]["setbg_opaque"])
    out = {}
    for key, (th, tw, intr) in dict(full=(h, w, K), crop=(ch, cw, Kc)).items():
        n = th * tw
        rays = rays_struct(name, "half", tgt_hw=(th, tw), intr=intr)
        with hip.knob("cv_mm", 1):
            cond = hip.cost_volume(sc, rays, dec.cond_stride).reshape(n, cfg.sample_intvs, -1).clone()
        rgb, depth, opacity = (torch.empty(n, c, device="cuda") for c in (3, 1, 1))
        ws = torch.empty(hip.render_workspace_bytes(n, cfg.sample_intvs, dec.cond_stride) // 4, device="cuda")
        hip.render_chunk(sc, dec, rays, ws, rgb, depth, opacity)
        out[key] = dict(cond=cond, rgb=rgb, depth=depth, opacity=opacity)
    del keep, keep_op, keep_dec
    return {k: v[pix.cuda()] for k, v in out["full"].items()}, out["crop"]


def test_tile_aligned_crop_is_the_crop_of_the_frame(hip):
    """x0 a multiple of 8, y0 of 4: the crop's 8 x 4 tiles are tiles of the frame - the same bits from both forms' kernels"""
    full, crop = _crop_case(hip, 8, 4)
    for k in ("cond", "rgb", "depth", "opacity"):
        assert torch.equal(full[k], crop[k]), k


def test_odd_offset_crop_is_within_tolerance(hip):
    """an odd offset regroups the pixels into other tiles: the matrix form's sums run in another order"""
    full, crop = _crop_case(hip, 3, 1)
    assert linf(full["cond"], crop["cond"]) < 5e-6
    assert linf(full["rgb"], crop["rgb"]) < 1e-4 and linf(full["opacity"], crop["opacity"]) < 1e-4
    assert linf(full["depth"], crop["depth"]) < 3e-4


# ------------------------------------------------------------------------------------------------ video


@pytest.mark.parametrize("ssaa", [None, 2])
def test_video_frames_come_out_at_render_hw(tmp_path, monkeypatch, ssaa):
    """`python test.py --yaml=demo_own --nerf.render_hw=40,64 [--nerf.render_ssaa=2]`: the clip and the GIF have the requested size"""
    import os
    import test as entry
    from conftest import GOLDEN
    from PIL import Image
    monkeypatch.chdir(tmp_path)
    argv = ["--yaml=demo_own", f"--data_test.colmap.root_dir={os.path.join(GOLDEN, 'demo_data')}", "--data_test.colmap.num_workers=0",
            "--data_test.tnt=", f"--output_root={tmp_path}", "--load=", "--nerf.video_n_frames=3", "--nerf.render_hw=40,64"]
    clip = entry.run(argv + ([f"--nerf.render_ssaa={ssaa}"] if ssaa else []))["colmap"]
    assert clip.shape == (3, 40, 64, 3) and clip.dtype == np.uint8
    assert 0 < clip.std() and not np.array_equal(clip[0], clip[1])
    out_dir = tmp_path / "test_video" / "demo" / "test_videos" / "colmap"
    with Image.open(out_dir / "printer_view00_src02_01_00.gif") as im:
        assert im.n_frames == 3 and im.size == (64, 40)
    with Image.open(out_dir / "printer_view00_src02_01_00.jpg") as im:
        assert im.size == (3 * 256, 160)  # the strip of source views keeps their size
