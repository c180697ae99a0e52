"""Caller-supplied rays on the GPU (include/mnerf.h "CALLER-SUPPLIED RAYS"): the camera models that fill a bundle, the segment walk
over a bundle against the walk over pixels, the per-sample geometry, bundles that no pinhole camera produces against the CPU oracle
composed for a bundle (free_ray_helpers.oracle_bundle: the same float32 rows go to the oracle and to the device), and the module.

Gates.  Bit for bit wherever the same arithmetic runs on the same numbers: pinhole rows against target_rays_chain, the walk over a
bundle against the walk over pixels (padding columns included), x_ndc / depth_s against mnerf_ray_samples, chunking, the box filter.
2e-6 absolute on the unit directions (and on origins relative to the scene's scale) of the other camera models against the float64
restatement: the sine helper's measured 3.0e-7 (csrc/common.hpp) in a product of two plus a three-term rotation is < 1e-6, a margin
of 2 on top.  Against the oracle the project's gates (tests/test_target_grid_gpu.py): conditioning rows 2e-5, per-sample rgb / sigma
5e-5, rendered rgb and opacity 1e-4, depth 3e-4."""
import numpy as np
import pytest
import torch

from free_ray_helpers import SPHERE_WINDOW_DEG, camera_rows_of, expected, oracle_bundle, scene_camera
from gpu_helpers import make_decoder_struct, make_scene_struct
from helpers import linf
from target_grid_helpers import SCENES, box_downsample_f32, case, rays_struct, scene_on_gpu, sizes, target_intrinsics, target_rays_chain

pytestmark = pytest.mark.gpu

WINDOW = tuple(float(np.deg2rad(v)) * s for v in SPHERE_WINDOW_DEG for s in (-1, 1))  # lon0, lon1, lat0, lat1


@pytest.fixture(scope="module")
def hip():
    from matchnerf_amd import hip as h
    h.load()
    assert torch.cuda.is_available(), "the gpu-marked tests need a GPU"
    return h


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def _free_rays(hip, name, n, near_far=None):
    _, cfg, _, batch, _, _ = case(name)
    h, w = batch["images"].shape[-2:]
    near, far = near_far or (float(batch["near_fars"][0, -1, 0]), float(batch["near_fars"][0, -1, 1]))
    return hip.make_free_rays(n, cfg.sample_intvs, h, w, near, far, legacy=cfg.legacy_coord, depth_inverse=(cfg.depth_param == "inverse"))


def _pinhole_camera(name, tag):
    th, tw = sizes(name)[tag]
    return scene_camera(name, "pinhole", th, tw, intr=target_intrinsics(name, tag))


# ------------------------------------------------------------------------------------------------ 1, 2: camera models
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("tag", ["tiny", "plus"])
def test_pinhole_rows_are_the_bits_of_the_pixel_rays(hip, name, tag):
    _, cfg, _, batch, _, _ = case(name)
    th, tw = sizes(name)[tag]
    center, ray = target_rays_chain(th, tw, batch["extrinsics"][0, -1, :3], target_intrinsics(name, tag), cfg.legacy_coord)
    want = np.zeros((th * tw, 8), np.float32)
    want[:, 0:3], want[:, 4:7] = center.numpy(), ray.numpy()
    cam = _pinhole_camera(name, tag)
    whole = hip.camera_rays(cam)
    assert whole.shape == (th * tw, 8) and np.array_equal(_bits(whole), want.view(np.int32))
    for begin, count in ((0, tw + tw // 2), (3, 2 * tw + 1), (65, 3 * tw + 2)):  # the counts end mid-row
        if begin + count > th * tw:
            begin, count = th * tw - 4, 3  # (pixel 65 of the 5 x 7 grid: its 35 pixels end before it)
        assert (begin + count) % tw
        out = torch.full((count + 1, 8), -7.0, device="cuda")
        hip.camera_rays(cam, begin, count, out=out)
        assert np.array_equal(_bits(out[:count]), want[begin:begin + count].view(np.int32)), (begin, count)
        assert float((out[count] + 7).abs().max()) == 0.0  # nothing behind the last row


def _cameras(name):
    """(tag, hip.Camera) of the non-pinhole cases: 9 x 13 grids of every model, the full panorama, the test window"""
    _, cfg, _, batch, _, _ = case(name)
    near = float(batch["near_fars"][0, -1, 0])
    return [("fisheye 9x13 fov 100", scene_camera(name, "fisheye", 9, 13, fov_deg=100.0)),
            ("fisheye 33x47 by intrinsics", scene_camera(name, "fisheye", 33, 47, fov_deg=None)),
            ("sphere 9x13 window", scene_camera(name, "sphere", 9, 13, lon_lat=WINDOW)),
            ("sphere 16x32 panorama", scene_camera(name, "sphere", 16, 32, fov_deg=360.0)),
            ("sphere 31x17 fov 200", scene_camera(name, "sphere", 31, 17, fov_deg=200.0)),
            ("ortho 9x13", scene_camera(name, "ortho", 9, 13, ortho_width=0.5 * near)),
            ("ortho 40x24", scene_camera(name, "ortho", 40, 24, ortho_width=2.0 * near))]


@pytest.mark.parametrize("name", SCENES)
def test_fisheye_sphere_ortho_against_float64(hip, name):
    worst = 0.0
    for tag, cam in _cameras(name):
        want = camera_rows_of(cam)
        got = hip.camera_rays(cam).cpu().numpy().astype(np.float64)
        scale = max(1.0, float(np.abs(want[:, 0:3]).max()))
        e_dir = float(np.abs(got[:, 4:7] - want[:, 4:7]).max())
        e_org = float(np.abs(got[:, 0:3] - want[:, 0:3]).max()) / scale
        unit = float(np.abs(np.linalg.norm(got[:, 4:7], axis=-1) - 1).max())
        print(f"\n[{name}] {tag}: direction {e_dir:.2e} origin / scale {e_org:.2e} | |d| - 1 | {unit:.2e}")
        worst = max(worst, e_dir, e_org)
        assert np.all(got[:, 3] == 0) and np.all(got[:, 7] == 0)
        assert e_dir < 2e-6 and e_org < 2e-6 and unit < 2e-6, tag
        part = hip.camera_rays(cam, 5, cam.width + 3)  # a run that ends mid-row: the same bits as in the whole frame
        assert np.array_equal(_bits(part), got[5:5 + cam.width + 3].astype(np.float32).view(np.int32)), tag
    print(f"[{name}] worst {worst:.2e}")
    # fisheye pixels at and next to the principal point (the centre pixel of the 9 x 13 grid in either pixel convention)
    cam = _cameras(name)[0][1]
    rows = hip.camera_rays(cam).cpu().numpy().astype(np.float64).reshape(9, 13, 8)
    want = camera_rows_of(cam).reshape(9, 13, 8)
    axis = np.array(cam.c2w, np.float64).reshape(3, 4)[:, 2]
    assert np.abs(rows[4, 6, 4:7] - axis).max() < 2e-6  # theta = 0: the optical axis
    assert np.abs(rows[3:6, 5:8, 4:7] - want[3:6, 5:8, 4:7]).max() < 2e-6


# ------------------------------------------------------------------------------------------------ 3: the same walk
def _seven_views(hip):
    """the 7-view synthetic shape of tests/test_fullsize_gpu.py (32 x 48, seed 24) with random pair-major maps"""
    from matchnerf_amd import camera, synthetic as syn
    from oracle import matchnerf_oracle as O
    from gpu_helpers import images_rgba
    v, s = 7, 64
    scene = syn.make_scene(32, 48, v, seed=24)
    batch = {k: torch.from_numpy(a) for k, a in scene.items()}
    cfg = O.OracleConfig(n_src_views=v, sample_intvs=s)
    gen = torch.Generator().manual_seed(7)
    pairs = v * (v - 1) // 2
    feats = [torch.randn(pairs, 2, 32 // d, 48 // d, 128, generator=gen).cuda() for d in (8, 4)]
    img = images_rgba(batch["images"][0, :v]).cuda()
    sc = make_scene_struct(cfg, batch, feats, img)
    te, ti = batch["extrinsics"][0, -1, :3], batch["intrinsics"][0, -1]
    kinv, c2w = camera.target_ray_consts(te, ti, True)
    near, far = float(batch["near_fars"][0, -1, 0]), float(batch["near_fars"][0, -1, 1])
    cam = camera.camera_model("pinhole", 32, 48, te, ti, True)

    def pixel_rays(n, idx):
        return hip.make_rays(n, s, 32, 48, kinv, c2w, near, far, legacy=True, ray_idx_ptr=idx.data_ptr())

    return sc, (feats, img), cam, pixel_rays, hip.make_free_rays(1, s, 32, 48, near, far), 7 * 4 + 10


def _same_walk(hip, sc, cs, cam, pixel_rays, free_rays, n):
    idx = torch.arange(n, dtype=torch.int32, device="cuda")
    want = hip.cost_volume(sc, pixel_rays(n, idx), cs)  # a ray_idx list: the segment walk
    rows = hip.camera_rays(cam, 0, n)
    free_rays.n_rays = n
    got = torch.full((n * free_rays.n_samples + 1, cs), -3.0, device="cuda")
    hip.cost_volume_rays(sc, free_rays, rows, cs, out=got)
    assert float((got[-1] + 3).abs().max()) == 0.0  # nothing behind the last row
    assert torch.equal(got[:-1], want), n  # padding columns included
    return got[:-1]


@pytest.mark.parametrize("name", ["c1_default", "nonlegacy", "v4"])
@pytest.mark.parametrize("n", [1, 17, 100])
def test_walk_over_pinhole_rows_equals_the_walk_over_pixels(hip, name, n):
    """3 and 4 views: cost_volume_lean_rays_kernel<8, false> against cost_volume_lean_kernel<8, false, false>"""
    g, cfg, _, batch, _, _ = case(name)
    sc, keep = scene_on_gpu(name)
    dc = sum(cfg.cos_n_group) + 4 * cfg.n_src_views
    cs = ((dc + 1 + 7) // 8) * 8
    h, w = batch["images"].shape[-2:]
    cam = scene_camera(name, "pinhole", h, w)
    rows = _same_walk(hip, sc, cs, cam, lambda m, idx: rays_struct(name, "half", n_rays=m, ray_idx_gpu=idx, tgt_hw=(h, w), intr=batch["intrinsics"][0, -1]),
                      _free_rays(hip, name, n), n)
    assert float((rows[:, dc] - 1).abs().max()) == 0.0 and float(rows[:, dc + 1:].abs().max() if cs > dc + 1 else 0.0) == 0.0


@pytest.mark.parametrize("pair_block", [-1, 0])
@pytest.mark.parametrize("n", [1, 17, 100])
def test_walk_over_pinhole_rows_in_pair_blocks(hip, n, pair_block):
    """7 views: the pair-block instance <8, true> (21 pairs in blocks of 8 by default, in one launch with MNERF_CV_PAIR_BLOCK=0)"""
    sc, keep, cam, pixel_rays, free_rays, dc = _seven_views(hip)
    cs = ((dc + 1 + 7) // 8) * 8
    with hip.knob("cv_pair_block", pair_block):
        rows = _same_walk(hip, sc, cs, cam, pixel_rays, free_rays, n)
    assert bool(torch.isfinite(rows).all()) and float(rows[:, :10].abs().max()) <= 1.0 + 1e-5


# ------------------------------------------------------------------------------------------------ 4: geometry
@pytest.mark.parametrize("name", SCENES)
def test_ray_samples_of_pinhole_rows(hip, name):
    _, cfg, _, batch, _, _ = case(name)
    th, tw = sizes(name)["plus"]
    n = th * tw
    cam = _pinhole_camera(name, "plus")
    rows = hip.camera_rays(cam)
    view0 = hip.make_view(batch["extrinsics"][0, 0, :3].numpy(), batch["intrinsics"][0, 0].numpy(),
                          float(batch["near_fars"][0, 0, 0]), float(batch["near_fars"][0, 0, 1]))
    _, ndc, depth = hip.ray_samples(rays_struct(name, "plus"), view0)
    x_ndc, dirs, depth_s, ray_len = hip.ray_samples_rays(_free_rays(hip, name, n), rows, view0)
    assert torch.equal(x_ndc, ndc) and torch.equal(depth_s, depth)
    d64 = rows[:, 4:7].double().cpu()
    len64 = d64.norm(dim=-1)
    dir64 = (d64 / len64[:, None]) @ batch["extrinsics"][0, 0, :3, :3].double().t()
    e_dir, e_len = linf(dirs.double().cpu(), dir64[:, None].expand(-1, cfg.sample_intvs, -1)), linf(ray_len.double().cpu(), len64)
    print(f"\n[{name}] dir {e_dir:.2e} ray_len {e_len:.2e}")
    assert e_dir < 2e-6 and e_len < 2e-6
    # every output is optional
    only = hip.load().mnerf_ray_samples_rays
    import ctypes as C
    fr = _free_rays(hip, name, n)
    lens = torch.empty(n, device="cuda")
    with torch.cuda.device(0):
        assert only(C.byref(fr), rows.data_ptr(), None, None, None, None, lens.data_ptr(), None) == 0
    assert torch.equal(lens, ray_len)


# ------------------------------------------------------------------------------------------------ 5, 6: render_rays
def _render(hip, name, rows, near_far=None, setbg=None):
    g, cfg, sd, batch, _, _ = case(name)
    sc, keep = scene_on_gpu(name)
    dec, keep_dec = make_decoder_struct(cfg, sd, setbg_opaque=g["meta"]["setbg_opaque"] if setbg is None else setbg)
    n, s = rows.shape[0], cfg.sample_intvs
    rows_gpu = torch.as_tensor(rows).cuda().contiguous()
    ws = torch.full((hip.render_rays_workspace_bytes(n, s, dec.cond_stride) // 4,), float("nan"), device="cuda")
    rgb, depth, opacity = (torch.full((n, c), -1.0, device="cuda") for c in (3, 1, 1))
    hip.render_rays(sc, dec, _free_rays(hip, name, n, near_far), rows_gpu, ws, rgb, depth, opacity)
    torch.cuda.synchronize()
    stages = {k: v.clone() for k, v in hip.render_rays_workspace_views(ws, n, s, dec.cond_stride).items()}
    del keep, keep_dec
    return dict(rgb=rgb, depth=depth, opacity=opacity, **stages), dec.cond_stride


@pytest.mark.parametrize("which", ["sphere", "jitter"])
@pytest.mark.parametrize("name", SCENES)
def test_bundles_that_are_not_pinhole_match_the_oracle(hip, name, which):
    want = expected(name, which)
    got, cs = _render(hip, name, want["rows"], want["near_far"])
    dc = want["cond"].shape[-1]
    n, s = want["sigma"].shape
    err = dict(cond=linf(got["cond"].reshape(n, s, cs)[..., :dc], want["cond"]), rgb_s=linf(got["rgb_s"], want["rgb_samples"]),
               sigma=linf(got["sigma"], want["sigma"]), rgb=linf(got["rgb"], want["rgb"]), opacity=linf(got["opacity"], want["opacity"]),
               depth=linf(got["depth"], want["depth"]), x_ndc=linf(got["x_ndc"], want["x_ref"]),
               ray_len=linf(got["ray_len"].double().cpu(), want["ray_len"]))
    print(f"\n[{name} {which}] " + " ".join(f"{k} {v:.2e}" for k, v in err.items()))
    assert np.array_equal(_bits(got["x_ndc"]), _bits(want["x_ref"])) and np.array_equal(_bits(got["depth_s"]), _bits(want["depth_samples"]))
    assert err["cond"] < 2e-5
    assert err["rgb_s"] < 5e-5 and err["sigma"] < 5e-5
    assert err["rgb"] < 1e-4 and err["opacity"] < 1e-4 and err["depth"] < 3e-4
    assert err["ray_len"] < 2e-6
    if which == "sphere":  # unit directions: the depth is the oracle's sum of w t, a Euclidean distance inside [near, far]
        assert float(got["depth"].max()) <= want["near_far"][1] * (1 + 1e-5)
    stride_pad = got["cond"].reshape(n * s, cs)
    assert float((stride_pad[:, dc] - 1).abs().max()) == 0.0


@pytest.mark.parametrize("name", SCENES)
def test_pinhole_rows_render_like_the_pixel_chunk(hip, name):
    """mnerf_render_rays on pinhole rows against mnerf_render_chunk on the same pixels (a ray_idx list: the walk).  Both are tied to
    the oracle by the gates above, so those gates hold between them; expected at the 1e-6 level (only `dir` may differ by an ulp)"""
    g, cfg, sd, batch, _, _ = case(name)
    th, tw = sizes(name)["half"]
    n = th * tw
    rows = hip.camera_rays(_pinhole_camera(name, "half"))
    got, _ = _render(hip, name, rows.cpu().numpy())
    sc, keep = scene_on_gpu(name)
    dec, keep_dec = make_decoder_struct(cfg, sd, setbg_opaque=g["meta"]["setbg_opaque"])
    idx = torch.arange(n, dtype=torch.int32, device="cuda")
    rgb, depth, opacity = (torch.empty(n, c, device="cuda") for c in (3, 1, 1))
    ws = torch.empty(hip.render_workspace_bytes(n, cfg.sample_intvs, dec.cond_stride) // 4, device="cuda")
    hip.render_chunk(sc, dec, rays_struct(name, "half", ray_idx_gpu=idx), ws, rgb, depth, opacity)
    err = (linf(got["rgb"], rgb), linf(got["opacity"], opacity), linf(got["depth"], depth))
    print(f"\n[{name}] render_rays vs render_chunk: rgb {err[0]:.2e} opacity {err[1]:.2e} depth {err[2]:.2e}")
    assert err[0] < 1e-4 and err[1] < 1e-4 and err[2] < 3e-4


# ------------------------------------------------------------------------------------------------ 7: the module
def _model(name):
    from test_target_grid_gpu import _model as build
    return build(name)


def _render_kw(model, batch):
    tgt, ref = model.extract_poses(batch)
    return dict(ref_poses=ref, ref_images=batch.images[:, :model.n_src_views], ref_feats_list=model.get_img_feat())


@pytest.mark.parametrize("name", SCENES)
def test_module_render_rays_is_chunk_invariant_and_matches_the_oracle(name, monkeypatch):
    from matchnerf_amd import matchnerf as M
    opt, model, batch = _model(name)
    want = expected(name, "jitter")
    rows = torch.from_numpy(want["rows"][:200]).cuda()
    nf = torch.tensor([want["near_far"]], device="cuda")
    with torch.no_grad():
        kw = _render_kw(model, batch)
        one = model.render_rays(opt, rows[:, 0:3], rows[:, 4:7], nf, mode="test", **kw)
        monkeypatch.setattr(M, "MAX_RAYS_PER_LAUNCH", 64)
        cut = model.render_rays(opt, rows[None, :, 0:3], rows[None, :, 4:7], nf, mode="test", **kw)  # [B,N,3] as well
        monkeypatch.undo()
    assert one.rgb.shape == (1, 200, 3) and one.depth.shape == (1, 200, 1) and one.opacity.shape == (1, 200, 1)
    for k in ("rgb", "depth", "opacity"):
        assert torch.equal(one[k], cut[k]), k
        assert linf(one[k][0], want[k][:200]) < (3e-4 if k == "depth" else 1e-4), k


@pytest.mark.parametrize("name", SCENES)
def test_forward_with_a_sphere_target_camera(hip, name):
    from matchnerf_amd.edict import EasyDict
    opt, model, batch = _model(name)
    spec = dict(model="sphere", lon_lat=WINDOW)
    with torch.no_grad():
        out = model(EasyDict(dict(batch), tgt_hw=(12, 20), tgt_camera=spec), mode="test")
        out = {k: out[k].clone() for k in ("rgb", "depth", "opacity")}
        # the rows the camera produced are data: the oracle renders the very same float32 rows
        rows = hip.camera_rays(scene_camera(name, "sphere", 12, 20, lon_lat=WINDOW)).cpu().numpy()
        want = oracle_bundle(name, rows)
        err = {k: linf(out[k][0], want[k]) for k in out}
        print(f"\n[{name}] forward(sphere 12x20) vs oracle: " + " ".join(f"{k} {v:.2e}" for k, v in err.items()))
        assert out["rgb"].shape == (1, 240, 3) and out["depth"].shape == (1, 240, 1)
        assert err["rgb"] < 1e-4 and err["opacity"] < 1e-4 and err["depth"] < 3e-4
        # supersampled: the 24 x 40 bundle of the same window, box-filtered on the device
        ss = model(EasyDict(dict(batch), tgt_hw=(12, 20), tgt_camera=spec, ssaa=2), mode="test")
        ss = {k: ss[k].clone() for k in out}
        big = model(EasyDict(dict(batch), tgt_hw=(24, 40), tgt_camera=spec), mode="test")
        for k, c in (("rgb", 3), ("depth", 1), ("opacity", 1)):
            assert ss[k].shape == (1, 240, c)
            down = box_downsample_f32(big[k][0].cpu().numpy().reshape(24, 40, c), 2).reshape(240, c)
            assert np.array_equal(_bits(ss[k][0]), down.view(np.int32)), k
        # a white background is honoured
        model.nerf_setbg_opaque = True
        white = model(EasyDict(dict(batch), tgt_hw=(12, 20), tgt_camera=spec), mode="test")
        model.nerf_setbg_opaque = False
        assert torch.equal(white.opacity, out["opacity"]) and torch.equal(white.depth, out["depth"])
        assert linf(white.rgb, out["rgb"] + (1 - out["opacity"])) < 1e-6 and float((1 - out["opacity"]).max()) > 1e-3
        # a pinhole "target camera" is today's path, bit for bit
        plain = model(EasyDict(dict(batch)), mode="test")
        named = model(EasyDict(dict(batch), tgt_camera="pinhole"), mode="test")
        for k in out:
            assert torch.equal(plain[k], named[k]), k


def test_bundles_are_inference_only(hip):
    from matchnerf_amd.edict import EasyDict
    name = "c1_default"
    opt, model, batch = _model(name)
    rows = torch.from_numpy(expected(name, "jitter")["rows"][:16]).cuda()
    nf = torch.tensor([expected(name, "jitter")["near_far"]])
    kw = _render_kw(model, batch)
    launches = []
    plain = hip.render_rays
    try:
        hip.render_rays = lambda *a, **k: launches.append(1)
        with torch.no_grad(), pytest.raises(NotImplementedError):
            model.render_rays(opt, rows[:, 0:3], rows[:, 4:7], nf, mode="train", **kw)
        with pytest.raises(NotImplementedError):
            model(EasyDict(dict(batch), tgt_hw=(4, 6), tgt_camera=dict(model="sphere", lon_lat=WINDOW)), mode="train")
        for p in model.parameters():
            p.requires_grad_(True)
        with pytest.raises(NotImplementedError):  # gradients required, whatever the mode says
            model.render_rays(opt, rows[:, 0:3], rows[:, 4:7], nf, mode="test", **kw)
        with pytest.raises(NotImplementedError):
            model(EasyDict(dict(batch), tgt_hw=(4, 6), tgt_camera=dict(model="sphere", lon_lat=WINDOW)), mode="test")
    finally:
        hip.render_rays = plain
    assert not launches  # refused before the first launch
    with pytest.raises(ValueError):
        model.target_camera(EasyDict(tgt_camera="cylinder"), "test")


def test_video_frames_through_a_sphere_camera(tmp_path, monkeypatch):
    """`python test.py --yaml=demo_own --nerf.render_camera=sphere --nerf.render_fov=40 --nerf.render_hw=24,48`: the clip is written at
    the requested size, and it is not the pinhole clip"""
    import os
    import test as entry
    from conftest import GOLDEN
    from PIL import Image
    monkeypatch.chdir(tmp_path)
    argv = ["--yaml=demo_own", f"--data_test.colmap.root_dir={os.path.join(GOLDEN, 'demo_data')}", "--data_test.colmap.num_workers=0",
            "--data_test.tnt=", f"--output_root={tmp_path}", "--load=", "--nerf.video_n_frames=3", "--nerf.render_hw=24,48"]
    sphere = entry.run(argv + ["--nerf.render_camera=sphere", "--nerf.render_fov=40"])["colmap"]
    assert sphere.shape == (3, 24, 48, 3) and sphere.dtype == np.uint8 and 0 < sphere.std()
    with Image.open(tmp_path / "test_video" / "demo" / "test_videos" / "colmap" / "printer_view00_src02_01_00.gif") as im:
        assert im.n_frames == 3 and im.size == (48, 24)
    pinhole = entry.run(argv + ["--nerf.render_camera=pinhole"])["colmap"]
    assert pinhole.shape == sphere.shape and not np.array_equal(pinhole, sphere)
    with pytest.raises(SystemExit, match="render_camera"):  # scored evaluation has pinhole ground truth
        entry.run(argv + ["--nerf.render_camera=sphere", "--nerf.render_fov=40", "--nerf.render_video=false"])


@pytest.mark.parametrize("name", SCENES)
def test_pose_batching_does_not_turn_a_sphere_video_pinhole(hip, name):
    """a pose table holds pinhole constants: with pose batching on, a video through another camera model still goes pose by pose
    through its ray bundle - the frames of the per-pose loop, bit for bit, and not the pinhole frames"""
    from matchnerf_amd.edict import EasyDict
    opt, model, batch = _model(name)
    th, tw = 8, 16  # 128 rays per pose: the shipped shape takes a pose table for it
    model.opts.nerf.video_n_frames = 3
    spec = dict(model="sphere", lon_lat=WINDOW)
    clips = {}
    with torch.no_grad(), hip.knob("cv_mm", 0):
        for key, batching, cam in (("loop", False, spec), ("batched", True, spec), ("pinhole", True, None)):
            model.pose_batching = batching
            extra = dict(tgt_hw=(th, tw)) if cam is None else dict(tgt_hw=(th, tw), tgt_camera=cam)
            out = model(EasyDict(dict(batch), **extra), mode="test", render_video=True, render_path_mode="interpolate")
            clips[key] = {k: out[k].clone() for k in ("rgb", "depth", "opacity")}
    model.pose_batching = False
    for k in ("rgb", "depth", "opacity"):
        assert clips["loop"][k].shape[:2] == (3, th * tw)
        assert torch.equal(clips["batched"][k], clips["loop"][k]), k
    assert not torch.equal(clips["batched"]["rgb"], clips["pinhole"]["rgb"])
