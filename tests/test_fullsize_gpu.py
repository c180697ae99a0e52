"""Parity beyond the golden fixtures:
* a 10-source-view case (BASELINE config[4] class: 45 view pairs, cond_dim 50) vs the CPU oracle;
* a Blender-like 128-sample case with white background (config[2] class) vs the oracle;
* at the FULL benchmark size (512x640, 3 views, 64 samples) size-independent properties:
  ray-subset consistency (bit-exact), chunk-boundary invariance, closed-form opacity,
  compositing bounds, cost-volume range — the oracle cannot cover 21 M samples in seconds;
* BASELINE config[2] (Blender-like 800x800, 128 samples/ray, white background: 2500-token attention windows of a
  100x100 map) and config[4] (10 source views at 512x640: 45 view pairs, 1.18 GB of feature maps that do not fit
  the 256 MiB Infinity Cache) AT FULL SIZE: the same properties plus a 256-ray slab rendered by the CPU oracle
  from the very feature maps the GPU encoder produced."""
import numpy as np
import pytest
import torch

from helpers import linf
from matchnerf_amd import options, synthetic as syn
from matchnerf_amd.edict import EasyDict
from oracle import matchnerf_oracle as O

pytestmark = pytest.mark.gpu


def build(n_views=3, S=64, **over):
    from matchnerf_amd.models import models_dict
    opt = options.load_options("configs/test.yaml", verbose=False)
    opt.device = "cuda"
    opt.n_src_views = n_views
    opt.nerf.sample_intvs = S
    for k, v in over.items():
        node = opt
        parts = k.split(".")
        for p in parts[:-1]:
            node = node[p]
        node[parts[-1]] = v
    model = models_dict[opt.model](opt).to("cuda").eval()
    w = syn.seeded_state_dict(syn.state_dict_spec(n_src_views=n_views), 1)
    model.load_state_dict(syn.to_torch(w, "cuda"))
    return opt, model, syn.to_torch(w)


def gpu_batch(scene):
    return EasyDict({k: torch.from_numpy(v).cuda() for k, v in scene.items()})


def test_ten_source_views_match_oracle():
    opt, model, sd = build(n_views=10, S=32)
    scene = syn.make_scene(32, 48, 10, seed=21)
    with torch.no_grad():
        out = model(gpu_batch(scene), mode="test")
        cfg = O.OracleConfig(n_src_views=10, sample_intvs=32)
        ref = O.forward_test(cfg, sd, {k: torch.from_numpy(v) for k, v in scene.items()})
    assert linf(out.rgb, ref["rgb"]) < 1e-4
    assert linf(out.opacity, ref["opacity"]) < 1e-4
    assert linf(out.depth, ref["depth"]) < 3e-4


@pytest.mark.parametrize("n_views", [10, 7])
@pytest.mark.parametrize("mm", [1, 0])  # matrix form (cost_volume_mm.hip) / segment walk
def test_pair_blocked_cost_volume_is_bit_identical_to_one_launch(n_views, mm):
    """From 6 views on the cost volume runs one launch per block of view pairs (cv_walk.hpp "PAIR BLOCKS"); the per-sample
    cosine sums travel through the rows between the blocks as raw sums and are accumulated pair by pair in the same order:
    the rendered frame and the conditioning rows are bit-identical for every block size, including ragged last blocks."""
    from matchnerf_amd import hip
    opt, model, sd = build(n_views=n_views, S=40)
    scene = syn.make_scene(32, 48, n_views, seed=23)
    batch = gpu_batch(scene)
    frames = {}
    with torch.no_grad():
        for blk in (0, 8, 4, 7, 1):  # 0: all pairs in one launch (the round-3 form)
            with hip.knob("cv_pair_block", blk), hip.knob("cv_mm", mm):
                out = model(batch, mode="test")
                frames[blk] = (out.rgb.clone(), out.depth.clone(), out.opacity.clone())
    for blk, fr in frames.items():
        for a, b in zip(fr, frames[0]):
            assert torch.equal(a, b), f"pair block {blk}"


@pytest.mark.parametrize("n_views", [7, 10])
def test_ping_pong_decoder_with_wider_film_stage_equals_the_staged_kernel_and_the_oracle(n_views):
    """6-11 source views: 34-54 conditioning inputs = a FiLM stage of 3 / 4 K16-steps.  decoder_pp_kernel<64, 3|4> (round 4)
    against decoder_kernel<4,64,2,0> (the two sum layer 5 in different orders: 3e-6) and against the CPU oracle."""
    from matchnerf_amd import hip
    opt, model, sd = build(n_views=n_views, S=64)
    scene = syn.make_scene(32, 48, n_views, seed=24)
    batch = gpu_batch(scene)
    with torch.no_grad():
        pp = model(batch, mode="test")
        pp = (pp.rgb.clone(), pp.depth.clone(), pp.opacity.clone())
        with hip.knob("decoder_pp", 0):
            st = model(batch, mode="test")
        cfg = O.OracleConfig(n_src_views=n_views, sample_intvs=64)
        ref = O.forward_test(cfg, sd, {k: torch.from_numpy(v) for k, v in scene.items()})
    assert linf(pp[0], st.rgb) < 3e-6 and linf(pp[2], st.opacity) < 3e-6 and linf(pp[1], st.depth) < 3e-5
    assert linf(pp[0], ref["rgb"]) < 1e-4 and linf(pp[2], ref["opacity"]) < 1e-4 and linf(pp[1], ref["depth"]) < 3e-4


def test_blender_like_128_samples_match_oracle():
    opt, model, sd = build(n_views=3, S=128)
    model.nerf_setbg_opaque = True
    scene = syn.make_scene(48, 48, 3, seed=22, wide=True, focal_scale=1.389, near_far=(2.0, 6.0))
    with torch.no_grad():
        out = model(gpu_batch(scene), mode="test")
        cfg = O.OracleConfig(n_src_views=3, sample_intvs=128)
        ref = O.forward_test(cfg, sd, {k: torch.from_numpy(v) for k, v in scene.items()}, setbg_opaque=True)
    assert linf(out.rgb, ref["rgb"]) < 1e-4
    assert linf(out.opacity, ref["opacity"]) < 1e-4


@pytest.fixture(scope="module")
def full_frame():
    """one 512x640x3-view frame at 64 samples/ray (BASELINE config[1])"""
    opt, model, sd = build(n_views=3, S=64)
    scene = syn.make_scene(512, 640, 3, seed=0)
    batch = gpu_batch(scene)
    with torch.no_grad():
        # ONE encoder pass shared by every render below: library GEMM / conv kernels are not
        # guaranteed bitwise reproducible run to run, the render kernels are
        feats = model.get_img_feat(batch.images[:, :3], cur_n_src_views=3)
        model.get_img_feat = lambda *a, **k: feats
        out = model(batch, mode="test")
        rgb, depth, opacity = out.rgb.clone(), out.depth.clone(), out.opacity.clone()
    return opt, model, batch, scene, rgb, depth, opacity


def test_fullsize_outputs_are_finite_and_bounded(full_frame):
    _, _, _, scene, rgb, depth, opacity = full_frame
    assert rgb.shape == (1, 512 * 640, 3)
    for t in (rgb, depth, opacity):
        assert bool(torch.isfinite(t).all())
    assert float(opacity.min()) >= 0 and float(opacity.max()) <= 1 + 1e-5      # weights sum <= 1
    assert float(rgb.min()) >= 0 and float(rgb.max()) <= 1 + 1e-5
    near, far = scene["near_fars"][0, -1]
    assert float(depth.max()) <= far * (1 + 1e-5)                                # sum w d <= far
    assert float((depth - opacity * near).min()) >= -1e-4                        # sum w d >= near * sum w


def _subset_checks(model, opt, batch, feats, n_views, h, w, rgb, depth, opacity, n_sub, seed):
    """Rays are independent.  (i) A ragged CONTIGUOUS run of pixels (``ray_range``: the kernels of the full-frame path, i.e. the
    matrix form of the cost volume, other tiles and workgroup neighbours) reproduces the frame's values exactly; (ii) a random
    subset through ``ray_idx`` takes the segment walk for the cost volume (the matrix form needs contiguous pixels): the same
    cosines to a few ulp, hence the frame's values to far inside the parity gate - and exactly with the frame's cost volume
    switched to the walk as well."""
    from matchnerf_amd import hip
    tgt, ref = model.extract_poses(batch)
    first, cnt = 37 * w + 11, 9 * w + 5
    idx = torch.randperm(h * w, generator=torch.Generator().manual_seed(seed))[:n_sub].cuda()
    with torch.no_grad():
        run = model.render(opt, tgt, ray_range=(first, cnt), mode="test", ref_poses=ref, ref_images=batch.images[:, :n_views],
                           ref_feats_list=feats)
        sub = model.render(opt, tgt, ray_idx=idx, mode="test", ref_poses=ref, ref_images=batch.images[:, :n_views],
                           ref_feats_list=feats)
        with hip.knob("cv_mm", 0):
            walk = model.render(opt, tgt, ray_range=(first, cnt), mode="test", ref_poses=ref, ref_images=batch.images[:, :n_views],
                                ref_feats_list=feats)
            sub_w = model.render(opt, tgt, ray_idx=first + torch.arange(cnt, device="cuda"), mode="test", ref_poses=ref,
                                 ref_images=batch.images[:, :n_views], ref_feats_list=feats)
    assert torch.equal(run.rgb[0], rgb[0, first:first + cnt]) and torch.equal(run.depth[0], depth[0, first:first + cnt])
    assert torch.equal(run.opacity[0], opacity[0, first:first + cnt])
    assert linf(sub.rgb[0], rgb[0, idx]) < 2e-5 and linf(sub.opacity[0], opacity[0, idx]) < 2e-5 and linf(sub.depth[0], depth[0, idx]) < 1e-4
    for k in ("rgb", "depth", "opacity"):
        assert torch.equal(walk[k], sub_w[k])


def test_fullsize_ray_subset_is_bit_identical(full_frame):
    opt, model, batch, _, rgb, depth, opacity = full_frame
    with torch.no_grad():
        feats = model.get_img_feat(batch.images[:, :3], cur_n_src_views=3)
    _subset_checks(model, opt, batch, feats, 3, 512, 640, rgb, depth, opacity, 5000, 5)


def test_fullsize_chunking_is_bit_identical(full_frame, monkeypatch):
    from matchnerf_amd import matchnerf as M
    opt, model, batch, _, rgb, depth, opacity = full_frame
    monkeypatch.setattr(M, "MAX_RAYS_PER_LAUNCH", 4096 * 7 + 13)  # awkward launch size, ragged tail
    with torch.no_grad():
        out = model(batch, mode="test")
    assert torch.equal(out.rgb, rgb) and torch.equal(out.opacity, opacity) and torch.equal(out.depth, depth)


def test_fullsize_opacity_closed_form_and_cost_volume_range(full_frame):
    """opacity = 1 - exp(-sum sigma) (wo_render_interval) checked on a slab of rays through the
    staged C-ABI entry points; cosines in [-1,1], masks in {0,1}, colours in [0,1]."""
    from matchnerf_amd import camera, hip
    opt, model, batch, scene, rgb, depth, opacity = full_frame
    n0, n = 200 * 640, 4096
    tgt, ref = model.extract_poses(batch)
    with torch.no_grad():
        feats = model.get_img_feat(batch.images[:, :3], cur_n_src_views=3)
    host = lambda t: t.detach().float().cpu().numpy()
    sc = model._sources(ref, batch.images[:, :3], feats).scene(0, matrix_form=model.cv_matrix_form)
    dec = model._decoder(64, torch.device("cuda"))
    kinv, c2w = camera.target_ray_consts(host(tgt["extrinsics"])[0], host(tgt["intrinsics"])[0], True)
    nf = host(tgt["near_fars"])[0]
    rays = hip.make_rays(n, 64, 512, 640, kinv, c2w, nf[0], nf[1], ray_begin=n0)
    cond = hip.cost_volume(sc, rays, dec.cond_stride)
    r, d, o, rgb_s, sigma = hip.decoder_chunk(dec, sc.views[0], rays, cond, want_samples=True)
    assert torch.equal(r, rgb[0, n0:n0 + n]) and torch.equal(o, opacity[0, n0:n0 + n, 0])
    assert linf(o, 1 - torch.exp(-sigma.sum(1))) < 2e-5
    c = cond.reshape(n, 64, -1)
    assert float(c[..., :10].abs().max()) <= 1 + 1e-5
    assert float(c[..., 10:19].min()) >= 0 and float(c[..., 10:19].max()) <= 1 + 1e-5
    m = c[..., 19:22]
    assert bool(((m == 0) | (m == 1)).all())
    assert float((c[..., 22] - 1).abs().max()) == 0


def test_fullsize_slab_matches_oracle(full_frame):
    """BASELINE config[1] itself: 256 rays of the 512x640 headline frame rendered by the CPU
    oracle from the very feature maps the GPU encoder produced, against the frame the HIP path rendered: rgb / opacity
    1e-4 (north_star's gate), depth 3e-4."""
    opt, model, batch, scene, rgb, depth, opacity = full_frame
    sd = syn.to_torch(syn.seeded_state_dict(syn.state_dict_spec(n_src_views=3), 1))  # the weights build() loads
    first = 256 * 640 + 213
    idx = torch.arange(first, first + 256)
    with torch.no_grad():
        feats = model.get_img_feat(batch.images[:, :3], cur_n_src_views=3)
    pair_feats = [(f[0, :, 0].permute(0, 3, 1, 2).cpu(), f[0, :, 1].permute(0, 3, 1, 2).cpu()) for f in feats]
    b = {k: torch.from_numpy(val) for k, val in scene.items()}
    cfg = O.OracleConfig(n_src_views=3, sample_intvs=64)
    te, ti, tn = b["extrinsics"][0, -1, :3], b["intrinsics"][0, -1], b["near_fars"][0, -1]
    se, si, sn = b["extrinsics"][0, :-1, :3], b["intrinsics"][0, :-1], b["near_fars"][0, :-1]
    with torch.no_grad():
        ref = O.render_rays(cfg, sd, idx, te, ti, tn, se, si, sn, b["images"][0, :3], pair_feats, False)
    assert linf(rgb[0, idx], ref[0]) < 1e-4
    assert linf(opacity[0, idx], ref[2]) < 1e-4
    assert linf(depth[0, idx], ref[1]) < 3e-4


# ----------------------------------------------------------------------------- config[2] / config[4] at full size

FULL_CASES = {
    "c3_blender_800": dict(n_views=3, S=128, hw=(800, 800), scene=dict(seed=31, wide=True, focal_scale=1.389, near_far=(2.0, 6.0)),
                           bg=True),
    "c5_ten_views": dict(n_views=10, S=64, hw=(512, 640), scene=dict(seed=32), bg=False),
}


@pytest.fixture(scope="module", params=sorted(FULL_CASES))
def big_frame(request):
    c = FULL_CASES[request.param]
    opt, model, sd = build(n_views=c["n_views"], S=c["S"])
    model.nerf_setbg_opaque = c["bg"]
    h, w = c["hw"]
    scene = syn.make_scene(h, w, c["n_views"], **c["scene"])
    batch = gpu_batch(scene)
    with torch.no_grad():
        feats = model.get_img_feat(batch.images[:, :c["n_views"]], cur_n_src_views=c["n_views"])
        model.get_img_feat = lambda *a, **k: feats
        out = model(batch, mode="test")
        rgb, depth, opacity = out.rgb.clone(), out.depth.clone(), out.opacity.clone()
    yield request.param, c, opt, model, sd, batch, scene, feats, rgb, depth, opacity
    del model, feats
    torch.cuda.empty_cache()


def test_big_frame_outputs_are_finite_and_bounded(big_frame):
    name, c, _, _, _, _, scene, feats, rgb, depth, opacity = big_frame
    h, w = c["hw"]
    p = c["n_views"] * (c["n_views"] - 1) // 2
    assert rgb.shape == (1, h * w, 3) and feats[0].shape == (1, p, 2, h // 8, w // 8, 128)
    for t in (rgb, depth, opacity):
        assert bool(torch.isfinite(t).all())
    assert float(opacity.min()) >= 0 and float(opacity.max()) <= 1 + 1e-5
    assert float(rgb.min()) >= 0 and float(rgb.max()) <= 1 + 1e-5
    near, far = scene["near_fars"][0, -1]
    assert float(depth.max()) <= far * (1 + 1e-5) and float((depth - opacity * near).min()) >= -1e-4
    assert float(rgb.std()) > 1e-3   # not a constant image


def test_big_frame_ray_subset_is_bit_identical(big_frame):
    name, c, opt, model, _, batch, _, feats, rgb, depth, opacity = big_frame
    h, w = c["hw"]
    _subset_checks(model, opt, batch, feats, c["n_views"], h, w, rgb, depth, opacity, 3000, 9)


def test_big_frame_slab_matches_oracle(big_frame):
    """256 rays from the middle of the frame rendered by the CPU oracle from the GPU encoder's own feature maps
    (so the comparison isolates the render path at full size: real map sizes, real pair counts)."""
    name, c, _, _, sd, batch, scene, feats, rgb, depth, opacity = big_frame
    h, w = c["hw"]
    v = c["n_views"]
    first = (h // 2) * w + w // 3
    idx = torch.arange(first, first + 256)
    pair_feats = [(f[0, :, 0].permute(0, 3, 1, 2).cpu(), f[0, :, 1].permute(0, 3, 1, 2).cpu()) for f in feats]
    b = {k: torch.from_numpy(val) for k, val in scene.items()}
    cfg = O.OracleConfig(n_src_views=v, sample_intvs=c["S"])
    te, ti, tn = b["extrinsics"][0, -1, :3], b["intrinsics"][0, -1], b["near_fars"][0, -1]
    se, si, sn = b["extrinsics"][0, :-1, :3], b["intrinsics"][0, :-1], b["near_fars"][0, :-1]
    with torch.no_grad():
        ref = O.render_rays(cfg, sd, idx, te, ti, tn, se, si, sn, b["images"][0, :v], pair_feats, c["bg"])
    assert linf(rgb[0, idx], ref[0]) < 1e-4
    assert linf(opacity[0, idx], ref[2]) < 1e-4
    assert linf(depth[0, idx], ref[1]) < 3e-4 * (6.0 / 4.5 if c["bg"] else 1.0)


def test_big_frame_opacity_closed_form(big_frame):
    """opacity = 1 - exp(-sum sigma) on a slab through the staged C-ABI entry points; masks exactly 0/1."""
    from matchnerf_amd import camera, hip
    name, c, opt, model, _, batch, _, feats, rgb, depth, opacity = big_frame
    h, w = c["hw"]
    v, S = c["n_views"], c["S"]
    n0, n = (h // 3) * w, 2048
    tgt, ref = model.extract_poses(batch)
    sc = model._sources(ref, batch.images[:, :v], feats).scene(0, matrix_form=model.cv_matrix_form)
    dec = model._decoder(S, torch.device("cuda"))
    t_ex, t_in, t_nf = model._tgt_host(tgt)
    kinv, c2w = camera.target_ray_consts(t_ex[0], t_in[0], True)
    rays = hip.make_rays(n, S, h, w, kinv, c2w, t_nf[0, 0], t_nf[0, 1], ray_begin=n0)
    cond = hip.cost_volume(sc, rays, dec.cond_stride)
    r, d, o, rgb_s, sigma = hip.decoder_chunk(dec, sc.views[0], rays, cond, want_samples=True)
    assert torch.equal(o, opacity[0, n0:n0 + n, 0])
    assert linf(o, 1 - torch.exp(-sigma.sum(1))) < 2e-5
    cc = cond.reshape(n, S, -1)
    dc = dec.cond_dim
    m = cc[..., dc - v:dc]
    assert bool(((m == 0) | (m == 1)).all()) and float(cc[..., :dc - 4 * v].abs().max()) <= 1 + 1e-5
