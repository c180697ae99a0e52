"""Target views at any frame size, the parts that need no GPU: the intrinsics of a resized grid, the two new fields of mnerf_rays,
the options, the fixed summation order of the box filter and the host-only argument checks of the new export."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from matchnerf_amd import camera, hip, options
from oracle import matchnerf_oracle as O
from target_grid_helpers import SCENES, box_downsample_f32, case, oracle_frame, project_to_view_chain, target_rays_chain


def _K(dtype=np.float32):
    return np.array([[410.5, 0.25, 317.25], [0.0, 395.0, 240.5], [0.0, 0.0, 1.0]], dtype)


def _corner_rays(K, h, w, legacy):
    """un-normalised camera-frame rays through the four corners of an (h, w) frame: kinv applied by hand, float64"""
    lo, (hx, hy) = (-0.5, (w - 0.5, h - 0.5)) if legacy else (0.0, (float(w), float(h)))
    pix = np.array([[lo, lo, 1.0], [hx, lo, 1.0], [lo, hy, 1.0], [hx, hy, 1.0]])
    return pix @ np.linalg.inv(np.asarray(K, np.float64)).T


@pytest.mark.parametrize("legacy", [True, False])
@pytest.mark.parametrize("tgt_hw", [(240, 320), (483, 645), (5, 7), (960, 640)])
def test_resize_intrinsics_keeps_the_field_of_view(legacy, tgt_hw):
    src_hw = (480, 640)
    K = _K(np.float64)
    Kr = camera.resize_intrinsics(K, src_hw, tgt_hw, legacy)
    sx, sy = tgt_hw[1] / src_hw[1], tgt_hw[0] / src_hw[0]
    M = np.array([[sx, 0, 0.5 * sx - 0.5], [0, sy, 0.5 * sy - 0.5], [0, 0, 1]]) if legacy else np.diag([sx, sy, 1.0])
    np.testing.assert_allclose(Kr, M @ K, rtol=1e-15, atol=0)
    a, b = _corner_rays(K, *src_hw, legacy), _corner_rays(Kr, *tgt_hw, legacy)
    assert np.abs(a - b).max() <= 1e-6 * np.abs(a).max()
    # the oracle's own rays through the corner PIXELS of both grids bracket the same frustum: a resized grid's corner pixel centre
    # lies half a (resized) pixel inside the frame corner, as the source grid's does
    eye = torch.eye(4)[:3]
    _, ray_t = O.target_rays(tgt_hw[0], tgt_hw[1], eye, torch.from_numpy(Kr).float(), legacy)
    off = 0.0 if legacy else 0.5
    want = np.array([off, off, 1.0]) @ np.linalg.inv(Kr).T
    np.testing.assert_allclose(ray_t[0].numpy(), want, rtol=1e-5, atol=1e-7)


def test_resize_intrinsics_identity_dtype_and_batch():
    K = _K()
    assert camera.resize_intrinsics(K, (480, 640), (480, 640), True) is K
    Kt = torch.from_numpy(np.stack([K, 2 * K]))
    for legacy in (True, False):
        host = camera.resize_intrinsics(Kt.numpy(), (480, 640), (483, 645), legacy)
        dev = camera.resize_intrinsics(Kt, (480, 640), (483, 645), legacy)
        assert host.dtype == np.float32 and dev.dtype == torch.float32 and host.shape == (2, 3, 3)
        assert np.array_equal(host, dev.numpy())  # a host copy and a tensor give the same bits
        assert np.array_equal(host[0], camera.resize_intrinsics(K, (480, 640), (483, 645), legacy))
    with pytest.raises(ValueError):
        camera.resize_intrinsics(K, (480, 640), (0, 7), True)


def test_make_rays_target_fields_and_header():
    kinv, c2w = np.eye(3, dtype=np.float32), np.eye(4, dtype=np.float32)[:3]
    r = hip.make_rays(128, 64, 8, 16, kinv, c2w, 2.0, 6.0)
    assert (r.tgt_height, r.tgt_width) == (0, 0) and (r.height, r.width) == (8, 16)
    r = hip.make_rays(35, 64, 8, 16, kinv, c2w, 2.0, 6.0, tgt_hw=(5, 7))
    assert (r.tgt_height, r.tgt_width) == (5, 7) and (r.height, r.width) == (8, 16)
    names = [n for n, _ in hip.Rays._fields_]
    assert names[-4:] == ["rays_per_pose", "tgt_height", "tgt_width", "pad_"]
    lib = hip.load()
    assert lib.mnerf_abi_version() == 12  # the layout change travels under the same version: the size check catches a stale mirror
    assert lib.mnerf_struct_size(hip.STRUCTS.index(hip.Rays)) == ctypes.sizeof(hip.Rays) == 160 + 8
    # the mirror's fields are the header's, in order
    text = open(os.path.join(os.path.dirname(__file__), "..", "include", "mnerf.h")).read()
    body = re.search(r"typedef struct mnerf_rays \{(.*?)\} mnerf_rays;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    declared = [n for st in body.split(";") if st.strip()
                for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", st.strip().replace("*", " "))]
    assert declared == names, (declared, names)
    assert "mnerf_box_downsample" in hip.EXPORTS and hasattr(lib, "mnerf_box_downsample")


def test_render_options_parse():
    cmd = options.parse_arguments(["--yaml=test", "--nerf.render_hw=96,128", "--nerf.render_ssaa=2"])
    assert cmd.nerf.render_hw == [96, 128] and cmd.nerf.render_ssaa == 2
    opt = options.set(cmd, make_output_dir=False, verbose=False)
    assert list(opt.nerf.render_hw) == [96, 128] and opt.nerf.render_ssaa == 2
    plain = options.set(options.parse_arguments(["--yaml=test"]), make_output_dir=False, verbose=False)
    assert getattr(plain.nerf, "render_hw", None) is None and getattr(plain.nerf, "render_ssaa", None) is None


@pytest.mark.parametrize("k", [1, 2, 3, 8])
@pytest.mark.parametrize("c", [1, 3])
def test_box_filter_restatement_against_float64(k, c):
    rng = np.random.default_rng(k * 10 + c)
    src = rng.random((33 * k, 21 * k, c), dtype=np.float32) + 0.25  # away from zero: a relative bound is meaningful
    got = box_downsample_f32(src, k)
    want = src.astype(np.float64).reshape(33, k, 21, k, c).mean((1, 3))
    assert got.dtype == np.float32 and got.shape == (33, 21, c)
    assert np.abs(got / want - 1).max() <= 1e-6  # 63 additions and a scale at 2^-24 each, random signs: ~5e-7 at worst
    if k == 1:
        assert np.array_equal(got, src)


def test_box_downsample_argument_checks_need_no_gpu():
    lib = hip.load()
    fn = lib.mnerf_box_downsample
    p = 1 << 20  # made-up, non-NULL: every check precedes the launch
    assert fn(p, 4, 4, 3, 0, p, None) == hip.MNERF_E_RANGE and b"k=0" in lib.mnerf_last_error()
    assert fn(p, 4, 4, 3, 9, p, None) == hip.MNERF_E_RANGE
    assert fn(p, 4, 4, 2, 2, p, None) == hip.MNERF_E_RANGE and b"channels=2" in lib.mnerf_last_error()
    assert fn(p, 4, 4, 4, 2, p, None) == hip.MNERF_E_RANGE
    assert fn(p, -1, 4, 3, 2, p, None) == hip.MNERF_E_RANGE
    assert fn(None, 4, 4, 3, 2, p, None) == hip.MNERF_E_NULL
    assert fn(p, 4, 4, 3, 2, None, None) == hip.MNERF_E_NULL
    assert fn(None, 0, 4, 3, 2, None, None) == hip.MNERF_OK  # an empty frame reads and writes nothing


def test_target_size_argument_checks_need_no_gpu():
    """a negative or half-set target size, and a run of pixels past the target grid, are refused before any launch"""
    lib = hip.load()
    kinv, c2w = np.eye(3, dtype=np.float32), np.eye(4, dtype=np.float32)[:3]
    p = 1 << 20
    view = hip.make_view(c2w, kinv, 2.0, 6.0)

    def rc(n_rays=35, ray_begin=0, **fields):
        r = hip.make_rays(n_rays, 8, 8, 16, kinv, c2w, 2.0, 6.0, ray_begin=ray_begin)
        for k, v in fields.items():
            setattr(r, k, v)
        return lib.mnerf_ray_samples(ctypes.byref(r), ctypes.byref(view), p, p, p, None)

    assert rc(tgt_height=5, tgt_width=0) == hip.MNERF_E_RANGE and b"target grid" in lib.mnerf_last_error()
    assert rc(tgt_height=0, tgt_width=7) == hip.MNERF_E_RANGE
    assert rc(tgt_height=-5, tgt_width=7) == hip.MNERF_E_RANGE
    assert rc(tgt_height=5, tgt_width=-7) == hip.MNERF_E_RANGE
    assert rc(n_rays=36, tgt_height=5, tgt_width=7) == hip.MNERF_E_RANGE and b"outside the 5x7" in lib.mnerf_last_error()
    assert rc(n_rays=30, ray_begin=6, tgt_height=5, tgt_width=7) == hip.MNERF_E_RANGE
    assert rc(n_rays=129) == hip.MNERF_E_RANGE and b"outside the 8x16" in lib.mnerf_last_error()  # 0, 0 = the views' size
    assert rc(n_rays=0, tgt_height=5, tgt_width=7) == hip.MNERF_OK  # an empty chunk launches nothing
    # the backward of the cost volume: a differing target grid is refused before the scene is even looked at closely
    sc = hip.Scene()
    sc.n_views, sc.n_scales = 3, 1
    sc.fh[0], sc.fw[0], sc.n_group[0] = 1, 2, 2
    sc.feat[0], sc.images = p, p
    r = hip.make_rays(35, 8, 8, 16, kinv, c2w, 2.0, 6.0, ray_idx_ptr=p, tgt_hw=(5, 7))
    assert lib.mnerf_cost_volume_backward(ctypes.byref(sc), ctypes.byref(r), 16, p, p, None, None) == hip.MNERF_E_UNSUPPORTED
    assert b"target grid 5x7" in lib.mnerf_last_error()


@pytest.mark.parametrize("name", SCENES)
def test_oracle_composition_equals_render_rays_at_the_views_size(name):
    """pins the helper the GPU tests take their expected values from: with the target grid = the views' size and the batch's own
    intrinsics it IS O.render_rays, bit for bit"""
    g, cfg, sd, batch, _, pair_feats = case(name)
    h, w = batch["images"].shape[-2:]
    idx = torch.from_numpy(g["stage_rays"]).long()
    te, ti, tn, se, si, sn = (batch["extrinsics"][0, -1, :3], batch["intrinsics"][0, -1], batch["near_fars"][0, -1],
                              batch["extrinsics"][0, :-1, :3], batch["intrinsics"][0, :-1], batch["near_fars"][0, :-1])
    with torch.no_grad():
        want = O.render_rays(cfg, sd, idx, te, ti, tn, se, si, sn, batch["images"][0, :cfg.n_src_views], pair_feats,
                             g["meta"]["setbg_opaque"], return_stages=True)
        got = oracle_frame(cfg, sd, batch, pair_feats, (h, w), ti, ray_idx=idx, setbg_opaque=g["meta"]["setbg_opaque"])
    for k in ("rgb", "depth", "opacity", "cond", "x_ref", "rgb_samples", "sigma", "depth_samples"):
        assert torch.equal(got[k], want[k]), k


@pytest.mark.parametrize("name", SCENES)
def test_chain_projection_is_the_reference_arithmetic(name):
    """the host-independent projection the expected values go through: the reference's own bits (the golden's x_ref, recorded
    from its CPU path) and, on any host, within the 1e-6 at which the project holds O.project_to_view to the reference"""
    g, cfg, sd, batch, _, _ = case(name)
    h, w = batch["images"].shape[-2:]
    se, si, sn = batch["extrinsics"][0, 0, :3], batch["intrinsics"][0, 0], batch["near_fars"][0, 0]
    pts = torch.from_numpy(g["pts"])
    got = project_to_view_chain(pts, se, si, w, h, sn[0], sn[1])
    assert np.array_equal(got.numpy().view(np.int32), g["x_ref"].view(np.int32))
    assert float((got - O.project_to_view(pts, se, si, w, h, sn[0], sn[1])).abs().max()) < 1e-6


@pytest.mark.parametrize("name", SCENES)
def test_chain_target_rays_are_the_reference_arithmetic(name):
    """the host-independent target rays: with the depths of the oracle they give the reference's own world points (the golden's
    pts, bit for bit), and on any host they lie within float32 rounding of O.target_rays - also on grids of other sizes, where
    a BLAS may sum in another order"""
    g, cfg, sd, batch, _, _ = case(name)
    h, w = batch["images"].shape[-2:]
    te, ti, tn = batch["extrinsics"][0, -1, :3], batch["intrinsics"][0, -1], batch["near_fars"][0, -1]
    idx = torch.from_numpy(g["stage_rays"]).long()
    center, ray = target_rays_chain(h, w, te, ti, cfg.legacy_coord)
    d = O.depth_samples(cfg, tn[0], tn[1], idx.numel())
    pts = center[idx][:, None] + ray[idx][:, None] * d[..., None]
    assert np.array_equal(pts.numpy().view(np.int32), g["pts"].view(np.int32))
    for th, tw in ((h, w), (5, 7), (2 * h, w), (h + 3, w + 5)):
        c0, r0 = O.target_rays(th, tw, te, ti, cfg.legacy_coord)
        c1, r1 = target_rays_chain(th, tw, te, ti, cfg.legacy_coord)
        assert torch.equal(c0, c1) and float((r0 - r1).abs().max()) <= 4e-7 * float(r0.abs().max())
