"""Caller-supplied rays without a GPU: the ABI additions, the argument checks of the free-ray entry points (all of them precede
any HIP call), the options, and the float64 restatement of the camera models that the GPU tests compare the device with."""
import ctypes as C

import numpy as np
import pytest

from helpers import read_header
from matchnerf_amd import camera, hip, options
from free_ray_helpers import camera_rows_f64, expected, sphere_window
from target_grid_helpers import SCENES, case, sizes, target_intrinsics, target_rays_chain

NEW_EXPORTS = ("mnerf_cost_volume_rays", "mnerf_ray_samples_rays", "mnerf_render_rays_workspace_bytes", "mnerf_render_rays",
               "mnerf_camera_rays")
FAKE = 0x10000  # a non-NULL, 16-byte aligned "device" address: the calls below fail their checks or have nothing to launch


def test_exports_struct_and_constants():
    header = read_header()
    names = [name for _, name, _ in header.prototypes]
    for name in NEW_EXPORTS:
        assert name in hip.EXPORTS and name in names, name
    lib = hip.load()
    assert lib.mnerf_abi_version() == 12 == hip.MNERF_ABI_VERSION == header.constants["MNERF_ABI_VERSION"]
    assert C.sizeof(hip.Rays) == 168 == lib.mnerf_struct_size(1)  # the bundle pointer is no field of mnerf_rays
    which = header.constants["MNERF_STRUCT_CAMERA"]
    assert which == hip.STRUCT_CAMERA and which >= len(hip.STRUCTS) and hip.Camera not in hip.STRUCTS
    assert lib.mnerf_struct_size(which) == C.sizeof(hip.Camera) == 4 * 4 + 4 * (9 + 12 + 4)
    assert lib.mnerf_struct_size(which + 1) == -1 and lib.mnerf_struct_size(len(hip.STRUCTS)) == -1
    camera_rays = next(params for _, name, params in header.prototypes if name == "mnerf_camera_rays")
    assert camera_rays[0] == "const void*"  # untyped: the by-type argument structs stay the ones the bindings count
    assert hip.MNERF_RAY_FLOATS == header.constants["MNERF_RAY_FLOATS"] == 8
    for i, name in enumerate(camera.CAMERA_MODELS):
        assert header.constants["MNERF_CAM_" + name.upper()] == i == getattr(hip, "CAM_" + name.upper())


def _scene(n_views=3):
    sc = hip.Scene()
    sc.n_views, sc.n_scales = n_views, 2
    for s, (fh, g) in enumerate(((8, 2), (16, 8))):
        sc.fh[s], sc.fw[s], sc.n_group[s], sc.feat[s] = fh, fh, g, FAKE
    sc.images = FAKE
    return sc


def _decoder(n_views=3):
    d = hip.Decoder()
    d.n_views, d.cond_dim, d.cond_stride = n_views, 10 + 4 * n_views, 24
    return d


def _rays(n_rays, **kw):
    r = hip.make_free_rays(n_rays, 8, 64, 64, 2.0, 4.0)
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def _calls(lib, rays, ray_od):
    """every free-ray entry point on the same rays struct and bundle pointer -> {name: rc}"""
    sc, dec, view = _scene(), _decoder(), hip.View()
    return {
        "cost_volume_rays": lib.mnerf_cost_volume_rays(C.byref(sc), C.byref(rays), ray_od, 24, FAKE, None),
        "ray_samples_rays": lib.mnerf_ray_samples_rays(C.byref(rays), ray_od, C.byref(view), FAKE, FAKE, FAKE, FAKE, None),
        "render_rays": lib.mnerf_render_rays(C.byref(sc), C.byref(dec), C.byref(rays), ray_od, FAKE, FAKE, FAKE, FAKE, None),
    }


def test_argument_checks_need_no_device():
    lib = hip.load()
    for name, rc in _calls(lib, _rays(5), None).items():
        assert rc == hip.MNERF_E_NULL and b"ray_od is NULL" in lib.mnerf_last_error(), name
    for off in (4, 8, 12):
        for name, rc in _calls(lib, _rays(5), FAKE + off).items():
            assert rc == hip.MNERF_E_ALIGN, (name, off)
    assert b"16B aligned" in lib.mnerf_last_error()
    for field in ("ray_idx", "pose_table"):
        for name, rc in _calls(lib, _rays(5, **{field: FAKE}), FAKE).items():
            assert rc == hip.MNERF_E_UNSUPPORTED, (name, field)
        for name, rc in _calls(lib, _rays(0, **{field: FAKE}), None).items():  # also for an empty launch
            assert rc == hip.MNERF_E_UNSUPPORTED, (name, field)
    assert b"ray_idx / pose_table" in lib.mnerf_last_error()
    for name, rc in _calls(lib, _rays(-1), FAKE).items():
        assert rc == hip.MNERF_E_RANGE, name
    # an empty launch touches no buffer
    sc, dec, rays = _scene(), _decoder(), _rays(0)
    assert lib.mnerf_cost_volume_rays(C.byref(sc), C.byref(rays), None, 24, None, None) == hip.MNERF_OK
    assert lib.mnerf_ray_samples_rays(C.byref(rays), None, None, None, None, None, None, None) == hip.MNERF_OK
    assert lib.mnerf_render_rays(C.byref(sc), C.byref(dec), C.byref(rays), None, None, None, None, None, None) == hip.MNERF_OK
    # the remaining checks of a non-empty launch, still before any HIP call
    rays = _rays(5)
    assert lib.mnerf_cost_volume_rays(C.byref(sc), C.byref(rays), FAKE, 24, None, None) == hip.MNERF_E_NULL  # cond
    assert lib.mnerf_cost_volume_rays(C.byref(sc), C.byref(rays), FAKE, 16, FAKE, None) == hip.MNERF_E_RANGE  # cond_stride < 23
    assert lib.mnerf_render_rays(C.byref(sc), C.byref(dec), C.byref(rays), FAKE, None, FAKE, FAKE, FAKE, None) == hip.MNERF_E_NULL
    assert lib.mnerf_render_rays(C.byref(sc), C.byref(dec), C.byref(rays), FAKE, FAKE + 8, FAKE, FAKE, FAKE, None) == hip.MNERF_E_ALIGN
    assert lib.mnerf_render_rays(C.byref(sc), C.byref(_decoder(4)), C.byref(rays), FAKE, FAKE, FAKE, FAKE, FAKE, None) == hip.MNERF_E_RANGE
    assert lib.mnerf_ray_samples_rays(C.byref(rays), FAKE, None, FAKE, None, None, None, None) == hip.MNERF_E_NULL  # view0 for x_ndc
    # the decoder's own refusals, as far as they can be told before the first step is enqueued
    assert lib.mnerf_render_rays(C.byref(sc), C.byref(dec), C.byref(rays), FAKE, FAKE, FAKE, FAKE, FAKE, None) == hip.MNERF_E_NULL
    assert b"decoder weights" in lib.mnerf_last_error()
    dec.wstream, dec.small_, dec.L_3D, dec.wstream_format = FAKE, FAKE, 10, hip.WSTREAM_F16X2
    dec.wstream_floats = lib.mnerf_decoder_wstream_floats(22, 24, 10, hip.WSTREAM_F16X2) - 8
    assert lib.mnerf_render_rays(C.byref(sc), C.byref(dec), C.byref(rays), FAKE, FAKE, FAKE, FAKE, FAKE, None) == hip.MNERF_E_RANGE
    dec.wstream_format = 7
    assert lib.mnerf_render_rays(C.byref(sc), C.byref(dec), C.byref(rays), FAKE, FAKE, FAKE, FAKE, FAKE, None) == hip.MNERF_E_UNSUPPORTED
    dec.wstream_format, dec.wstream = hip.WSTREAM_F16X2, FAKE + 4
    assert lib.mnerf_render_rays(C.byref(sc), C.byref(dec), C.byref(rays), FAKE, FAKE, FAKE, FAKE, FAKE, None) == hip.MNERF_E_ALIGN
    many = _rays(5, n_samples=257)
    dec.wstream = FAKE
    assert lib.mnerf_render_rays(C.byref(sc), C.byref(dec), C.byref(many), FAKE, FAKE, FAKE, FAKE, FAKE, None) == hip.MNERF_E_UNSUPPORTED


def test_camera_rays_argument_checks():
    lib = hip.load()
    cam = camera.camera_model("sphere", 4, 6, np.eye(4)[:3], legacy=False, fov_deg=90)
    assert lib.mnerf_camera_rays(None, 0, 1, FAKE, None) == hip.MNERF_E_NULL
    assert lib.mnerf_camera_rays(C.byref(cam), 0, 24, None, None) == hip.MNERF_E_NULL
    assert lib.mnerf_camera_rays(C.byref(cam), 0, 24, FAKE + 4, None) == hip.MNERF_E_ALIGN
    assert lib.mnerf_camera_rays(C.byref(cam), 3, 22, FAKE, None) == hip.MNERF_E_RANGE  # one pixel past the grid
    assert lib.mnerf_camera_rays(C.byref(cam), -1, 2, FAKE, None) == hip.MNERF_E_RANGE
    assert lib.mnerf_camera_rays(C.byref(cam), 24, 0, None, None) == hip.MNERF_OK  # nothing to do
    cam.model = 4
    assert lib.mnerf_camera_rays(C.byref(cam), 0, 1, FAKE, None) == hip.MNERF_E_RANGE
    with pytest.raises(ValueError):
        camera.camera_model("cylinder", 4, 6, np.eye(4)[:3])
    with pytest.raises(ValueError):
        camera.camera_model("ortho", 4, 6, np.eye(4)[:3])  # no width


def test_workspace_bytes_formula():
    lib = hip.load()
    f = lib.mnerf_render_rays_workspace_bytes
    assert f(-1, 8, 24) == -1 and f(4, 0, 24) == -1 and f(4, 8, 0) == -1
    assert f(0, 8, 24) == 0
    prev = 0
    for r in (1, 2, 3, 5, 17, 100, 65536):
        for s, cs in ((1, 8), (7, 24), (64, 24), (128, 96)):
            b = f(r, s, cs)
            n = r * s
            up4 = lambda x: (x + 3) & ~3  # noqa: E731
            assert b == 4 * (up4(n * cs) + 3 * up4(3 * n) + 2 * up4(n) + up4(r)) and b % 16 == 0
            assert b >= lib.mnerf_render_workspace_bytes(r, s, cs) + 4 * 11 * n  # the conditioning rows + 11 staging floats per sample
            assert f(r + 1, s, cs) > b and f(r, s + 1, cs) > b and f(r, s, cs + 1) >= b
        assert f(r, 64, 24) > prev
        prev = f(r, 64, 24)
    assert f(65536, 256, 96) > 2 ** 32  # 64-bit


def test_options_parse_and_default_to_none():
    cmd = options.parse_arguments(["--yaml=test", "--nerf.render_camera=sphere", "--nerf.render_fov=60", "--nerf.render_ortho_width=2.5"])
    assert cmd.nerf.render_camera == "sphere" and cmd.nerf.render_fov == 60 and cmd.nerf.render_ortho_width == 2.5
    opt = options.set(opt_cmd=cmd, make_output_dir=False, verbose=False)
    assert opt.nerf.render_camera == "sphere" and float(opt.nerf.render_fov) == 60.0 and float(opt.nerf.render_ortho_width) == 2.5
    plain = options.set(opt_cmd=options.parse_arguments(["--yaml=test"]), make_output_dir=False, verbose=False)
    for key in ("render_camera", "render_fov", "render_ortho_width"):
        assert getattr(plain.nerf, key, None) is None, key


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("tag", ["tiny", "plus"])
def test_float64_pinhole_agrees_with_the_chain(name, tag):
    """the float64 restatement of the pinhole model against the bits the kernels pin (target_rays_chain): a few float32 ulps"""
    _, cfg, _, batch, _, _ = case(name)
    th, tw = sizes(name)[tag]
    intr = target_intrinsics(name, tag)
    te = batch["extrinsics"][0, -1, :3]
    center, ray = target_rays_chain(th, tw, te, intr, cfg.legacy_coord)
    cam = camera.camera_model("pinhole", th, tw, te, intr, cfg.legacy_coord)
    assert (cam.model, cam.height, cam.width, cam.legacy_coord) == (0, th, tw, int(cfg.legacy_coord))
    kinv, c2w = camera.target_ray_consts(te, intr, cfg.legacy_coord)
    assert np.array_equal(np.array(cam.kinv, np.float32), kinv.reshape(-1)) and np.array_equal(np.array(cam.c2w, np.float32), c2w.reshape(-1))
    rows = camera_rows_f64("pinhole", th, tw, kinv, c2w, cfg.legacy_coord)
    assert np.array_equal(rows[:, 0:3].astype(np.float32), center.numpy())
    # camera-space coordinates are O(1) (z = 1), the world direction a 3-term sum of them: 4 roundings of 2^-24 each
    assert np.abs(rows[:, 4:7] - ray.numpy().astype(np.float64)).max() < 4 * 2.0 ** -24 * 1.5
    assert np.all(rows[:, 3] == 0) and np.all(rows[:, 7] == 0)
    part = camera_rows_f64("pinhole", th, tw, kinv, c2w, cfg.legacy_coord, pixel_begin=3, n_pixels=tw + 2)
    assert np.array_equal(part, rows[3:3 + tw + 2])


def test_float64_models_are_what_the_header_says():
    eye = np.eye(4)[:3]
    # fisheye: 90 degrees across 9 columns, principal point = the centre pixel; the corner columns look 45 degrees off axis
    for legacy in (True, False):
        cam = camera.camera_model("fisheye", 9, 9, eye, legacy=legacy, fov_deg=90)
        kinv, c2w, _ = (np.array(a, np.float32) for a in (cam.kinv, cam.c2w, cam.lon_lat))
        rows = camera_rows_f64("fisheye", 9, 9, kinv, c2w, legacy)
        d = rows[:, 4:7].reshape(9, 9, 3)
        assert np.abs(np.linalg.norm(d, axis=-1) - 1).max() < 1e-12
        if legacy:  # integer pixel centres: pixel (4, 4) is the principal point
            assert np.allclose(d[4, 4], [0, 0, 1], atol=1e-7)
            assert np.allclose(np.degrees(np.arctan2(d[4, 8, 0], d[4, 8, 2])), 40.0, atol=1e-4)  # 4 pixels x 10 degrees
        else:
            assert np.allclose(np.degrees(np.arctan2(d[4, 8, 0], d[4, 8, 2])), 40.0, atol=1e-4) and abs(d[4, 4, 0]) < 1e-6
    # sphere: the full panorama on a legacy 5 x 9 grid has the poles in the first / last row and wraps in longitude
    cam = camera.camera_model("sphere", 5, 9, eye, legacy=True, fov_deg=360)
    ll = np.array(cam.lon_lat, np.float32)
    assert np.allclose(ll, [-np.pi, np.pi, -np.pi / 2, np.pi / 2])
    d = camera_rows_f64("sphere", 5, 9, cam.kinv, cam.c2w, True, ll)[:, 4:7].reshape(5, 9, 3)
    assert np.allclose(d[0, :, 1], -1, atol=1e-6) and np.allclose(d[4, :, 1], 1, atol=1e-6)  # y down: row 0 looks up
    assert np.allclose(d[2, 4], [0, 0, 1], atol=1e-7) and np.allclose(d[2, 6], [1, 0, 0], atol=1e-6) and np.allclose(d[2, 0], d[2, 8], atol=1e-6)
    # ortho: parallel rays, origins 2.0 world units across the frame's width
    cam = camera.camera_model("ortho", 4, 8, eye, legacy=False, ortho_width=2.0)
    rows = camera_rows_f64("ortho", 4, 8, cam.kinv, cam.c2w, False)
    assert np.allclose(rows[:, 4:7], [0, 0, 1]) and np.allclose(rows[7, 0] - rows[0, 0], 2.0 * 7 / 8) and np.allclose(rows[:, 2], 0)
    assert np.allclose(rows[0, 0:2], [-1 + 0.125, -0.5 + 0.125])


def test_ray_bundle_packs_rows():
    import torch
    o, d = torch.arange(6.0).reshape(2, 3), -torch.arange(6.0).reshape(2, 3)
    rows = camera.ray_bundle(o, d)
    assert rows.shape == (2, 8) and rows.dtype == torch.float32
    assert torch.equal(rows[:, :3], o) and torch.equal(rows[:, 4:7], d) and float(rows[:, 3].abs().max() + rows[:, 7].abs().max()) == 0
    with pytest.raises(ValueError):
        camera.ray_bundle(o, d[:1])


@pytest.mark.parametrize("name", SCENES)
def test_the_test_bundles_meet_the_precondition(name):
    """free_ray_helpers asserts it while it evaluates the oracle: here, on the CPU, for the bundles the GPU tests use"""
    for which in ("sphere", "jitter"):
        e = expected(name, which)
        n = e["rows"].shape[0]
        assert 300 <= n <= 600 and e["rgb"].shape == (n, 3) and e["rows"].dtype == np.float32
        assert -0.2 <= float(e["x_ref"].min()) and float(e["x_ref"].max()) <= 1.2
    cam, rows = sphere_window(name)
    assert np.abs(np.linalg.norm(rows[:, 4:7].astype(np.float64), axis=-1) - 1).max() < 1e-7  # unit: depth is a distance
    lens = np.linalg.norm(expected(name, "jitter")["rows"][:, 4:7], axis=-1)
    assert lens.min() < 0.85 and lens.max() > 1.2


def test_scored_evaluation_refuses_another_camera():
    from matchnerf_amd.coach import Coach
    from matchnerf_amd.edict import EasyDict
    c = Coach.__new__(Coach)
    c.opts = EasyDict(nerf=EasyDict(render_camera="fisheye"))
    with pytest.raises(ValueError, match="pinhole"):
        c.test_model()
    with pytest.raises(ValueError, match="pinhole"):
        c._require_pinhole("evaluation", EasyDict(tgt_camera=dict(model="sphere")))
    c.opts.nerf.render_camera = "pinhole"
    c._require_pinhole("evaluation")
    c._require_pinhole("evaluation", EasyDict(tgt_camera="pinhole"))
    c._require_pinhole("evaluation", EasyDict())


def test_sharded_rendering_refuses_another_camera():
    """dist.render_frame_sharded / render_views_sharded have no bundle form: refused before the encoder and any collective"""
    from matchnerf_amd import dist
    from matchnerf_amd.edict import EasyDict
    from matchnerf_amd.matchnerf import MatchNeRF

    class Model:
        opts = EasyDict(nerf=EasyDict(render_camera="fisheye", render_fov=90))
        target_camera = MatchNeRF.target_camera

        def __getattr__(self, name):
            raise AssertionError(f"nothing of the model is touched before the refusal: {name}")

    for fn, args in ((dist.render_frame_sharded, ()), (dist.render_views_sharded, ([],))):
        with pytest.raises(NotImplementedError, match="fisheye"):
            fn(Model(), EasyDict(), *args, mode="test")
        with pytest.raises(NotImplementedError, match="sphere"):
            fn(Model(), EasyDict(tgt_camera="sphere"), *args, mode="train")
