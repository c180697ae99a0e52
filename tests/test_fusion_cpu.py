"""Geometry export without a GPU: the ABI additions, every argument refusal of the three entry points (all precede any HIP call),
the workspace formula, the PLY writer, the colour map's statement, the options, and self-checks of the float64 restatement that
the GPU tests compare the device with (tests/fusion_helpers.py)."""
import ctypes as C
import math

import numpy as np
import pytest

import fusion_helpers as F
from helpers import read_header
from matchnerf_amd import fusion, hip, options

NEW_EXPORTS = ("mnerf_depth_consistency", "mnerf_point_cloud_workspace_bytes", "mnerf_point_cloud", "mnerf_depth_colormap")
FAKE = 0x10000  # a non-NULL, 16-byte aligned "device" address: the calls below fail their checks or have nothing to launch
FAKE_I32 = C.cast(C.c_void_p(FAKE), C.POINTER(C.c_int32))  # the same where the header says int32_t*


def _views(k=3, h=8, w=8):
    return hip.view_array([hip.make_view(c["extr"], c["intr"], c["near"], c["far"]) for c in F.arc_cameras(k, h, w)])


def test_exports_and_abi_stay_put():
    header = read_header()
    names = [name for _, name, _ in header.prototypes]
    for name in NEW_EXPORTS:
        assert name in hip.EXPORTS and name in names, name
    lib = hip.load()
    assert lib.mnerf_abi_version() == 12 == hip.MNERF_ABI_VERSION == header.constants["MNERF_ABI_VERSION"]
    assert len(hip.STRUCTS) == 11 and lib.mnerf_struct_size(11) == -1 and lib.mnerf_struct_size(33) == -1  # no new struct
    protos = {name: params for _, name, params in header.prototypes}
    assert protos["mnerf_depth_consistency"][0] == protos["mnerf_point_cloud"][0] == "const mnerf_view*"  # poses travel as views
    assert hip.POINT_FLOATS == hip.MNERF_RAY_FLOATS == 8  # a point row has the size of a ray-bundle row


def _consistency(lib, views=None, n_views=3, ref=0, h=8, w=8, depth=FAKE, opacity=None, px=1.0, rel=0.01, min_op=0.5, fused=FAKE,
                 count=FAKE_I32):
    views = _views(max(n_views, 2), max(h, 1), max(w, 1)) if views is None else views
    return lib.mnerf_depth_consistency(views, n_views, ref, h, w, 0, depth, opacity, px, rel, min_op, fused, count, None)


def test_depth_consistency_refusals_need_no_device():
    lib = hip.load()
    for kw in (dict(ref=-1), dict(ref=3), dict(n_views=1), dict(n_views=17, views=_views(16)), dict(h=0), dict(w=0), dict(h=-3),
               dict(h=1 << 16, w=1 << 15), dict(px=0.0), dict(px=-1.0), dict(px=math.inf), dict(px=math.nan), dict(rel=0.0),
               dict(rel=math.nan), dict(rel=math.inf), dict(opacity=FAKE, min_op=math.nan)):
        assert _consistency(lib, **kw) == hip.MNERF_E_RANGE, kw
        assert b"mnerf_depth_consistency" in lib.mnerf_last_error()
    for kw in (dict(depth=None), dict(fused=None), dict(count=None)):
        assert _consistency(lib, **kw) == hip.MNERF_E_NULL, kw
    assert lib.mnerf_depth_consistency(None, 3, 0, 8, 8, 0, FAKE, None, 1.0, 0.01, 0.5, FAKE, FAKE_I32, None) == hip.MNERF_E_NULL
    singular = _views()
    singular[1].intr[0] = 0.0  # no focal length: the pixel cannot be lifted
    assert _consistency(lib, views=singular) == hip.MNERF_E_RANGE and b"singular" in lib.mnerf_last_error()
    flat = _views()
    for i in range(4):
        flat[2].extr[8 + i] = flat[2].extr[4 + i]
    assert _consistency(lib, views=flat) == hip.MNERF_E_RANGE and b"view 2" in lib.mnerf_last_error()


def _cloud(lib, view=True, h=8, w=8, depth=FAKE, rgb=FAKE, cnt=FAKE_I32, points=FAKE, capacity=64, count=FAKE, ws=FAKE):
    v = _views()[0] if view is True else view
    return lib.mnerf_point_cloud(None if v is None else C.byref(v), h, w, 0, depth, rgb, cnt, 1, points, capacity, count, ws, None)


def test_point_cloud_refusals_and_workspace():
    lib = hip.load()
    for kw in (dict(h=-1), dict(w=-1), dict(h=1 << 16, w=1 << 15), dict(capacity=-1)):
        assert _cloud(lib, **kw) == hip.MNERF_E_RANGE, kw
    for kw in (dict(view=None), dict(depth=None), dict(rgb=None), dict(count=None), dict(ws=None), dict(points=None),
               dict(cnt=None)):
        assert _cloud(lib, **kw) == hip.MNERF_E_NULL, kw
    for kw in (dict(points=FAKE + 8), dict(points=FAKE + 4), dict(ws=FAKE + 2), dict(count=FAKE + 4)):
        assert _cloud(lib, **kw) == hip.MNERF_E_ALIGN, kw
    singular = _views()[0]
    singular.intr[4] = 0.0
    assert _cloud(lib, view=singular) == hip.MNERF_E_RANGE
    # no pixel: nothing to do, no buffer touched
    assert lib.mnerf_point_cloud(None, 0, 8, 0, None, None, None, 1, None, 0, None, None, None) == hip.MNERF_OK
    assert lib.mnerf_point_cloud(None, 8, 0, 0, None, None, None, 1, None, 0, None, None, None) == hip.MNERF_OK
    # the workspace: one int32 per workgroup of 256 pixels + one per tile of 1024 workgroups, rounded up to 16 bytes
    size = lib.mnerf_point_cloud_workspace_bytes
    assert size(-1) == -1 and size(-(1 << 40)) == -1 and size(0) == 0
    assert size(1) == 16 and size(256) == 16 and size(257) == 16 and size(256 * 3) == 16 and size(256 * 3 + 1) == 32
    previous = 0
    for n in (1, 255, 256, 257, 1961, 262144, 262145, 327680, (1 << 31) - 1, 1 << 40):
        blocks = -(-n // 256)
        assert size(n) == (4 * (blocks + -(-blocks // 1024)) + 15) // 16 * 16 >= previous, n
        previous = size(n)
    assert size(1 << 40) > 1 << 32  # 64-bit in and out
    assert hip.point_cloud_workspace_bytes(327680) == size(327680)


def test_depth_colormap_refusals_need_no_device():
    lib = hip.load()
    assert lib.mnerf_depth_colormap(FAKE, -1, 0.0, 1.0, FAKE, None) == hip.MNERF_E_RANGE
    for lo, hi in ((math.nan, 1.0), (0.0, math.inf), (-math.inf, 1.0)):
        assert lib.mnerf_depth_colormap(FAKE, 4, lo, hi, FAKE, None) == hip.MNERF_E_RANGE, (lo, hi)
    assert lib.mnerf_depth_colormap(None, 4, 0.0, 1.0, FAKE, None) == hip.MNERF_E_NULL
    assert lib.mnerf_depth_colormap(FAKE, 4, 0.0, 1.0, None, None) == hip.MNERF_E_NULL
    assert lib.mnerf_depth_colormap(None, 0, 0.0, 1.0, None, None) == hip.MNERF_OK  # n == 0 touches nothing


def test_colormap_statement():
    """the integer form of the header equals its real-valued statement at all 256 indices; end points, clamping and NaN"""
    index = np.arange(256)
    ints = np.stack([np.clip(383 - np.abs(4 * index - c), 0, 255) for c in (765, 510, 255)], -1).astype(np.uint8)
    assert np.array_equal(ints, F.jet_float(index))
    lo, hi = 2.0, 6.0
    ramp = lo + (index + 0.5) / 255.0 * (hi - lo)  # mid-points: every index once
    assert np.array_equal(F.colormap(ramp, lo, hi), ints)
    assert np.array_equal(F.colormap(ramp.astype(np.float32), lo, hi, dtype=np.float32), ints)
    assert tuple(ints[0]) == (0, 0, 128) and tuple(ints[255]) == (128, 0, 0) and tuple(ints[128]) == (130, 255, 126)
    edge = F.colormap(np.array([np.nan, 0.0, lo - 1.0, lo, hi, hi + 100.0, np.inf, -np.inf]), lo, hi)
    assert all(tuple(edge[i]) == (0, 0, 128) for i in (0, 1, 2, 3, 7))  # NaN -> 0 -> below lo: index 0
    # hi itself: in float64 255 * 4 / (4 + 1e-8) truncates to 254; in the header's float32 the denominator rounds to 4: 255
    assert tuple(edge[4]) == tuple(ints[254]) and tuple(edge[5]) == tuple(edge[6]) == tuple(ints[255])
    assert tuple(F.colormap(np.array([hi], np.float32), lo, hi, dtype=np.float32)[0]) == tuple(ints[255])


def test_ply_round_trip(tmp_path):
    rng = np.random.default_rng(5)
    pts = rng.normal(size=(37, 8)).astype(np.float32)
    pts[:, 4:7] = rng.uniform(-0.2, 1.2, (37, 3))  # colours beyond [0, 1] are clipped
    pts[3, 5] = np.nan
    path = str(tmp_path / "cloud.ply")
    assert fusion.write_ply(path, pts) == 37
    xyz, rgb = F.read_ply(path)
    assert np.array_equal(xyz, pts[:, :3])
    assert np.array_equal(rgb, np.rint(np.clip(np.nan_to_num(pts[:, 4:7]), 0, 1) * 255).astype(np.uint8))
    import torch
    assert fusion.write_ply(path, torch.from_numpy(pts[:5])) == 5 and len(F.read_ply(path)[0]) == 5
    assert fusion.write_ply(path, np.zeros((0, 8), np.float32)) == 0 and len(F.read_ply(path)[0]) == 0


def test_partner_choice():
    centres = np.array([[float(i), 0.0, 0.0] for i in range(20)])
    assert fusion.partners_of(centres[:5], 2) == [0, 1, 3, 4]
    assert fusion.partners_of(centres, 0) == list(range(1, 16))
    assert fusion.partners_of(centres, 10) == [2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 14, 15, 16, 17]  # 2 | 18: the tie goes to the lower index
    cams = F.arc_cameras(4, 8, 8)
    got = fusion.camera_centres([hip.make_view(c["extr"], c["intr"], c["near"], c["far"]) for c in cams])
    angles = np.linspace(-0.35, 0.35, 4)  # the arc: radius 2.2 in the x-z plane, a small height wobble
    assert np.allclose(got[:, 0], 2.2 * np.sin(angles), atol=1e-5) and np.allclose(got[:, 2], -2.2 * np.cos(angles), atol=1e-5)


def test_options_parse_and_default_to_none():
    opt = options.load_options("configs/test.yaml", verbose=False)
    for name in ("export_geometry", "fuse_px_tol", "fuse_rel_tol", "fuse_min_opacity", "fuse_min_views"):
        assert getattr(opt.nerf, name, None) is None and name not in opt.nerf, name
    cmd = options.parse_arguments(["--nerf.export_geometry=path", "--nerf.fuse_px_tol=0.5", "--nerf.fuse_rel_tol=0.02",
                                   "--nerf.fuse_min_opacity=0.7", "--nerf.fuse_min_views=3", "--vis_depth"])
    opt = options.override_options(opt, cmd)
    assert opt.nerf.export_geometry == "path" and opt.vis_depth is True
    assert (opt.nerf.fuse_px_tol, opt.nerf.fuse_rel_tol, opt.nerf.fuse_min_opacity, opt.nerf.fuse_min_views) == (0.5, 0.02, 0.7, 3)


@pytest.mark.parametrize("k,h,w,legacy", F.GPU_CASES)
def test_restatement_on_the_analytic_scene(k, h, w, legacy):
    """what makes the GPU comparison meaningful: few borderline pixels, a non-trivial selection, the planted outliers rejected, and
    the fp32 restatement within the cap the fused-depth gate puts on it"""
    for variant in (F.VARIANTS if k == 3 else ("plain",)):
        refs = F.reference(k, h, w, legacy, variant)
        s = F.scene(k, h, w, legacy, variant)
        need = min(2, k - 1)
        assert np.mean([r["border"].mean() for r in refs]) <= F.BORDERLINE_CAP, variant
        selected = np.mean([(r["count"] >= need).mean() for r in refs])
        assert 0.2 < selected <= 1.0, (variant, selected)
        assert (refs[0]["count"][s["outliers"]] < need).mean() >= 0.95, variant
        for r in refs:
            assert np.array_equal(r["count"][~r["border"]], r["count32"][~r["border"]])  # fp32 only differs on borderline pixels
            same = (r["count"] == r["count32"]) & (r["fused"] > 0)
            assert (np.abs(r["fused32"] - r["fused"])[same] / r["fused"][same]).max() < 1e-5
        if variant == "opacity":  # the transparent stripe of view 1 is invalid as a reference ...
            assert (refs[1]["count"][:, w // 3:w // 3 + 4] == 0).all() and (refs[1]["fused"][:, w // 3:w // 3 + 4] == 0).all()
        if variant == "invalid":  # ... and so is every planted value
            with np.errstate(invalid="ignore"):
                bad = ~(np.isfinite(s["depth"]) & (s["depth"] >= 0.5) & (s["depth"] <= 6.0))
            assert bad.sum() > 20 and all((r["count"][b] == 0).all() and (r["fused"][b] == 0).all() for r, b in zip(refs, bad))


def test_point_rows_restatement():
    k, h, w = 3, 24, 32
    s, refs = F.scene(k, h, w, False), F.reference(k, h, w, False)
    rgb = np.random.default_rng(0).random((h * w, 3)).astype(np.float32)
    idx, rows = F.point_rows(s["cams"][1], h, w, False, refs[1]["fused"].astype(np.float32), rgb, refs[1]["count"], 2)
    assert len(idx) == (refs[1]["count"] >= 2).sum() and np.all(np.diff(idx) > 0)
    inv = F.inverse_cameras(s["cams"], np.float64)[1]
    u, v, z = F.proj(inv, rows[:, :3])  # every row reprojects to its own pixel centre and depth
    assert np.abs(u - (idx % w + 0.5)).max() < 1e-9 and np.abs(v - (idx // w + 0.5)).max() < 1e-9 and np.abs(z - rows[:, 3]).max() < 1e-9
    assert np.abs(rows[:, 2]).max() < 0.7  # the points lie on the plane z = 0 or on the box in front of it
