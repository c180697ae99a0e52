"""Shared by the free-ray tests (caller-supplied rays, include/mnerf.h): the four camera models restated in float64 numpy, the CPU
oracle's building blocks composed for a ray BUNDLE (rows ox oy oz 0 | dx dy dz 0 instead of a pixel grid), and the test bundles.

Test bundles are data: the same float32 rows go to the oracle and to the device.  The oracle composition is O.depth_samples,
pts = o + d t elementwise in float32, O.cost_volume_cond, the projection into view 0 through
target_grid_helpers.project_to_view_chain (host-independent bits, see its docstring), O.decoder and O.composite.

PRECONDITION on a bundle, asserted here from oracle quantities (a condition on the inputs, not a skip): every sample lies in front
of every source camera, q_z >= near_v / 2, and its view-0 coordinates lie in [-0.2, 1.2] - the argument of the positional encoding
then stays below the 2000 for which csrc/common.hpp documents its sine (1.2 x 2^9 x pi = 1930).  The windows below are chosen so
that the goldens satisfy it; a bundle that does not is shrunk, the bounds are not."""
import numpy as np
import torch
import torch.nn.functional as F

from helpers import split_poses
from oracle import matchnerf_oracle as O
from target_grid_helpers import case, project_to_view_chain

MODELS = ("pinhole", "fisheye", "sphere", "ortho")  # index = MNERF_CAM_*


# ------------------------------------------------------------------------------------------------ camera models, float64
def camera_rows_f64(model, height, width, kinv, c2w, legacy, lon_lat=None, pixel_begin=0, n_pixels=None):
    """include/mnerf.h "Camera models" restated in float64 on the camera's float32 constants -> rows [n, 8] float64.  Pinhole in
    float64 is the mathematical camera, not make_ray's bits (target_grid_helpers.target_rays_chain has those)."""
    kinv = np.asarray(kinv, np.float32).reshape(3, 3).astype(np.float64)
    c2w = np.asarray(c2w, np.float32).reshape(3, 4).astype(np.float64)
    n = height * width - pixel_begin if n_pixels is None else n_pixels
    pix = np.arange(pixel_begin, pixel_begin + n)
    off = 0.0 if legacy else 0.5
    x, y = (pix % width) + off, (pix // width) + off
    xn = kinv[0, 0] * x + kinv[0, 1] * y + kinv[0, 2]
    yn = kinv[1, 0] * x + kinv[1, 1] * y + kinv[1, 2]
    zn = kinv[2, 0] * x + kinv[2, 1] * y + kinv[2, 2]
    rot, centre = c2w[:, :3], c2w[:, 3]
    origin = np.broadcast_to(centre, (n, 3)).copy()
    if model == "pinhole":
        d = np.stack([xn, yn, zn], -1) @ rot.T
    elif model == "fisheye":
        theta = np.hypot(xn, yn)
        s = np.where(theta > 0, np.sin(theta) / np.where(theta > 0, theta, 1.0), 0.0)
        d = np.stack([s * xn, s * yn, np.cos(theta)], -1) @ rot.T
    elif model == "sphere":
        ll = np.asarray(lon_lat, np.float32).astype(np.float64)
        wn, hn = (max(width - 1, 1), max(height - 1, 1)) if legacy else (width, height)
        lon = ll[0] + x / wn * (ll[1] - ll[0])
        lat = ll[2] + y / hn * (ll[3] - ll[2])
        d = np.stack([np.cos(lat) * np.sin(lon), np.sin(lat), np.cos(lat) * np.cos(lon)], -1) @ rot.T
    elif model == "ortho":
        origin = np.stack([xn, yn, np.zeros(n)], -1) @ rot.T + centre
        d = np.broadcast_to(rot[:, 2] / np.linalg.norm(rot[:, 2]), (n, 3)).copy()
    else:
        raise ValueError(model)
    rows = np.zeros((n, 8))
    rows[:, 0:3], rows[:, 4:7] = origin, d
    return rows


def camera_consts(cam):
    """(kinv [3,3], c2w [3,4], lon_lat [4]) float32 numpy of a hip.Camera"""
    return (np.array(cam.kinv, np.float32).reshape(3, 3), np.array(cam.c2w, np.float32).reshape(3, 4), np.array(cam.lon_lat, np.float32))


def camera_rows_of(cam, pixel_begin=0, n_pixels=None):
    """``camera_rows_f64`` of a hip.Camera struct"""
    kinv, c2w, ll = camera_consts(cam)
    return camera_rows_f64(MODELS[cam.model], cam.height, cam.width, kinv, c2w, bool(cam.legacy_coord), ll, pixel_begin, n_pixels)


def scene_camera(name, model, height, width, **kw):
    """the camera ``model`` on a ``height`` x ``width`` grid at the golden's target pose (its intrinsics for pinhole)"""
    from matchnerf_amd import camera
    _, cfg, _, batch, _, _ = case(name)
    return camera.camera_model(model, height, width, batch["extrinsics"][0, -1, :3], kw.pop("intr", batch["intrinsics"][0, -1]),
                               cfg.legacy_coord, **kw)


# ------------------------------------------------------------------------------------------------ the oracle over a bundle
def check_precondition(pts, se, si, sn, x_ref):
    """the module docstring's PRECONDITION, from oracle quantities"""
    for v in range(se.shape[0]):
        qz = (torch.cat([pts, torch.ones_like(pts[..., :1])], -1) @ se[v].t())[..., 2] * si[v][2, 2]
        assert float(qz.min()) >= float(sn[v, 0]) / 2, f"a sample lies behind / too close to source view {v}: q_z {float(qz.min()):.3f}"
    assert -0.2 <= float(x_ref.min()) and float(x_ref.max()) <= 1.2, \
        f"view-0 coordinates {float(x_ref.min()):.3f} .. {float(x_ref.max()):.3f} outside [-0.2, 1.2]: shrink the window"


def oracle_bundle(name, rows, near_far=None, setbg_opaque=None, chunk=1024):
    """The oracle's stages for the bundle ``rows`` ([N,8] float32, numpy or tensor) seen from the sources of golden ``name``:
    dict(rgb [N,3], depth [N,1], opacity [N,1], cond, x_ref, dir_ref, rgb_samples, sigma, depth_samples, ray_len)."""
    g, cfg, sd, batch, _, pair_feats = case(name)
    _, _, tn, se, si, sn = split_poses(batch)
    rows = torch.as_tensor(np.asarray(rows, np.float32))
    assert rows.dtype == torch.float32 and rows.shape[1] == 8
    near, far = (tn[0], tn[1]) if near_far is None else (torch.tensor(near_far[0]), torch.tensor(near_far[1]))
    setbg = g["meta"]["setbg_opaque"] if setbg_opaque is None else setbg_opaque
    v = cfg.n_src_views
    src_images = batch["images"][0, :v]
    height, width = src_images.shape[-2:]
    plain = O.project_to_view
    O.project_to_view = project_to_view_chain  # (cost_volume_cond reads the module attribute)
    parts = []
    try:
        with torch.no_grad():
            for c in range(0, rows.shape[0], chunk):
                o, r = rows[c:c + chunk, 0:3], rows[c:c + chunk, 4:7]
                d = O.depth_samples(cfg, near, far, r.shape[0])
                pts = o[:, None] + r[:, None] * d[..., None]  # float32, multiply and add rounded separately
                cond, mask = O.cost_volume_cond(cfg, pts, se, si, sn, src_images, pair_feats, height, width)
                x_ref = project_to_view_chain(pts, se[0], si[0], width, height, sn[0, 0], sn[0, 1])
                check_precondition(pts, se, si, sn, x_ref)
                dir_ref = F.normalize(r, dim=-1) @ se[0][:, :3].t()
                rgb_s, sigma = O.decoder(cfg, sd, x_ref, dir_ref, cond, mask)
                rgb, depth, opacity, _ = O.composite(cfg, r, rgb_s, sigma, d, setbg)
                parts.append(dict(rgb=rgb, depth=depth, opacity=opacity, cond=cond, x_ref=x_ref, dir_ref=dir_ref, rgb_samples=rgb_s,
                                  sigma=sigma, depth_samples=d, ray_len=r.double().norm(dim=-1)))
    finally:
        O.project_to_view = plain
    return {k: torch.cat([p[k] for p in parts], 0) for k in parts[0]}


# ------------------------------------------------------------------------------------------------ the test bundles
SPHERE_HW = (16, 24)       # 384 rays
# half-widths in longitude / latitude around the target pose's optical axis.  Shrunk from +-20 x +-15 degrees (view-0 coordinates
# -0.47 .. 1.53) and +-14 x +-10 (1.203 on c1_default) until the oracle alone meets the precondition on both scenes: -0.05 .. 1.12,
# so the window still reaches outside the source frames (border clamp, visibility masks 0).
SPHERE_WINDOW_DEG = (12.0, 9.0)


def sphere_window(name, hw=SPHERE_HW, half_deg=SPHERE_WINDOW_DEG):
    """-> (hip.Camera of the window, rows [N,8] float32: the float64 restatement rounded once - unit directions)"""
    lon, lat = np.deg2rad(half_deg[0]), np.deg2rad(half_deg[1])
    cam = scene_camera(name, "sphere", hw[0], hw[1], lon_lat=(-lon, lon, -lat, lat))
    return cam, camera_rows_of(cam).astype(np.float32)


def jittered_bundle(name, n=331, seed=5):
    """rays that no camera model produces: origins scattered around the target camera's centre (a thin-lens aperture of 2 % of the
    near distance), directions towards random points of the window at mid depth, lengths between 0.8 and 1.25 (NOT unit: the
    compositing's |d| and the decoder's normalisation are exercised).  -> rows [n,8] float32"""
    _, cfg, _, batch, _, _ = case(name)
    cam, win = sphere_window(name)
    rng = np.random.default_rng(seed)
    near, far = (float(v) for v in batch["near_fars"][0, -1])
    pick = rng.integers(0, win.shape[0], n)
    focus = win[pick, 0:3].astype(np.float64) + win[pick, 4:7].astype(np.float64) * (0.5 * (near + far))
    origin = win[pick, 0:3].astype(np.float64) + rng.normal(size=(n, 3)) * (0.02 * near)
    d = focus - origin
    d = d / np.linalg.norm(d, axis=-1, keepdims=True) * rng.uniform(0.8, 1.25, (n, 1))
    rows = np.zeros((n, 8), np.float32)
    rows[:, 0:3], rows[:, 4:7] = origin, d
    return rows


_EXPECTED = {}


def expected(name, which):
    """the oracle's stages of bundle ``which`` ("sphere" | "jitter") of scene ``name``: computed once, shared, never modified.
    The jittered bundle samples t in [near / 0.8, far / 1.25], so that with lengths in [0.8, 1.25] every sample's distance stays in
    the target's [near, far]."""
    if (name, which) not in _EXPECTED:
        _, _, _, batch, _, _ = case(name)
        near, far = (float(v) for v in batch["near_fars"][0, -1])
        if which == "sphere":
            rows, nf = sphere_window(name)[1], (near, far)
        else:
            rows, nf = jittered_bundle(name), (near / 0.8, far / 1.25)
        out = oracle_bundle(name, rows, near_far=nf)
        out["rows"], out["near_far"] = rows, nf
        _EXPECTED[name, which] = out
    return _EXPECTED[name, which]
