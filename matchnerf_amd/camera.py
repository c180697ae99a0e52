"""Host-side camera algebra of the hot path (tiny 3x3 / 4x4 work, done once per target pose).

The per-ray arithmetic of the reference's misc/camera.py (get_center_and_ray 255-278,
get_3D_points_from_depth 281-286, get_coord_ref_ndc 351-379) lives inside the HIP kernels
(csrc/common.hpp); what stays on the host is what the reference also computes once per call:
the inverse intrinsics and the camera->world matrix of the target view.
"""
import numpy as np
import torch


def target_ray_consts(extr34, intr33, legacy=True):
    """-> (kinv [3,3], c2w [3,4]) float32 numpy.

    kinv: fp32 ``intr.inverse()`` (camera.py:221-222).
    c2w : legacy — inverse of the 4x4 world->cam taken in float64 then cast to float32
          (cam2world_legacy, camera.py:231-240); otherwise [R^T | -R^T t] in float32
          (Pose.invert, camera.py:36-42)."""
    extr = torch.as_tensor(extr34, dtype=torch.float32).detach().cpu().reshape(3, 4)
    intr = torch.as_tensor(intr33, dtype=torch.float32).detach().cpu().reshape(3, 3)
    kinv = intr.inverse()
    if legacy:
        sq = torch.eye(4)
        sq[:3] = extr
        c2w = sq.double().inverse()[:3].float()
    else:
        rot_inv = extr[:, :3].t()
        c2w = torch.cat([rot_inv, -(rot_inv @ extr[:, 3:])], 1)
    return kinv.numpy().copy(), c2w.contiguous().numpy().copy()


def pair_list(n_views):
    """Ordered view pairs (a<b) (gmflow.py:49, matchnerf.py:194)."""
    return [(a, b) for a in range(n_views - 1) for b in range(a + 1, n_views)]


def resize_intrinsics(K, src_hw, tgt_hw, legacy=True):
    """Intrinsics of the same field of view on another pixel grid: ``K`` [..., 3, 3] (numpy or torch) of a ``src_hw`` = (H, W)
    frame -> those of a ``tgt_hw`` = (h', w') frame, with sx = w'/W, sy = h'/H:

    non-legacy (pixel centres at +0.5, the frame spans [0, W]):      diag(sx, sy, 1) @ K
    legacy (integer pixel centres, the frame spans [-0.5, W - 0.5]):  [[sx, 0, 0.5 sx - 0.5], [0, sy, 0.5 sy - 0.5], [0, 0, 1]] @ K

    The product is written out row by row (the matrix has two entries per row), in K's own dtype: a host copy and a device copy of
    K give the same bits.  The identity size returns ``K`` itself."""
    (src_h, src_w), (tgt_h, tgt_w) = (int(v) for v in src_hw), (int(v) for v in tgt_hw)
    if min(src_h, src_w, tgt_h, tgt_w) < 1:
        raise ValueError(f"resize_intrinsics: frame sizes {src_hw} -> {tgt_hw}")
    if (src_h, src_w) == (tgt_h, tgt_w):
        return K
    sx, sy = tgt_w / src_w, tgt_h / src_h
    ox, oy = (0.5 * sx - 0.5, 0.5 * sy - 0.5) if legacy else (0.0, 0.0)
    if torch.is_tensor(K):
        out = K.clone()
    else:
        K = np.asarray(K)
        out = K.copy()
        sx, sy, ox, oy = (K.dtype.type(v) for v in (sx, sy, ox, oy))
    out[..., 0, :] = K[..., 0, :] * sx
    out[..., 1, :] = K[..., 1, :] * sy
    if legacy:
        out[..., 0, :] += K[..., 2, :] * ox
        out[..., 1, :] += K[..., 2, :] * oy
    return out


# ----------------------------------------------------------------------- camera models of caller-supplied rays (include/mnerf.h)
CAMERA_MODELS = ("pinhole", "fisheye", "sphere", "ortho")  # index = mnerf_camera.model (MNERF_CAM_*)


def camera_model(name, height, width, extr34, intr33=None, legacy=True, fov_deg=None, ortho_width=None, lon_lat=None):
    """-> ``hip.Camera`` (struct mnerf_camera) of a ``height`` x ``width`` grid at the pose ``extr34`` (world -> camera, 3x4):

    "pinhole"  ``intr33`` (of this grid): the rows are the pixel rays of the render path, bit for bit;
    "fisheye"  equidistant, the angle off the axis grows linearly with the distance from the principal point: ``fov_deg`` across the
               frame's width around its centre, or ``intr33`` (focal length = pixels per radian);
    "sphere"   equirectangular window of ``fov_deg`` degrees of longitude centred on the optical axis, the latitude range in the
               grid's aspect ratio (clipped to +-90), or ``lon_lat`` = (lon0, lon1, lat0, lat1) in radians; fov_deg=360 on a 1:2 grid
               is the full panorama;
    "ortho"    parallel rays along the optical axis through a plane at the camera centre, ``ortho_width`` world units across the
               frame's width (square pixels).
    Pixel centres follow ``legacy`` (integer coordinates / + 0.5), c2w is that of ``target_ray_consts``."""
    from . import hip
    if name not in CAMERA_MODELS:
        raise ValueError(f"camera model {name!r}: one of {CAMERA_MODELS}")
    height, width = int(height), int(width)
    if min(height, width) < 1:
        raise ValueError(f"camera_model: grid {height}x{width}")
    cam = hip.Camera()
    cam.model, cam.height, cam.width, cam.legacy_coord = CAMERA_MODELS.index(name), height, width, int(bool(legacy))
    cx, cy = ((width - 1) / 2.0, (height - 1) / 2.0) if legacy else (width / 2.0, height / 2.0)  # the frame's centre in pixel coordinates
    if name == "pinhole" or (name == "fisheye" and fov_deg is None):
        if intr33 is None:
            raise ValueError(f"camera_model({name!r}): needs intr33" + (" or fov_deg" if name == "fisheye" else ""))
        intr = intr33
    elif name == "fisheye":
        f = width / np.deg2rad(float(fov_deg))  # pixels per radian
        intr = [[f, 0, cx], [0, f, cy], [0, 0, 1]]
    elif name == "ortho":
        if ortho_width is None or float(ortho_width) <= 0:
            raise ValueError("camera_model('ortho'): needs ortho_width > 0 (world units across the frame)")
        f = width / float(ortho_width)  # pixels per world unit
        intr = [[f, 0, cx], [0, f, cy], [0, 0, 1]]
    else:
        intr = np.eye(3)
    kinv, c2w = target_ray_consts(extr34, np.asarray(intr, np.float32), legacy)
    hip._fill(cam.kinv, kinv)
    hip._fill(cam.c2w, c2w)
    if name == "sphere":
        if lon_lat is None:
            if fov_deg is None:
                raise ValueError("camera_model('sphere'): needs fov_deg or lon_lat")
            half_lon = np.deg2rad(float(fov_deg)) / 2
            half_lat = min(half_lon * (height / width), np.pi / 2)
            lon_lat = (-half_lon, half_lon, -half_lat, half_lat)
        hip._fill(cam.lon_lat, lon_lat)
    return cam


def ray_bundle(origins, dirs):
    """[N,3] world origins + [N,3] un-normalised world directions (tensors on the device) -> the ray bundle [N, 8] fp32 the
    free-ray entry points take: ox oy oz 0 | dx dy dz 0 (32-byte rows; a fresh tensor, so 16-byte aligned)."""
    if origins.shape != dirs.shape or origins.dim() != 2 or origins.shape[1] != 3:
        raise ValueError(f"ray_bundle: origins {tuple(origins.shape)} and dirs {tuple(dirs.shape)} must both be [N, 3]")
    out = torch.zeros(origins.shape[0], 8, dtype=torch.float32, device=origins.device)
    out[:, 0:3] = origins
    out[:, 4:7] = dirs
    return out
