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
