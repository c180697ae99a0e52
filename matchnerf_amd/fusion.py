"""Geometry export: depth maps rendered at several poses of one encoded scene, filtered by cross-view consistency and back-projected
into one coloured point cloud (include/mnerf.h "GEOMETRY EXPORT", matchnerf_amd/csrc/fusion.hip).

Depth-map fusion rather than a density grid: the ray transformer makes a sample's density depend on all samples of its ray, so a
point query has no meaning without a ray, whereas a depth map rendered at a pose is well-defined.  Every view is the reference once
(the MVSNet criterion, ``hip.depth_consistency``); its surviving pixels are compacted in pixel order into its own segment of one
buffer of K h w rows (``hip.point_cloud``), the K counts reach the host in ONE copy, and the segments are trimmed and joined.
Everything else stays on the device.  There is no CPU fallback.
"""
import numpy as np
import torch

from . import hip

MAX_PARTNERS = hip.MNERF_MAX_VIEWS - 1  # a launch takes the reference and up to 15 partners


def camera_centres(views):
    """[hip.View, ...] -> float64 [K, 3] camera centres in the world, -R^-1 t"""
    out = np.zeros((len(views), 3))
    for i, v in enumerate(views):
        e = np.asarray(list(v.extr), np.float64).reshape(3, 4)
        out[i] = -np.linalg.solve(e[:, :3], e[:, 3])
    return out


def partners_of(centres, ref, max_partners=MAX_PARTNERS):
    """The views ``ref`` is checked against, ascending: all others, or the ``max_partners`` nearest by camera centre (ties: the lower
    index) when there are more."""
    others = [j for j in range(len(centres)) if j != ref]
    if len(others) <= max_partners:
        return others
    dist = np.linalg.norm(centres[others] - centres[ref], axis=1)
    order = np.argsort(dist, kind="stable")[:max_partners]
    return sorted(others[i] for i in order)


def fuse(views, depths, opacities, rgbs, hw, legacy, px_tol=1.0, rel_tol=0.01, min_opacity=0.5, min_consistent=None,
         return_counts=False):
    """K views of one scene -> points [M, 8] float32 on the device, rows ``x y z d | r g b n``: the pixels of every view whose depth
    at least ``min_consistent`` other views confirm (default min(2, K - 1)), view after view and in pixel order inside a view; d is the
    fused depth, n the number of confirming views.
      views      [hip.View] * K: world->camera extr, the intr of the (h, w) grid, near_ / far_ = the valid depth range
      depths     [K, h*w] (any shape of K h w elements) float32 CUDA, camera-z depths as ``render`` returns them for pixel rays
      opacities  the same shape or None; with it the depth used is depth / opacity and pixels below ``min_opacity`` are invalid
      rgbs       [K, h*w, 3]
    ``return_counts``: -> (points, [rows of view k] * K).  One device->host copy (the K counts)."""
    h, w = int(hw[0]), int(hw[1])
    n, k_views = h * w, len(views)
    if k_views < 2:
        raise ValueError(f"fuse: {k_views} view(s); cross-view consistency needs at least 2")
    if min_consistent is None:
        min_consistent = min(2, k_views - 1)
    depths = depths.reshape(k_views, h, w)
    opacities = None if opacities is None else opacities.reshape(k_views, h, w)
    rgbs = rgbs.reshape(k_views, n, 3)
    dev = depths.device
    points = torch.empty(k_views * n, hip.POINT_FLOATS, device=dev)
    counts = torch.zeros(k_views, dtype=torch.int64, device=dev)
    workspace = torch.empty(max(hip.point_cloud_workspace_bytes(n), 16), dtype=torch.uint8, device=dev)
    out = (torch.empty(h, w, device=dev), torch.empty(h, w, dtype=torch.int32, device=dev))
    all_views = hip.view_array(views) if k_views <= hip.MNERF_MAX_VIEWS else None
    centres = None if all_views is not None else camera_centres(views)
    for k in range(k_views):
        if all_views is not None:
            arr, ref, d, o = all_views, k, depths, opacities
        else:  # the reference and its 15 nearest partners, in the views' order
            group = sorted(partners_of(centres, k) + [k])
            index = torch.as_tensor(group, device=dev)
            arr, ref = hip.view_array([views[j] for j in group]), group.index(k)
            d = depths.index_select(0, index)
            o = None if opacities is None else opacities.index_select(0, index)
        fused, cnt = hip.depth_consistency(arr, ref, d, o, legacy=legacy, px_tol=px_tol, rel_tol=rel_tol, min_opacity=min_opacity,
                                           out=out)
        hip.point_cloud(views[k], (h, w), fused, rgbs[k], cnt, min_consistent, legacy=legacy, points=points[k * n:(k + 1) * n],
                        count=counts[k:k + 1], workspace=workspace)
    rows = [int(c) for c in counts.cpu()]  # the one copy of the scene
    cloud = torch.cat([points[k * n:k * n + rows[k]] for k in range(k_views)], 0)
    return (cloud, rows) if return_counts else cloud


def write_ply(path, points):
    """points [M, >= 7] (x y z . r g b ..., colours in [0, 1]; a tensor or an array) -> a binary little-endian PLY of float xyz and
    uchar rgb vertices."""
    pts = points.detach().cpu().numpy() if torch.is_tensor(points) else np.asarray(points)
    pts = pts.reshape(-1, pts.shape[-1]) if pts.size else np.zeros((0, 8), np.float32)
    vertex = np.zeros(len(pts), dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    for i, name in enumerate(("x", "y", "z")):
        vertex[name] = pts[:, i]
    for i, name in enumerate(("red", "green", "blue")):
        vertex[name] = np.rint(np.clip(np.nan_to_num(pts[:, 4 + i]), 0.0, 1.0) * 255.0).astype(np.uint8)
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" \
             "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" % len(pts)
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(vertex.tobytes())
    return len(pts)
