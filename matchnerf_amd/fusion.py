"""Geometry export: depth maps rendered at several poses of one encoded scene, filtered by cross-view consistency and back-projected
into one coloured point cloud (include/mnerf.h "GEOMETRY EXPORT", matchnerf_amd/csrc/fusion.hip).

Depth-map fusion rather than a density grid: the ray transformer makes a sample's density depend on all samples of its ray, so a
point query has no meaning without a ray, whereas a depth map rendered at a pose is well-defined.  Every view is the reference once
(the MVSNet criterion, ``hip.depth_consistency``); its surviving pixels are compacted in pixel order into its own segment of one
buffer of K h w rows (``hip.point_cloud``), the K counts reach the host in ONE copy, and the segments are trimmed and joined.
Everything else stays on the device.  There is no CPU fallback.

``mesh`` turns the same maps into a surface (include/mnerf.h "MESH EXPORT", matchnerf_amd/csrc/mesh.hip): the fused depths and their
counts are integrated into a truncated-signed-distance volume over the cloud's box, and marching tetrahedra extract a welded,
indexed, coloured triangle mesh whose vertex and face order is defined - two runs give the same bytes.

``finish`` and ``vertex_normals`` clean such a mesh - or any indexed mesh in the same layout - up on the device (include/mnerf.h "MESH
FINISHING", matchnerf_amd/csrc/mesh_finish.hip): small connected components dropped, Taubin smoothing of the positions,
area-weighted vertex normals; ``write_ply`` takes the normals.  ``decimate`` reduces it by quadric vertex clustering over a uniform
grid (``hip.mesh_decimate``): one vertex per occupied cell, the same bytes on every run.

``texture`` bakes the views' colours onto such a mesh (include/mnerf.h "MESH TEXTURE", matchnerf_amd/csrc/mesh_texture.hip): a
per-triangle atlas whose layout is a function of the triangle count, filled from every view that sees a texel's surface point;
``write_obj`` writes the result with its material and image.

``render_mesh`` looks at such a mesh (include/mnerf.h "MESH RASTER", matchnerf_amd/csrc/mesh_raster.hip): a deterministic rasterizer
gives, per pose, the triangle, depth and colour of every pixel.  ``mesh_report`` compares those frames with the field's own maps,
and ``texture(visibility="mesh")`` tests a texel's visibility against the mesh's depth instead of the views'.
"""
import numpy as np
import torch

from . import hip

MAX_PARTNERS = hip.MNERF_MAX_VIEWS - 1  # a launch takes the reference and up to 15 partners
MESH_GUESS_ROWS = 16  # the mesher's first buffers: vertex rows per voxel of the grid's three faces (twice as many triangles)
SPARSE_GUESS_ROWS = 256  # the sparse mesher's: vertex rows per allocated brick - four per voxel of a brick's face


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
    workspace = hip.export_workspace("point_cloud", None, hip.point_cloud_workspace_bytes(n), dev)
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


def _auto_bounds(views, fused, counts, rgbs, hw, legacy, min_consistent):
    """The axis-aligned box of the selected pixels' points -> float64 [2, 3] on the host (the ONE copy before the mesh): the K point
    clouds of ``fuse`` in one buffer, a masked min / max over it on the device."""
    h, w = hw
    n, k_views = h * w, len(views)
    dev = fused.device
    points = torch.empty(k_views * n, hip.POINT_FLOATS, device=dev)
    rows = torch.zeros(k_views, dtype=torch.int64, device=dev)
    workspace = hip.export_workspace("point_cloud", None, hip.point_cloud_workspace_bytes(n), dev)
    for k in range(k_views):
        hip.point_cloud(views[k], (h, w), fused[k], rgbs[k], counts[k], min_consistent, legacy=legacy, points=points[k * n:(k + 1) * n],
                        count=rows[k:k + 1], workspace=workspace)
    written = torch.arange(n, device=dev)[None, :] < rows[:, None]
    xyz = points.view(k_views, n, hip.POINT_FLOATS)[..., :3]
    inf = torch.full((), float("inf"), device=dev)
    lo = torch.where(written[..., None], xyz, inf).amin((0, 1))
    hi = torch.where(written[..., None], xyz, -inf).amax((0, 1))
    box = torch.stack([lo, hi]).double().cpu().numpy()
    if not np.isfinite(box).all():
        raise ValueError("mesh: no pixel survives the selection, so there is no box to mesh; pass bounds or loosen the thresholds")
    return box


def _texture_block(what, block, power):
    """the block size and the weight exponent of a texture, checked before anything is launched; block 0 = no texture"""
    if int(block) != block or not (int(block) == 0 or hip.TEXTURE_MIN_BLOCK <= int(block) <= hip.TEXTURE_MAX_BLOCK):
        raise ValueError(f"{what}: a texture block of {block!r}; it must be an integer in {hip.TEXTURE_MIN_BLOCK}.."
                         f"{hip.TEXTURE_MAX_BLOCK} (0: no texture)")
    if int(power) != power or not 0 <= int(power) <= hip.TEXTURE_MAX_POWER:
        raise ValueError(f"{what}: a texture power of {power!r}; it must be an integer in 0..{hip.TEXTURE_MAX_POWER}")
    return int(block), int(power)


def _visibility(what, visibility):
    """the depth a texture's visibility test reads, checked before anything is launched"""
    if visibility not in ("views", "mesh"):
        raise ValueError(f"{what}: a texture visibility of {visibility!r}; it is 'views' or 'mesh'")
    return visibility


def _consistent_maps(views, depths, opacities, legacy, px_tol, rel_tol, min_opacity):
    """``hip.depth_consistency`` with every view as the reference once -> (fused [K, h, w] float32, counts [K, h, w] int32): what the
    integrator and the texture read instead of the raw maps.  Beyond 16 views a reference is checked against its 15 nearest partners."""
    k_views, h, w = depths.shape
    dev = depths.device
    fused = torch.empty(k_views, h, w, device=dev)
    counts = torch.empty(k_views, h, w, dtype=torch.int32, device=dev)
    all_views = hip.view_array(views) if k_views <= hip.MNERF_MAX_VIEWS else None
    centres = None if all_views is not None else camera_centres(views)
    for k in range(k_views):
        if all_views is not None:
            arr, ref, d, o = all_views, k, depths, opacities
        else:
            group = sorted(partners_of(centres, k) + [k])
            index = torch.as_tensor(group, device=dev)
            arr, ref = hip.view_array([views[j] for j in group]), group.index(k)
            d = depths.index_select(0, index)
            o = None if opacities is None else opacities.index_select(0, index)
        hip.depth_consistency(arr, ref, d, o, legacy=legacy, px_tol=px_tol, rel_tol=rel_tol, min_opacity=min_opacity,
                              out=(fused[k], counts[k]))
    return fused, counts


def _bake(vertices, faces, views, maps, map_opacity, counts, min_consistent, rgbs, legacy, min_opacity, block, vis_rel_tol, power, best):
    """the launches of a texture: uv, one accumulate per group of 16 views on one zeroed buffer, resolve in place -> (uv, atlas)"""
    vertices, faces = vertices.contiguous(), faces.contiguous()
    n_faces, dev = faces.shape[0], faces.device
    width, height = hip.mesh_texture_atlas(n_faces, block)
    uv = hip.mesh_texture_uv(n_faces, block, device=dev)
    atlas = torch.zeros(height, width, hip.ATLAS_FLOATS, device=dev)
    for first in range(0, len(views), hip.MNERF_MAX_VIEWS):
        group = slice(first, min(first + hip.MNERF_MAX_VIEWS, len(views)))
        hip.mesh_texture_accumulate(vertices, faces, block, views[group], maps[group], rgbs[group], atlas,
                                    opacity=None if map_opacity is None else map_opacity[group],
                                    n_consistent=None if counts is None else counts[group], min_consistent=min_consistent, legacy=legacy,
                                    min_opacity=min_opacity, vis_rel_tol=vis_rel_tol, power=power, best=best)
    return uv, hip.mesh_texture_resolve(vertices, faces, block, atlas, best=best, out=atlas)


def texture(vertices, faces, views, depths, opacities, rgbs, hw, legacy, *, block=8, consistency=True, px_tol=1.0, rel_tol=0.01,
            min_opacity=0.5, min_consistent=None, vis_rel_tol=0.02, power=2, best=False, visibility="views"):
    """Bake a texture atlas for an indexed mesh from K views of its scene (include/mnerf.h "MESH TEXTURE") -> (uv [T, 3, 2] float32: the
    texture coordinates of every triangle's corners, origin top-left; atlas [H, W, 4] float32 ``r g b a``) on the device.  Every
    triangle owns a right-triangle patch of a ``block`` x ``block`` square it shares with one other triangle, so the atlas's size is a
    function of T and ``block`` alone and costs no copy.  A texel takes the frames' colours at its surface point from every view that
    faces it and SEES it - whose depth map agrees with the point's camera-z within ``vis_rel_tol`` - weighted by cos^``power`` of the
    angle between the view and the normal (``best``: the single view of the largest weight); where no view sees the surface it falls
    back to the triangle's vertex colours, with a = 0.  The maps are selected as in ``mesh`` (``consistency``, ``px_tol``, ``rel_tol``,
    ``min_opacity``, ``min_consistent``); views beyond 16 are accumulated in groups of 16, in order.  No device->host copy; the same
    bytes on every run.
      visibility    "views" (the default): as above.  "mesh": the depth a texel is tested against is the MESH's own, rasterized at
                    every view (``mesh_depths``), so a surface that decimation or smoothing moved away from the views' depth maps
                    still takes their colours; the maps' selection (``consistency`` ...) then plays no part and nothing of it is
                    launched"""
    h, w = int(hw[0]), int(hw[1])
    n, k_views = h * w, len(views)
    block, power = _texture_block("texture", block, power)
    visibility = _visibility("texture", visibility)
    if block == 0:
        raise ValueError("texture: a block of 0")
    if visibility == "mesh":
        if k_views < 1:
            raise ValueError("texture: no view")
        mesh_views, maps = mesh_depths(vertices, faces, views, (h, w), legacy)
        return _bake(vertices, faces, mesh_views, maps, None, None, 0, rgbs.reshape(k_views, n, 3), legacy, min_opacity, block, vis_rel_tol,
                     power, best)
    if k_views < 1 or (consistency and k_views < 2):
        raise ValueError(f"texture: {k_views} view(s); cross-view consistency needs at least 2")
    if min_consistent is None:
        min_consistent = min(2, k_views - 1)
    depths = depths.reshape(k_views, h, w)
    opacities = None if opacities is None else opacities.reshape(k_views, h, w)
    rgbs = rgbs.reshape(k_views, n, 3)
    if consistency:
        maps, counts = _consistent_maps(views, depths, opacities, legacy, px_tol, rel_tol, min_opacity)
        map_opacity = None
    else:
        maps, map_opacity, counts, min_consistent = depths, opacities, None, 0
    return _bake(vertices, faces, views, maps, map_opacity, counts, min_consistent, rgbs, legacy, min_opacity, block, vis_rel_tol, power,
                 best)


def mesh(views, depths, opacities, rgbs, hw, legacy, *, bounds=None, resolution=256, voxel=None, trunc=None, min_weight=None,
         consistency=True, px_tol=1.0, rel_tol=0.01, min_opacity=0.5, min_consistent=None, min_component=0,
         min_component_fraction=0.0, smooth=0, smooth_lambda=0.5, smooth_mu=-0.53, decimate=0.0, texture=0, texture_vis_rel_tol=0.02,
         texture_power=2, texture_best=False, texture_rgbs=None, sparse=False, texture_visibility="views"):
    """K views of one scene -> (vertices [V, 8] float32 rows ``x y z w | r g b 0``, faces [T, 3] int32) on the device: the depth maps
    fused into a truncated-signed-distance volume (``hip.tsdf_integrate``) and its zero surface extracted by marching tetrahedra
    (``hip.tsdf_mesh``: welded vertices, vertices and faces in a defined order, the same bytes on every run).  Arguments as ``fuse``.
      consistency   True: ``hip.depth_consistency`` per view as in ``fuse``; the integrator takes the fused depth and reads only
                    texels that ``min_consistent`` other views confirm.  False: the maps as they are (depth / opacity, ``min_opacity``)
      bounds        ((x0, y0, z0), (x1, y1, z1)), used as given; None: the box of the selected pixels' points, padded by ``trunc``
      voxel         the voxel side; default: the longest side of the (unpadded) box / ``resolution``
      trunc         the truncation distance in world units; default 4 voxels
      min_weight    views that must have updated a lattice point for it to take part; default min(2, K - 1), at least 1
    Views beyond 16 are integrated in groups of 16, in order.  Device->host copies: the box (with ``bounds=None`` only) before the
    mesh launch and the two counts after it.  The vertex and face buffers are sized from a first guess (a few rows per voxel of the
    grid's three faces); when the counts exceed it the mesher is RUN AGAIN ONCE with exact sizes - no further copy.
      min_component, min_component_fraction, smooth, smooth_lambda, smooth_mu    ``finish`` applied to the result (one more copy
                    when a component threshold is set)
      decimate      > 0: the finished mesh is decimated (``decimate`` below) with cells of ``decimate`` VOXELS on a grid aligned with the
                    volume - the same origin, ceil(n / decimate) cells per axis - so no box is copied; one more copy, of the counts
      texture       B > 0: -> (vertices, faces, uv, atlas), the FINISHED mesh textured (``texture`` below) with blocks of B texels from
                    the maps this call selected - the fused depths and counts are computed once - and ``texture_vis_rel_tol``,
                    ``texture_power``, ``texture_best``; ``texture_rgbs`` [K, h*w, 3]: colours to bake instead of ``rgbs`` (the vertex
                    colours stay those of ``rgbs``).  No further copy.  0: nothing is launched and the pair is returned
      texture_visibility   "views", or "mesh": the texels' visibility is tested against the finished mesh rasterized at every view
                    (``texture`` below) - what a decimated mesh wants
      sparse        True: the volume is stored in bricks of 8^3 voxels, only where a view saw a surface within ``trunc``
                    (include/mnerf.h "SPARSE TSDF VOLUME": ``hip.tsdf_bricks_mark``, ``tsdf_bricks_table``, ``tsdf_integrate_sparse``,
                    ``tsdf_mesh_sparse``), so memory follows the surface and grids the dense path refuses can be meshed.  The mesh is
                    the dense one bit for bit - the same vertex rows and triangles - in another order: bricks ascending, then the
                    in-brick index.  One more copy (the brick count); the first guess is a few hundred rows per brick.  ``decimate``
                    keeps the grid aligned with the virtual volume and is refused, before the volume is allocated, when that grid
                    has more cells than ``hip.mesh_decimate`` takes"""
    h, w = int(hw[0]), int(hw[1])
    n, k_views = h * w, len(views)
    decimate = _decimate_cell("mesh", decimate)
    sparse = _sparse_flag("mesh", sparse)
    texture, texture_power = _texture_block("mesh", texture, texture_power)
    texture_visibility = _visibility("mesh", texture_visibility)
    if k_views < 1 or (consistency and k_views < 2):
        raise ValueError(f"mesh: {k_views} view(s); cross-view consistency needs at least 2")
    if min_consistent is None:
        min_consistent = min(2, k_views - 1)
    if min_weight is None:
        min_weight = max(1, min(2, k_views - 1))
    depths = depths.reshape(k_views, h, w)
    opacities = None if opacities is None else opacities.reshape(k_views, h, w)
    rgbs = rgbs.reshape(k_views, n, 3)
    dev = depths.device
    if consistency:
        fused, counts = _consistent_maps(views, depths, opacities, legacy, px_tol, rel_tol, min_opacity)
        maps, map_opacity = fused, None
    else:
        maps, map_opacity, counts, min_consistent = depths, opacities, None, 0
    if bounds is None:
        if consistency:
            box = _auto_bounds(views, fused, counts, rgbs, (h, w), legacy, min_consistent)
        else:  # the selection of the integrator, but for the near / far range
            z = depths if opacities is None else torch.where(opacities >= min_opacity, depths / opacities, torch.zeros_like(depths))
            box = _auto_bounds(views, z.contiguous(), torch.zeros(k_views, h, w, dtype=torch.int32, device=dev), rgbs, (h, w), legacy, 0)
    else:
        box = np.asarray(bounds, np.float64).reshape(2, 3)
        if not (np.isfinite(box).all() and (box[1] >= box[0]).all()):
            raise ValueError(f"mesh: bounds {bounds!r} are no box")
    side = float((box[1] - box[0]).max())
    if voxel is None:
        voxel = side / int(resolution)
    voxel = float(voxel)
    if not (np.isfinite(voxel) and voxel > 0):
        raise ValueError(f"mesh: voxel={voxel}; the box {box.tolist()} has no extent")
    trunc = 4.0 * voxel if trunc is None else float(trunc)
    if bounds is None:
        box = np.stack([box[0] - trunc, box[1] + trunc])
    dims = tuple(max(1, int(np.ceil((box[1, a] - box[0, a]) / voxel - 1e-9))) for a in range(3))
    origin = tuple(float(x) for x in box[0])
    if sparse and decimate > 0:
        _decimate_grid_fits("mesh", dims, decimate)
    groups = []  # the integrator's arguments per group of 16 views
    for first in range(0, k_views, hip.MNERF_MAX_VIEWS):
        group = slice(first, min(first + hip.MNERF_MAX_VIEWS, k_views))
        groups.append((views[group], maps[group], rgbs[group],
                       dict(opacity=None if map_opacity is None else map_opacity[group],
                            n_consistent=None if counts is None else counts[group], min_consistent=min_consistent, legacy=legacy,
                            min_opacity=min_opacity)))
    vertices, faces = (_sparse_volume_mesh if sparse else _dense_volume_mesh)(groups, origin, voxel, dims, trunc, min_weight, dev)
    result = finish(vertices, faces, min_component=min_component, min_component_fraction=min_component_fraction,
                    smooth=smooth, smooth_lambda=smooth_lambda, smooth_mu=smooth_mu, decimate_cell=decimate * voxel, decimate_origin=origin,
                    decimate_dims=tuple(int(np.ceil(d / decimate)) for d in dims) if decimate > 0 else None)
    if texture == 0:
        return result
    colours = rgbs if texture_rgbs is None else texture_rgbs.reshape(k_views, n, 3)
    if texture_visibility == "mesh":
        mesh_views, mesh_maps = mesh_depths(*result, views, (h, w), legacy)
        return result + _bake(*result, mesh_views, mesh_maps, None, None, 0, colours, legacy, min_opacity, texture, texture_vis_rel_tol,
                              texture_power, texture_best)
    return result + _bake(*result, views, maps, map_opacity, counts, min_consistent, colours, legacy, min_opacity, texture,
                          texture_vis_rel_tol, texture_power, texture_best)


def _run_mesher(run, guess, dev):
    """``run(vertices, faces, counts)`` = one run of a mesher on buffers of a first guess of ``guess`` vertex rows (twice as many
    triangles); the ONE copy of the two counts; a second run with exact sizes when they exceed the guess -> (vertices, faces)"""
    vertices = torch.empty(guess, hip.VERTEX_FLOATS, device=dev)
    faces = torch.empty(2 * guess, 3, dtype=torch.int32, device=dev)
    _, _, totals = run(vertices, faces, None)
    n_vertices, n_faces = (int(c) for c in totals.cpu())  # the one copy after the launch
    if n_vertices > vertices.shape[0] or n_faces > faces.shape[0]:
        vertices = torch.empty(n_vertices, hip.VERTEX_FLOATS, device=dev)
        faces = torch.empty(n_faces, 3, dtype=torch.int32, device=dev)
        run(vertices, faces, totals)
    return vertices[:n_vertices], faces[:n_faces]


def _dense_volume_mesh(groups, origin, voxel, dims, trunc, min_weight, dev):
    """the dense volume of ``mesh``: integrate every group, mesh -> (vertices, faces)"""
    need = hip.tsdf_mesh_workspace_bytes(dims)
    if need < 0:
        raise ValueError(f"mesh: a grid of {dims} voxels is too large; raise voxel or lower resolution, or pass sparse=True")
    nx, ny, nz = dims
    sums = torch.zeros(nz, ny, nx, 4, device=dev)
    weight = torch.zeros(nz, ny, nx, device=dev)
    for group_views, group_maps, group_rgbs, args in groups:
        hip.tsdf_integrate(group_views, group_maps, group_rgbs, origin, voxel, dims, trunc, sums, weight, **args)
    workspace = hip.export_workspace("tsdf_mesh", None, need, dev)
    guess = min(7 * nx * ny * nz, max(1024, MESH_GUESS_ROWS * (nx * ny + ny * nz + nz * nx)))
    return _run_mesher(lambda vertices, faces, totals: hip.tsdf_mesh(sums, weight, origin, voxel, dims, min_weight, vertices, faces,
                                                                      counts=totals, workspace=workspace), guess, dev)


def _sparse_volume_mesh(groups, origin, voxel, dims, trunc, min_weight, dev):
    """the brick-sparse volume of ``mesh(sparse=True)``: mark the bricks every group of views can put a surface in, build the table,
    copy the brick count (the ONE copy the dense path does not make), allocate, integrate, mesh -> (vertices, faces)"""
    bdims = hip.brick_dims(dims)
    if hip.tsdf_bricks_table_workspace_bytes(bdims) < 0:
        raise ValueError(f"mesh: a grid of {dims} voxels has 2^31 bricks or more; raise voxel or lower resolution")
    marks = torch.zeros(bdims[2], bdims[1], bdims[0], dtype=torch.uint8, device=dev)
    for group_views, group_maps, _, args in groups:
        hip.tsdf_bricks_mark(group_views, group_maps, origin, voxel, dims, trunc, marks, **args)
    table, bricks, count = hip.tsdf_bricks_table(marks, bdims)
    n_bricks = int(count.cpu())  # the copy
    if n_bricks > hip.MAX_BRICKS:
        raise ValueError(f"mesh: the surface touches {n_bricks} bricks of {hip.TSDF_BRICK}^3 voxels, more than the {hip.MAX_BRICKS} the "
                         f"sparse mesher takes; raise voxel or lower resolution")
    if n_bricks == 0:
        return torch.empty(0, hip.VERTEX_FLOATS, device=dev), torch.empty(0, 3, dtype=torch.int32, device=dev)
    sums = torch.zeros(n_bricks, hip.BRICK_POINTS, 4, device=dev)
    weight = torch.zeros(n_bricks, hip.BRICK_POINTS, device=dev)
    for group_views, group_maps, group_rgbs, args in groups:
        hip.tsdf_integrate_sparse(group_views, group_maps, group_rgbs, origin, voxel, dims, trunc, bricks, n_bricks, sums, weight, **args)
    workspace = hip.export_workspace("tsdf_mesh_sparse", None, hip.tsdf_mesh_sparse_workspace_bytes(n_bricks, bdims), dev)
    guess = min(7 * hip.BRICK_POINTS * n_bricks, max(1024, SPARSE_GUESS_ROWS * n_bricks))
    return _run_mesher(lambda vertices, faces, totals: hip.tsdf_mesh_sparse(sums, weight, table, bricks, n_bricks, origin, voxel, dims,
                                                                             min_weight, vertices, faces, counts=totals,
                                                                             workspace=workspace), guess, dev)


def _decimate_grid_fits(what, dims, cell):
    """refuse a decimation grid of ceil(n / cell) cells per axis that ``hip.mesh_decimate`` does not take, naming the smallest whole
    number of voxels per cell that fits; host arithmetic only"""
    cells = lambda k: tuple(int(np.ceil(d / k)) for d in dims)
    fits = lambda g: g[0] * g[1] < 2 ** 31 and g[0] * g[1] * g[2] < 2 ** 31
    if fits(cells(cell)):
        return
    k = max(1, int(np.ceil(cell)))
    while not fits(cells(k)):
        k += 1
    raise ValueError(f"{what}: decimate={cell:g} lays {cells(cell)} cells over the grid of {dims} voxels, more than the decimation takes; "
                     f"the smallest decimate that fits is {k}")


def _sparse_flag(what, flag):
    """the sparse switch of a mesh, checked before anything is launched: a bool (or 0 / 1), nothing else"""
    if not isinstance(flag, (bool, int, np.bool_)) or int(flag) not in (0, 1):
        raise ValueError(f"{what}: sparse={flag!r}; it is a switch: true or false")
    return bool(flag)


def _decimate_cell(what, cell):
    """the cell size of a decimation, checked before anything is launched; 0 = none"""
    cell = float(cell)
    if not (np.isfinite(cell) and cell >= 0.0):
        raise ValueError(f"{what}: a decimation cell of {cell}; it must be finite and >= 0 (0: no decimation)")
    return cell


def finish(vertices, faces, *, min_component=0, min_component_fraction=0.0, smooth=0, smooth_lambda=0.5, smooth_mu=-0.53,
           decimate_cell=0.0, decimate_origin=None, decimate_dims=None):
    """Clean an indexed mesh up on the device (include/mnerf.h "MESH FINISHING") -> (vertices [V', 8], faces [T', 3]):
      min_component, min_component_fraction   drop every connected component with fewer than ``min_component`` triangles or fewer
                    than ``min_component_fraction`` of the largest component's (the floaters next to the surface); the kept rows
                    and faces keep their order.  The two counts of the result cost ONE device->host copy
      smooth        rounds of Taubin smoothing (``smooth_lambda``, ``smooth_mu``) of the positions over the adjacency OF THE RESULT;
                    colours and weights stay, boundary vertices do not move
      decimate_cell, decimate_origin, decimate_dims   > 0: ``decimate`` of the result, applied LAST (components, smoothing, decimation)
    The same bytes on every run.  With nothing asked for the inputs are returned and nothing is launched."""
    decimate_cell = _decimate_cell("finish", decimate_cell)
    filtering = int(min_component) > 0 or float(min_component_fraction) > 0.0
    if decimate_cell > 0.0:
        vertices, faces = finish(vertices, faces, min_component=min_component, min_component_fraction=min_component_fraction, smooth=smooth,
                                 smooth_lambda=smooth_lambda, smooth_mu=smooth_mu)
        return decimate(vertices, faces, decimate_cell, decimate_origin, decimate_dims)
    if not filtering and int(smooth) == 0:
        return vertices, faces
    vertices, faces = vertices.contiguous(), faces.contiguous()
    n_vertices, n_faces = vertices.shape[0], faces.shape[0]
    workspace = hip.export_workspace("mesh_finish", None, hip.mesh_finish_workspace_bytes(n_vertices, n_faces), vertices.device)
    if filtering:
        _, keep = hip.mesh_components(faces, n_vertices, min_component, min_component_fraction, workspace=workspace)
        vertices, faces, totals = hip.mesh_compact(vertices, faces, keep, workspace=workspace)
        n_vertices, n_faces = (int(c) for c in totals.cpu())  # the one copy
        vertices, faces = vertices[:n_vertices], faces[:n_faces]
    if int(smooth) > 0 and n_vertices:
        adjacency = hip.mesh_adjacency(faces, n_vertices, workspace=workspace)
        vertices = hip.mesh_smooth(vertices, faces, adjacency, int(smooth), smooth_lambda, smooth_mu, workspace=workspace)
    return vertices, faces


def decimate(vertices, faces, cell, origin=None, dims=None):
    """Decimate an indexed mesh by quadric vertex clustering (``hip.mesh_decimate``) -> (vertices [V', 8], faces [T', 3]) on the device:
    the vertices of every cell of side ``cell`` become one vertex - where the squared distances to the planes of the cell's triangles
    are smallest, kept inside the cell; weight and colour are the cell's means - and the triangles that still join three cells are kept
    once each, in their order.  The geometric error is bounded by the cell's diagonal; the result need not be manifold (two sheets
    closer than a cell merge).
      origin, dims  the grid: its corner (x, y, z) and (gx, gy, gz) cells; vertices outside belong to the nearest border cell.  Both
                    None: the grid of the vertices' finite bounding box, which costs one device->host copy (the box)
    The two counts of the result cost one more copy; the output buffers have the input's sizes (upper bounds), so nothing is run
    twice.  The same bytes on every run."""
    cell = _decimate_cell("decimate", cell)
    if cell == 0.0:
        raise ValueError("decimate: a cell of 0")
    if (origin is None) != (dims is None):
        raise ValueError("decimate: origin and dims go together")
    vertices, faces = vertices.contiguous(), faces.contiguous()
    n_vertices = vertices.shape[0]
    if n_vertices == 0:
        return vertices, faces
    if origin is None:
        xyz = vertices[:, :3]
        finite = torch.isfinite(xyz).all(1, keepdim=True)
        inf = torch.full((), float("inf"), device=vertices.device)
        box = torch.stack([torch.where(finite, xyz, inf).amin(0), torch.where(finite, xyz, -inf).amax(0)]).double().cpu().numpy()  # the copy
        if not np.isfinite(box).all():
            raise ValueError("decimate: no vertex is finite, so there is no box to lay a grid over; pass origin and dims")
        origin = tuple(float(x) for x in box[0])
        dims = tuple(int(np.floor((box[1, a] - box[0, a]) / cell)) + 1 for a in range(3))
    origin, dims = tuple(float(x) for x in origin), tuple(int(d) for d in dims)
    if len(origin) != 3 or len(dims) != 3 or not np.isfinite(origin).all() or min(dims) < 1:
        raise ValueError(f"decimate: origin {origin!r} / dims {dims!r} are no grid")
    if hip.mesh_decimate_workspace_bytes(n_vertices, faces.shape[0], dims) < 0:
        raise ValueError(f"decimate: a grid of {dims} cells is too large; raise cell")
    adjacency = hip.mesh_adjacency(faces, n_vertices)
    vertices, faces, totals = hip.mesh_decimate(vertices, faces, adjacency, origin, cell, dims)
    n_vertices, n_faces = (int(c) for c in totals.cpu())  # the one copy
    return vertices[:n_vertices], faces[:n_faces]


def vertex_normals(vertices, faces):
    """-> [V, 4] float32 rows ``nx ny nz a`` on the device: the area-weighted unit normal of every vertex (0 0 0 where the sum
    vanishes; on ``mesh``'s output it points towards the observed free space) and a third of its incident area."""
    vertices, faces = vertices.contiguous(), faces.contiguous()
    adjacency = hip.mesh_adjacency(faces, vertices.shape[0])
    return hip.mesh_normals(vertices, faces, adjacency)


# ------------------------------------------------------------------------------------------------ looking at the mesh
MESH_FAR = 3.0e38  # the far_ of a view that clips no mesh depth (any finite fp32 depth is below it)


def _open_views(views):
    """the views with a depth range that clips nothing: near_ = 0 (a rastered depth is > 0), far_ = MESH_FAR"""
    return [hip.make_view(list(v.extr), list(v.intr), 0.0, MESH_FAR) for v in views]


def _frame_size(what, hw):
    """the frame of a raster, checked before anything is allocated or launched -> (h, w)"""
    h, w = int(hw[0]), int(hw[1])
    if hip.mesh_raster_workspace_bytes(h, w) < 0:
        raise ValueError(f"{what}: a frame of {h}x{w}; both sides must be at least 1 and h w below 2^31")
    return h, w


def render_mesh(vertices, faces, views, hw, legacy, *, atlas=None, block=0, normals=False):
    """Rasterize and shade an indexed mesh at K poses (include/mnerf.h "MESH RASTER") -> (rgba [K, h, w, 4] float32, depth [K, h, w]
    float32, face [K, h, w] int32) on the device, and normals [K, h, w, 4] as a fourth with ``normals``.
      views      [hip.View] * K, any K >= 0: extr, the intr of the (h, w) grid; only depths in near_ .. far_ are drawn
      face       the triangle a pixel sees (the nearest; equal depths go to the lower index), -1 where none
      depth      its camera-z there, 0 where none;  rgba: a = 1 on a hit and 0 0 0 0 elsewhere
      atlas, block   shade from the atlas of ``texture`` instead of the vertex colours
    Two-sided; triangles that cross the camera plane are dropped, not clipped.  One key buffer of 8 h w bytes serves all poses.  No
    device->host copy; the same bytes on every run."""
    h, w = _frame_size("render_mesh", hw)
    vertices, faces = vertices.contiguous(), faces.contiguous()
    dev, k_views = faces.device, len(views)
    if atlas is not None:
        atlas = atlas.contiguous()
    rgba = torch.empty(k_views, h, w, hip.RGBA_FLOATS, device=dev)
    depth = torch.empty(k_views, h, w, device=dev)
    face = torch.empty(k_views, h, w, dtype=torch.int32, device=dev)
    normal = torch.empty(k_views, h, w, hip.RGBA_FLOATS, device=dev) if normals else None
    workspace = hip.export_workspace("mesh_raster", None, hip.mesh_raster_workspace_bytes(h, w), dev)
    bary = torch.empty(h, w, 2, device=dev)
    for k, view in enumerate(views):
        hip.mesh_raster(vertices, faces, view, (h, w), legacy=legacy, out=(face[k], depth[k], bary), workspace=workspace)
        hip.mesh_shade(vertices, faces, face[k], bary, view, atlas=atlas, block=block, normals=normals,
                       out=(rgba[k], normal[k]) if normals else rgba[k])
    return (rgba, depth, face, normal) if normals else (rgba, depth, face)


def mesh_depths(vertices, faces, views, hw, legacy):
    """The mesh's own depth maps at the views -> (views with near_ / far_ so wide that no mesh depth is clipped, depth [K, h, w]
    float32).  What ``texture(visibility="mesh")`` hands to the accumulation as its depth maps.  Rasterized only: nothing is shaded.
    A pixel that sees no triangle takes the SMALLEST depth its eight neighbours see, and 0 - not VALID: near_ is the smallest positive
    float - if none sees one.  The accumulation wants all four taps of a projection VALID, and without that rim every texel within
    a pixel of the mesh's silhouette would lose its view; the smallest neighbour is the conservative choice next to an occluder."""
    h, w = _frame_size("mesh_depths", hw)
    vertices, faces = vertices.contiguous(), faces.contiguous()
    dev = faces.device
    open_views = _open_views(views)
    depth = torch.empty(len(views), h, w, device=dev)
    face, bary = torch.empty(h, w, dtype=torch.int32, device=dev), torch.empty(h, w, 2, device=dev)
    workspace = hip.export_workspace("mesh_raster", None, hip.mesh_raster_workspace_bytes(h, w), dev)
    for k, view in enumerate(open_views):
        hip.mesh_raster(vertices, faces, view, (h, w), legacy=legacy, out=(face, depth[k], bary), workspace=workspace)
    if len(views):  # the rim: a min-pool over the hit depths (no arithmetic on them - the same bytes on every run)
        hit = depth > 0
        nearest = -torch.nn.functional.max_pool2d(-torch.where(hit, depth, torch.full_like(depth, float("inf")))[:, None], 3, 1, 1)[:, 0]
        depth = torch.where(hit, depth, torch.where(torch.isfinite(nearest), nearest, torch.zeros_like(depth))).contiguous()
    tiny = float(np.finfo(np.float32).tiny)  # the accumulation's VALID test: near_ <= z, and z == 0 where nothing was hit
    return [hip.make_view(list(v.extr), list(v.intr), tiny, MESH_FAR) for v in views], depth


REPORT_KEYS = ("coverage", "spurious", "depth_rel_mean", "depth_rel_median", "psnr", "field_pixels", "mesh_pixels", "common_pixels")


def mesh_report(vertices, faces, views, depths, opacities, rgbs, hw, legacy, *, atlas=None, block=0, min_opacity=0.5):
    """Compare an indexed mesh with the field it was made from: the mesh rendered at the K fusion views (``render_mesh``, no depth
    clipped) against the field's own maps -> dict(views=[row] * K, pooled=row), a row being a dict of
      coverage           the share of the pixels with field opacity >= ``min_opacity`` that the mesh covers
      spurious           the share of the mesh's pixels where the field is below ``min_opacity``
      depth_rel_mean, depth_rel_median    of |z_mesh - z_field| / z_field on the COMMON pixels (both of the above), z_field = depth /
                         opacity as in ``fuse``
      psnr               of the mesh's colour (``atlas`` / ``block``: shaded from the atlas) against ``rgbs`` on the common pixels, dB
      field_pixels, mesh_pixels, common_pixels   the counts
    ``opacities`` None: every pixel with a finite depth > 0 is the field's.  A share or a mean over no pixel is NaN.  The reductions
    are plain tensor operations on the device; the table reaches the host in ONE copy."""
    h, w = int(hw[0]), int(hw[1])
    n, k_views = h * w, len(views)
    if k_views < 1:
        raise ValueError("mesh_report: no view")
    depths = depths.reshape(k_views, n)
    colours = rgbs.reshape(k_views, n, 3)
    rgba, z_mesh, face = render_mesh(vertices, faces, _open_views(views), (h, w), legacy, atlas=atlas, block=block)
    z_mesh, rgba = z_mesh.reshape(k_views, n), rgba.reshape(k_views, n, 4)
    if opacities is None:
        z_field = depths
        field = torch.isfinite(depths) & (depths > 0)
    else:
        opacities = opacities.reshape(k_views, n)
        field = opacities >= min_opacity
        z_field = depths / torch.where(field, opacities, torch.ones_like(opacities))
        field = field & torch.isfinite(z_field) & (z_field > 0)
    on_mesh = face.reshape(k_views, n) >= 0
    common = field & on_mesh
    rel = torch.where(common, (z_mesh - z_field).abs() / torch.where(common, z_field, torch.ones_like(z_field)), torch.zeros_like(z_field))
    err = torch.where(common[..., None], rgba[..., :3] - colours, torch.zeros_like(colours)).double().square().sum(-1)

    def rows(field, on_mesh, common, rel, err):  # over the last axis
        nf, nm, nc = field.sum(-1).double(), on_mesh.sum(-1).double(), common.sum(-1).double()
        nan = torch.full_like(rel, float("nan"))
        median = torch.where(common, rel, nan).nanmedian(-1).values.double()
        mse = err.sum(-1) / (3.0 * nc)
        return torch.stack([nc / nf, (nm - nc) / nm, rel.double().sum(-1) / nc, median, -10.0 * torch.log10(mse), nf, nm, nc], -1)

    table = torch.cat([rows(field, on_mesh, common, rel, err),
                       rows(field.reshape(1, -1), on_mesh.reshape(1, -1), common.reshape(1, -1), rel.reshape(1, -1), err.reshape(1, -1))], 0)
    table = table.cpu().numpy()  # the one copy
    as_row = lambda r: {key: (int(x) if key.endswith("_pixels") else float(x)) for key, x in zip(REPORT_KEYS, r)}
    return dict(views=[as_row(r) for r in table[:-1]], pooled=as_row(table[-1]))


def write_ply(path, points, faces=None, normals=None):
    """points [M, >= 7] (x y z . r g b ..., colours in [0, 1]; a tensor or an array) -> a binary little-endian PLY of float xyz and
    uchar rgb vertices; with ``faces`` [T, 3] (integer vertex rows) also ``element face`` with ``property list uchar int
    vertex_indices``.  Without faces the file is the point cloud's, byte for byte.  With ``normals`` [M, >= 3] the vertex element is
    x y z nx ny nz red green blue (float normals); without them the file is what it was before normals existed."""
    pts = points.detach().cpu().numpy() if torch.is_tensor(points) else np.asarray(points)
    pts = pts.reshape(-1, pts.shape[-1]) if pts.size else np.zeros((0, 8), np.float32)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if normals is not None:
        nrm = normals.detach().cpu().numpy() if torch.is_tensor(normals) else np.asarray(normals)
        nrm = nrm.reshape(-1, nrm.shape[-1]) if nrm.size else np.zeros((0, 4), np.float32)
        if len(nrm) != len(pts) or nrm.shape[1] < 3:
            raise ValueError(f"write_ply: normals {nrm.shape} do not match the {len(pts)} vertices")
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    vertex = np.zeros(len(pts), dtype=fields + [("red", "u1"), ("green", "u1"), ("blue", "u1")])
    for i, name in enumerate(("x", "y", "z")):
        vertex[name] = pts[:, i]
    for i, name in enumerate(("red", "green", "blue")):
        vertex[name] = np.rint(np.clip(np.nan_to_num(pts[:, 4 + i]), 0.0, 1.0) * 255.0).astype(np.uint8)
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" % len(pts)
    if normals is not None:
        for i, name in enumerate(("nx", "ny", "nz")):
            vertex[name] = nrm[:, i]
        header += "property float nx\nproperty float ny\nproperty float nz\n"
    header += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    body = vertex.tobytes()
    if faces is not None:
        tri = faces.detach().cpu().numpy() if torch.is_tensor(faces) else np.asarray(faces)
        tri = tri.reshape(-1, 3)
        if tri.size and (tri.min() < 0 or tri.max() >= len(pts)):
            raise ValueError(f"write_ply: face indices outside the {len(pts)} vertices")
        face = np.zeros(len(tri), dtype=[("n", "u1"), ("v", "<i4", 3)])
        face["n"], face["v"] = 3, tri
        header += "element face %d\nproperty list uchar int vertex_indices\n" % len(tri)
        body += face.tobytes()
    with open(path, "wb") as f:
        f.write((header + "end_header\n").encode("ascii"))
        f.write(body)
    return len(pts)


def write_obj(path, vertices, faces, uv, atlas, normals=None):
    """A textured mesh as Wavefront OBJ: ``path`` (.obj), the same stem + ``.mtl`` and the same stem + ``.png``.
      vertices [V, >= 3], faces [T, 3], uv [T, 3, 2] and atlas [H, W, >= 3] as ``texture`` returns them (tensors or arrays)
    The OBJ has ``v`` lines, one ``vt`` per corner with v flipped (OBJ's origin is bottom-left, the atlas's top-left), ``vn`` lines
    with ``normals`` [V, >= 3], and ``f i/t`` or ``f i/t/n`` (1-based).  The PNG is RGB 8-bit, ``rint(clip * 255)`` as ``write_ply``
    rounds (PIL writes it).  -> the number of vertices."""
    import os
    from PIL import Image
    host = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    pts, tri, tex, img = host(vertices), host(faces).reshape(-1, 3), host(uv).reshape(-1, 3, 2), host(atlas)
    pts = pts.reshape(-1, pts.shape[-1]) if pts.size else np.zeros((0, 8), np.float32)
    if len(tex) != len(tri):
        raise ValueError(f"write_obj: uv {tex.shape} does not match the {len(tri)} faces")
    if tri.size and (tri.min() < 0 or tri.max() >= len(pts)):
        raise ValueError(f"write_obj: face indices outside the {len(pts)} vertices")
    if img.ndim != 3 or img.shape[2] < 3:
        raise ValueError(f"write_obj: atlas {img.shape} is no [H, W, >= 3] image")
    nrm = None
    if normals is not None:
        nrm = host(normals)
        nrm = nrm.reshape(-1, nrm.shape[-1]) if nrm.size else np.zeros((0, 4), np.float32)
        if len(nrm) != len(pts) or nrm.shape[1] < 3:
            raise ValueError(f"write_obj: normals {nrm.shape} do not match the {len(pts)} vertices")
    stem = os.path.splitext(path)[0]
    name = os.path.basename(stem)
    pixels = np.rint(np.clip(np.nan_to_num(img[..., :3].astype(np.float64)), 0.0, 1.0) * 255.0).astype(np.uint8)
    if pixels.size:
        Image.fromarray(np.ascontiguousarray(pixels)).save(stem + ".png")
    else:  # PIL writes no empty image: the atlas of a mesh without faces is one black texel
        Image.fromarray(np.zeros((1, 1, 3), np.uint8)).save(stem + ".png")
    with open(stem + ".mtl", "w") as f:
        f.write(f"newmtl {name}\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 0\nmap_Kd {name}.png\n")
    lines = [f"mtllib {name}.mtl", f"usemtl {name}"]
    lines += ["v %.9g %.9g %.9g" % tuple(float(x) for x in p[:3]) for p in pts]
    lines += ["vt %.9g %.9g" % (float(c[0]), 1.0 - float(c[1])) for c in tex.reshape(-1, 2)]
    if nrm is not None:
        lines += ["vn %.9g %.9g %.9g" % tuple(float(x) for x in q[:3]) for q in nrm]
    for t, (a, b, c) in enumerate(tri.tolist()):
        corner = lambda k, i: f"{i + 1}/{3 * t + k + 1}" + (f"/{i + 1}" if nrm is not None else "")
        lines.append(f"f {corner(0, a)} {corner(1, b)} {corner(2, c)}")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return len(pts)
