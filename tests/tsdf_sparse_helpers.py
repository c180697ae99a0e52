"""The brick-sparse TSDF volume (include/mnerf.h "SPARSE TSDF VOLUME") restated in numpy on top of tests/mesh_helpers.py: which voxels
are NEAR, which bricks that asks for, the table, the bricked layout of a dense volume, and the renumbering between the dense
mesher's order and the sparse one's - derived from ``vertex_key`` / ``face_key`` of ``M.mesh``.

``near`` follows ``M.integrate`` operation by operation (the same projection, texel and tests), with ``dtype`` float64 (the reference)
or float32.  In float64 it also returns the voxels whose NEAR decision fp32 may take the other way for a reason ``M.integrate``'s
``border`` does not cover: an sdf within 1e-5 trunc of +trunc."""
import functools

import numpy as np

import fusion_helpers as F
import mesh_helpers as M

BRICK = 8
POINTS = BRICK ** 3
MAX_BRICKS = ((1 << 31) - 1) // 12 // POINTS
# (origin, voxel, dims, trunc = 4 voxels): the scene of M.GRIDS[3] on a grid of 6 x 6 x 8 bricks, every axis partial; and M's
# "half_outside" so
FINE_DIMS = (47, 43, 57)
GRIDS = {"fine": ((-0.93, -0.83, -0.71), 0.04, FINE_DIMS, 0.16), "fine_half_outside": ((0.01, -1.73, -1.51), 0.08, FINE_DIMS, 0.32)}


def grid_of(k, grid):
    return GRIDS[grid] if grid in GRIDS else M.grid_of(k, grid)


def brick_dims(dims):
    return tuple(-(-d // BRICK) for d in dims)


# ------------------------------------------------------------------------------------------------ mark
def near(cams, h, w, legacy, depth, opacity, origin, voxel, dims, trunc, n_consistent=None, min_consistent=0,
         min_opacity=M.MIN_OPACITY, dtype=np.float64):
    """-> near [nz, ny, nx] bool: some view updates the voxel with t < 1;  edge [nz, ny, nx] bool: an sdf within 1e-5 trunc of trunc"""
    nx, ny, nz = dims
    inv = F.inverse_cameras(cams, dtype)
    z_all, valid_all, _ = F.values(cams, depth, opacity, min_opacity, dtype)
    off, tr = dtype(0.0 if legacy else 0.5), dtype(trunc)
    p = M.centres(origin, voxel, dims, dtype)
    out, edge = np.zeros((nz, ny, nx), bool), np.zeros((nz, ny, nx), bool)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for j in range(len(cams)):
            u, v, zc = F.proj(inv[j], p)
            fx, fy = np.floor((u - off) + dtype(0.5)), np.floor((v - off) + dtype(0.5))
            inside = (zc > 0) & (fx >= 0) & (fx < w) & (fy >= 0) & (fy < h)
            index = np.where(inside, fy * w + fx, 0).astype(np.int64)
            ok = inside & valid_all[j].reshape(-1)[index]
            if n_consistent is not None:
                ok &= np.asarray(n_consistent)[j].reshape(-1)[index] >= min_consistent
            sdf = np.where(ok, z_all[j].reshape(-1)[index], dtype(1)) - zc
            added = ok & ~(sdf < -tr)
            out |= added & (np.minimum(dtype(1), sdf / tr) < 1)
            edge |= ok & (np.abs(sdf - tr) < 1e-5 * tr)
    return out, edge


def dilate(mask):
    """the 3 x 3 x 3 neighbourhood inside the grid"""
    nz, ny, nx = mask.shape
    padded = np.zeros((nz + 2, ny + 2, nx + 2), bool)
    padded[1:-1, 1:-1, 1:-1] = mask
    out = np.zeros_like(mask)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                out |= padded[dz:dz + nz, dy:dy + ny, dx:dx + nx]
    return out


def bricks_holding(mask):
    """[nz, ny, nx] bool -> [bz, by, bx] bool: the bricks with a voxel of the mask"""
    nz, ny, nx = mask.shape
    bx, by, bz = brick_dims((nx, ny, nz))
    padded = np.zeros((bz * BRICK, by * BRICK, bx * BRICK), bool)
    padded[:nz, :ny, :nx] = mask
    return padded.reshape(bz, BRICK, by, BRICK, bx, BRICK).any((1, 3, 5))


def wanted_bricks(near_mask):
    """the rule of mnerf_tsdf_bricks_mark: the brick of every voxel of a NEAR voxel's neighbourhood"""
    return bricks_holding(dilate(near_mask))


# ------------------------------------------------------------------------------------------------ table and layout
def table_of(bricks):
    """[bz, by, bx] bool -> (table int32 [bz, by, bx]: slots ascending with the linear index, -1 elsewhere; the list of the bricks'
    linear indices)"""
    flat = bricks.reshape(-1)
    table = np.where(flat, np.cumsum(flat) - 1, -1).astype(np.int32)
    return table.reshape(bricks.shape), np.flatnonzero(flat).astype(np.int32)


def point_of(table, iz, iy, ix):
    """the sparse point index slot 512 + in-brick index of the voxels (iz, iy, ix) (arrays); -1 in a brick without a slot"""
    slot = table[iz >> 3, iy >> 3, ix >> 3].astype(np.int64)
    return np.where(slot < 0, -1, slot * POINTS + ((iz & 7) * 8 + (iy & 7)) * 8 + (ix & 7))


def brick_volume(sums, weight, table, poison=True):
    """a dense volume -> (sums [n, 512, 4], weight [n, 512]) of the table's bricks.  ``poison``: the voxels of partial bricks outside
    the grid hold weight 3 and S = -3 - lattice points inside the surface, had the mesher read them"""
    nz, ny, nx = weight.shape
    n = int(table.max()) + 1 if table.size else 0
    out_s = np.zeros((n, POINTS, 4), np.float32)
    out_w = np.zeros((n, POINTS), np.float32)
    if poison:
        out_s[..., 0], out_w[...] = -3.0, 3.0
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    p = point_of(table, iz, iy, ix)
    keep = p >= 0
    out_s.reshape(-1, 4)[p[keep]] = sums[keep]
    out_w.reshape(-1)[p[keep]] = weight[keep]
    return out_s, out_w


def mask_volume(sums, weight, bricks):
    """a dense volume zeroed outside the bricks"""
    nz, ny, nx = weight.shape
    keep = np.repeat(np.repeat(np.repeat(bricks, BRICK, 0), BRICK, 1), BRICK, 2)[:nz, :ny, :nx]
    return np.where(keep[..., None], sums, 0).astype(sums.dtype), np.where(keep, weight, 0).astype(weight.dtype)


# ------------------------------------------------------------------------------------------------ order
def renumber(dense, dims, table):
    """``dense`` = M.mesh's dict of the dense volume -> (vertices, faces) in the sparse mesher's order: vertices ascending in (slot,
    in-brick index of the owner, direction), triangles in (slot of the cell's origin point, in-brick index, tet, triangle), the
    indices renumbered.  Every owner and every cell origin must lie in a brick with a slot."""
    nx, ny, nz = dims
    owner, direction = dense["vertex_key"][:, 0], dense["vertex_key"][:, 1]
    vp = point_of(table, owner // (nx * ny), owner // nx % ny, owner % nx)
    assert (vp >= 0).all(), "a vertex's owner lies in no allocated brick"
    vorder = np.argsort(vp * 7 + direction, kind="stable")
    new_index = np.empty(len(vorder), np.int64)
    new_index[vorder] = np.arange(len(vorder))
    cx, cy = max(nx - 1, 0), max(ny - 1, 0)
    cell, tet, tri = dense["face_key"][:, 0], dense["face_key"][:, 1], dense["face_key"][:, 2]
    fp = point_of(table, cell // (cx * cy), cell // cx % cy, cell % cx) if len(cell) else np.zeros(0, np.int64)
    assert (fp >= 0).all(), "a cell's origin lies in no allocated brick"
    forder = np.argsort((fp * 6 + tet) * 2 + tri, kind="stable")
    return dense["vertices"][vorder], new_index[dense["faces"][forder]].astype(np.int32)


def canonical(vertices, faces):
    """a mesh whose vertex rows are distinct -> (rows sorted as uint32 words, faces over those rows, sorted): equal for two meshes
    iff one is the other with its vertices and its triangles reordered"""
    words = np.ascontiguousarray(vertices, np.float32).view(np.uint32).reshape(len(vertices), -1)
    order = np.lexsort(words.T[::-1])
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    sorted_rows = words[order]
    assert len(words) < 2 or (sorted_rows[1:] != sorted_rows[:-1]).any(1).all(), "two vertex rows are the same bits"
    f = rank[np.asarray(faces, np.int64)]
    return sorted_rows, f[np.lexsort(f.T[::-1])]


# ------------------------------------------------------------------------------------------------ cases
# (k, h, w, legacy, variant, consistent, grid) -> (the bricks the rule asks for, of how many, vertices, faces of the mesh at
# min_weight = max(1, min(2, K - 1))): neither all bricks nor none
CPU_CASES = {(3, 24, 32, True, "plain", False, "default"): (18, 27, 1280, 2266), (3, 24, 32, False, "plain", True, "fine"): (72, 288, 3468, 6060),
             (2, 24, 32, True, "plain", False, "fine"): (103, 288, 11658, 21956),
             (3, 24, 32, True, "plain", True, "fine_half_outside"): (22, 288, 453, 688)}


def min_weight_of(k):
    return float(max(1, min(2, k - 1)))
# what the GPU marks: every axis partial; 16 views; 20 views in two calls; both pixel-centre conventions; half outside
MARK_CASES = [(3, 24, 32, False, "plain", False, "fine"), (3, 24, 32, True, "plain", True, "fine"), (16, 37, 53, False, "plain", False, "default"),
              (20, 24, 32, True, "plain", False, "default"), (3, 24, 32, True, "plain", True, "half_outside"),
              (3, 24, 32, False, "opacity", False, "default")]


@functools.lru_cache(maxsize=None)
def reference(k, h, w, legacy, variant="plain", consistent=False, grid="default"):
    """M.integrate_reference on any grid of ``grid_of``, plus near / near32 (the NEAR voxels in float64 / float32) and ``unsure``
    (float64: M's borderline voxels and those with an sdf at +trunc).  Computed once and shared, read-only."""
    s = F.scene(k, h, w, legacy, variant)
    origin, voxel, dims, trunc = grid_of(k, grid)
    rgb = M.scene_colours(k, h, w)
    depth, opacity, counts, min_consistent = s["depth"], s["opacity"], None, 0
    if consistent:
        refs = F.reference(k, h, w, legacy, variant)
        depth = np.stack([r["fused"] for r in refs]).astype(np.float32)
        counts = np.stack([r["count"] for r in refs]).astype(np.int32)
        opacity, min_consistent = None, min(2, k - 1)
    args = dict(n_consistent=counts, min_consistent=min_consistent)
    _, _, border = M.integrate(s["cams"], h, w, legacy, depth, opacity, rgb, origin, voxel, dims, trunc, **args)
    sums32, weight32, _ = M.integrate(s["cams"], h, w, legacy, depth, opacity, rgb, origin, voxel, dims, trunc, dtype=np.float32, **args)
    near64, edge = near(s["cams"], h, w, legacy, depth, opacity, origin, voxel, dims, trunc, **args)
    near32, _ = near(s["cams"], h, w, legacy, depth, opacity, origin, voxel, dims, trunc, dtype=np.float32, **args)
    return dict(cams=s["cams"], depth=depth, opacity=opacity, rgb=rgb, counts=counts, min_consistent=min_consistent, origin=origin,
                voxel=voxel, dims=dims, trunc=trunc, sums32=sums32, weight32=weight32, near=near64, near32=near32, unsure=border | edge)


# ------------------------------------------------------------------------------------------------ argument refusals
def assert_refusals(hip):
    """every MNERF_E_* the header names for the sparse entry points, from fake addresses: each call fails its checks, or has nothing
    to launch, before any HIP call"""
    import ctypes as C
    lib = hip.load()
    fake, odd, two = C.c_void_p(0x10000), C.c_void_p(0x10004), C.c_void_p(0x10002)
    i32 = lambda p: None if p is None else C.cast(p, C.POINTER(C.c_int32))
    views = hip.view_array([hip.make_view(c["extr"], c["intr"], c["near"], c["far"]) for c in F.arc_cameras(3, 8, 8)])
    singular = hip.view_array([hip.make_view(np.zeros((3, 4), np.float32), c["intr"], c["near"], c["far"]) for c in F.arc_cameras(1, 8, 8)])
    nan, inf = float("nan"), float("inf")
    r, n, a, ok = hip.MNERF_E_RANGE, hip.MNERF_E_NULL, hip.MNERF_E_ALIGN, hip.MNERF_OK
    huge = (1 << 14, 1 << 14, 1 << 13)  # 2^41 voxels, 2^32 bricks: each axis fits an int32, the bricks do not

    def mark(views=views, n_views=3, h=8, w=8, depth=fake, opacity=None, counts=None, min_opacity=0.5, trunc=0.1, origin=(0.0, 0.0, 0.0),
             voxel=0.1, dims=(12, 9, 20), marks=fake):
        return lib.mnerf_tsdf_bricks_mark(views, n_views, h, w, 1, depth, opacity, i32(counts), 1, min_opacity, trunc, *origin, voxel, *dims,
                                          marks, None)

    maps_refused = [(r, dict(n_views=0)), (r, dict(n_views=hip.MNERF_MAX_VIEWS + 1)), (r, dict(h=0)), (r, dict(w=0)),
                    (r, dict(h=1 << 16, w=1 << 15)), (r, dict(trunc=0.0)), (r, dict(trunc=nan)), (r, dict(trunc=inf)),
                    (r, dict(opacity=fake, min_opacity=nan)), (r, dict(dims=(-1, 4, 4))), (r, dict(dims=huge)), (r, dict(voxel=0.0)),
                    (r, dict(voxel=nan)), (r, dict(origin=(0.0, inf, 0.0))), (r, dict(views=singular, n_views=1)), (n, dict(views=None)),
                    (n, dict(depth=None))]
    for want, kwargs in maps_refused + [(n, dict(marks=None)), (ok, dict(dims=(4, 0, 4), marks=None, depth=None))]:
        assert mark(**kwargs) == want, ("mark", kwargs, lib.mnerf_last_error())

    def table(marks=fake, bdims=(2, 2, 3), table=fake, bricks=fake, count=fake, workspace=fake):
        return lib.mnerf_tsdf_bricks_table(marks, *bdims, i32(table), i32(bricks), count, workspace, None)

    for want, kwargs in [(r, dict(bdims=(-1, 2, 2))), (r, dict(bdims=(1 << 11, 1 << 10, 1 << 10))), (n, dict(count=None)),
                         (n, dict(marks=None)), (n, dict(table=None)), (n, dict(bricks=None)), (n, dict(workspace=None)),
                         (a, dict(table=two)), (a, dict(bricks=two)), (a, dict(workspace=two)), (a, dict(count=odd))]:
        assert table(**kwargs) == want, ("table", kwargs, lib.mnerf_last_error())

    def integrate(views=views, n_views=3, h=8, w=8, depth=fake, opacity=None, counts=None, rgb=fake, min_opacity=0.5, trunc=0.1,
                  origin=(0.0, 0.0, 0.0), voxel=0.1, dims=(12, 9, 20), bricks=fake, n_bricks=5, sums=fake, weight=fake):
        return lib.mnerf_tsdf_integrate_sparse(views, n_views, h, w, 1, depth, opacity, i32(counts), 1, rgb, min_opacity, trunc, *origin,
                                               voxel, *dims, i32(bricks), n_bricks, sums, weight, None)

    for want, kwargs in maps_refused + [(r, dict(n_bricks=-1)), (r, dict(n_bricks=13)), (r, dict(dims=(1 << 10,) * 3, n_bricks=MAX_BRICKS + 1)),
                                        (n, dict(rgb=None)), (n, dict(bricks=None)), (n, dict(sums=None)), (n, dict(weight=None)),
                                        (a, dict(sums=odd)), (a, dict(weight=two)), (a, dict(bricks=two)),
                                        (ok, dict(n_bricks=0, sums=None, weight=None, depth=None, bricks=None)),
                                        (ok, dict(dims=(4, 0, 4), n_bricks=0, sums=None, weight=None, depth=None))]:
        assert integrate(**kwargs) == want, ("integrate", kwargs, lib.mnerf_last_error())

    def mesh(sums=fake, weight=fake, table=fake, bricks=fake, n_bricks=5, origin=(0.0, 0.0, 0.0), voxel=0.1, dims=(12, 9, 20), min_weight=1.0,
             vertices=fake, vcap=8, triangles=fake, tcap=8, counts=fake, workspace=fake):
        return lib.mnerf_tsdf_mesh_sparse(sums, weight, i32(table), i32(bricks), n_bricks, *origin, voxel, *dims, min_weight, vertices, vcap,
                                          i32(triangles), tcap, counts, workspace, None)

    for want, kwargs in [(r, dict(dims=(4, -1, 4))), (r, dict(dims=huge)), (r, dict(n_bricks=-1)), (r, dict(n_bricks=13)),
                         (r, dict(dims=(1 << 10,) * 3, n_bricks=MAX_BRICKS + 1)), (r, dict(voxel=-1.0)), (r, dict(voxel=inf)),
                         (r, dict(origin=(nan, 0.0, 0.0))), (r, dict(min_weight=0.0)), (r, dict(min_weight=nan)), (r, dict(vcap=-1)),
                         (r, dict(tcap=-1)), (n, dict(sums=None)), (n, dict(weight=None)), (n, dict(table=None)), (n, dict(bricks=None)),
                         (n, dict(counts=None)), (n, dict(workspace=None)), (n, dict(vertices=None)), (n, dict(triangles=None)),
                         (a, dict(sums=odd)), (a, dict(vertices=odd)), (a, dict(counts=odd)), (a, dict(weight=two)), (a, dict(triangles=two)),
                         (a, dict(table=two)), (a, dict(bricks=two)), (a, dict(workspace=two)),
                         (ok, dict(n_bricks=0, sums=None, weight=None, table=None, bricks=None, counts=None, workspace=None, vertices=None,
                                   triangles=None))]:
        assert mesh(**kwargs) == want, ("mesh", kwargs, lib.mnerf_last_error())
    # the workspace formulas of the header
    for bdims in ((1, 1, 1), (6, 6, 8), (128, 128, 128)):
        bricks = bdims[0] * bdims[1] * bdims[2]
        blocks = -(-bricks // 256)
        assert hip.tsdf_bricks_table_workspace_bytes(bdims) == (4 * (blocks + -(-blocks // 1024)) + 15) // 16 * 16, bdims
        for n_bricks in (0, 1, min(bricks, 7), min(bricks, 600), min(bricks, MAX_BRICKS)):
            points = 512 * n_bricks
            blocks = 2 * n_bricks
            tiles = -(-blocks // 1024)
            assert hip.tsdf_mesh_sparse_workspace_bytes(n_bricks, bdims) == (4 * (points + 2 * blocks + 2 * tiles) + 2 * points + 15) // 16 * 16
    assert hip.tsdf_bricks_table_workspace_bytes((0, 5, 5)) == 0 and hip.tsdf_bricks_table_workspace_bytes((-1, 5, 5)) == -1
    assert hip.tsdf_bricks_table_workspace_bytes((1 << 11, 1 << 10, 1 << 10)) == -1
    assert hip.tsdf_mesh_sparse_workspace_bytes(28, (3, 3, 3)) == -1 and hip.tsdf_mesh_sparse_workspace_bytes(-1, (3, 3, 3)) == -1
    assert hip.tsdf_mesh_sparse_workspace_bytes(MAX_BRICKS + 1, (128, 128, 128)) == -1 and MAX_BRICKS == hip.MAX_BRICKS == 349525
