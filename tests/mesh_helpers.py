"""Mesh export (include/mnerf.h "MESH EXPORT") restated in numpy: the TSDF integrator and the marching-tetrahedra mesher, operation by
operation after the header's text, with ``dtype`` float64 (the reference) or float32 (the device's format, whose distance from
float64 sizes the gates).  Cameras, ``raycast``, ``proj`` and ``values`` are those of tests/fusion_helpers.py.

In float64 ``integrate`` also marks the BORDERLINE voxels, whose update may legitimately differ in fp32: for some view a projection
within 1e-3 px of a texel boundary or of the frame (counted where the texel on either side of that boundary would be added - where
both are skipped, the voxel's sums do not depend on the choice), a camera-z within 1e-6 of 0, an sdf within 1e-5 trunc of -trunc,
or a texel that ``values`` marks as decided by a margin.

The restatement and the kernels have one author; the properties tested on the sphere (watertight, Euler characteristic, outward
normals, distance to the surface, area) are what is independent of both."""
import functools

import numpy as np

import fusion_helpers as F

MIN_OPACITY = F.MIN_OPACITY
BORDERLINE_CAP = F.BORDERLINE_CAP
DIMS = (19, 17, 23)  # nx, ny, nz: 7429 voxels = 29 workgroups + 5 voxels, every axis odd
# (K, h, w) -> the grid (origin, voxel, trunc).  The plane z = 0 and the box in front of it are seen from z < 0: the grid reaches
# from in front of the box to behind the plane.  With 16 views the share of voxels that SOME view projects next to a texel boundary
# is eight times that of 2 views (2 % at the voxel of 0.1, the restatement finds), so those cases take voxels of 0.2 around the
# same scene: a tenth of the voxels is updated and 0.4 - 0.7 % are borderline.
GRIDS = {2: ((-0.93, -0.83, -0.71), 0.1, 0.25), 3: ((-0.93, -0.83, -0.71), 0.1, 0.25), 16: ((-1.93, -1.73, -1.51), 0.2, 0.35),
         20: ((-1.93, -1.73, -1.51), 0.2, 0.35)}
INTEGRATE_CASES = [(k, h, w, legacy) for (k, h, w) in ((2, 24, 32), (3, 24, 32), (16, 37, 53)) for legacy in (True, False)]
VARIANTS = F.VARIANTS

# ------------------------------------------------------------------------------------------------ the header's tables
TET_AXES = ((0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1))  # the first two axes of xyz xzy yxz yzx zxy zyx
TET_ODD = (0, 1, 1, 0, 0, 1)


def tet_corners(t):
    a, b = TET_AXES[t]
    return (0, 1 << a, (1 << a) | (1 << b), 7)


def tet_case(code):
    """the header's rule for a positively oriented tet -> [triangle], a triangle = 3 edges (lo, hi) of tet vertices"""
    ins = [k for k in range(4) if code >> k & 1]
    outs = [k for k in range(4) if not code >> k & 1]
    edge = lambda p, q: (min(p, q), max(p, q))
    if len(ins) in (1, 3):
        a, rest = (ins[0], outs) if len(ins) == 1 else (outs[0], ins)
        tris = [[edge(a, r) for r in rest]]
    elif len(ins) == 2:
        (a, b), (c, d) = ins, outs
        tris = [[edge(a, c), edge(a, d), edge(b, d)], [edge(a, c), edge(b, d), edge(b, c)]]
    else:
        return []
    if sum(i > o for i in ins for o in outs) % 2:
        tris = [[t[0], t[2], t[1]] for t in tris]
    return tris


# ------------------------------------------------------------------------------------------------ grid and volumes
def centres(origin, voxel, dims, dtype):
    """-> [nz, ny, nx, 3]"""
    ax = [dtype(origin[a]) + (np.arange(dims[a]).astype(dtype) + dtype(0.5)) * dtype(voxel) for a in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([x, y, z], -1)


SPHERE_C = (np.sqrt(2.0) - 1.0, np.sqrt(3.0) - 1.5, np.pi - 3.0)  # irrational: no lattice value is 0
SPHERE_R = np.e / 4.0


def sphere_grid(dims):
    """a grid around the sphere with a margin of about two voxels, the lattice off the centre by an uneven part of a voxel (centred,
    lattice points would lie on the sphere exactly) -> (origin, voxel)"""
    voxel = np.floor(1024.0 * 2.0 * SPHERE_R / (min(dims) - 4.3)) / 1024.0  # a multiple of 2^-10: exact in fp32
    return tuple(float(SPHERE_C[a] - (0.5 * dims[a] + (0.137, 0.291, 0.073)[a]) * voxel) for a in range(3)), float(voxel)


@functools.lru_cache(maxsize=None)
def sphere_volume(dims, open_octant=False):
    """-> dict(sums [nz,ny,nx,4] f32, weight [nz,ny,nx] f32, origin, voxel): S = 3 d with weight 3, d = |p - c| - r in voxels of
    truncation, a colour that varies with the position; ``open_octant``: the weights of the octant above the centre are 0"""
    origin, voxel = sphere_grid(dims)
    p = centres(origin, voxel, dims, np.float64)
    d = np.linalg.norm(p - np.array(SPHERE_C), axis=-1) - SPHERE_R
    weight = np.full(d.shape, 3.0, np.float32)
    if open_octant:
        weight[(p > np.array(SPHERE_C)).all(-1)] = 0.0
    colour = 0.5 + 0.5 * np.sin(3.0 * p)
    sums = np.concatenate([(3.0 * d / (4.0 * voxel))[..., None], 3.0 * colour], -1).astype(np.float32)
    assert (sums[..., 0] != 0).all()
    return dict(sums=sums, weight=weight, origin=origin, voxel=voxel)


# ------------------------------------------------------------------------------------------------ a. integration
def scene_colours(k, h, w):
    return np.random.default_rng(7 * k + h).random((k, h * w, 3)).astype(np.float32)


def integrate(cams, h, w, legacy, depth, opacity, rgb, origin, voxel, dims, trunc, n_consistent=None, min_consistent=0,
              min_opacity=MIN_OPACITY, dtype=np.float64, volume=None):
    """-> sums [nz,ny,nx,4], weight [nz,ny,nx] (dtype; added to ``volume`` = (sums, weight)), borderline [nz,ny,nx] bool"""
    nx, ny, nz = dims
    inv = F.inverse_cameras(cams, dtype)
    z_all, valid_all, edge_all = F.values(cams, depth, opacity, min_opacity, dtype)
    off, tr = dtype(0.0 if legacy else 0.5), dtype(trunc)
    p = centres(origin, voxel, dims, dtype)
    sums = np.zeros((nz, ny, nx, 4), dtype) if volume is None else volume[0].astype(dtype).copy()
    weight = np.zeros((nz, ny, nx), dtype) if volume is None else volume[1].astype(dtype).copy()
    border = np.zeros((nz, ny, nx), bool)
    colour = np.asarray(rgb).reshape(len(cams), h * w, 3).astype(dtype)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for j in range(len(cams)):
            u, v, zc = F.proj(inv[j], p)
            front = zc > 0

            def texel(u, v):
                """-> texel index (0 where there is none), the sdf, `added`: the voxel takes this texel"""
                fx, fy = np.floor((u - off) + dtype(0.5)), np.floor((v - off) + dtype(0.5))
                inside = front & (fx >= 0) & (fx < w) & (fy >= 0) & (fy < h)
                index = np.where(inside, fy * w + fx, 0).astype(np.int64)
                ok = inside & valid_all[j].reshape(-1)[index]
                if n_consistent is not None:
                    ok &= np.asarray(n_consistent)[j].reshape(-1)[index] >= min_consistent
                sdf = np.where(ok, z_all[j].reshape(-1)[index], dtype(1)) - zc
                return index, sdf, ok & ~(sdf < -tr), inside, ok

            index, sdf, added, inside, ok = texel(u, v)
            t = np.minimum(dtype(1), sdf / tr)
            sums[..., 0] = sums[..., 0] + np.where(added, t, dtype(0))
            sums[..., 1:] = sums[..., 1:] + np.where(added[..., None], colour[j][index], dtype(0))
            weight = weight + added.astype(dtype)
            if dtype is np.float64:
                border |= np.abs(zc) < 1e-6
                border |= inside & edge_all[j].reshape(-1)[index]
                border |= ok & (np.abs(sdf + tr) < 1e-5 * tr)
                for sx in (-1e-3, 1e-3):  # the texel an fp32 projection may pick instead
                    for sy in (-1e-3, 1e-3):
                        index2, sdf2, added2, _, _ = texel(u + sx, v + sy)
                        border |= front & (index2 != index) & (added | added2)
                        border |= front & (added != added2)
    return sums, weight, border


def grid_of(k, grid="default"):
    """-> origin, voxel, dims, trunc.  "single": one voxel in front of the box; "half_outside": the x axis starts at the scene's
    centre and runs 3.8 units out of it, past every frustum (their half width at the plane is about 1.2)"""
    if grid == "single":
        return (-0.083, -0.061, -0.93), 0.1, (1, 1, 1), 0.25  # (off the optical axes: those project onto a texel boundary)
    if grid == "half_outside":
        return (0.01, -1.73, -1.51), 0.2, DIMS, 0.35
    origin, voxel, trunc = GRIDS[k]
    return origin, voxel, DIMS, trunc


@functools.lru_cache(maxsize=None)
def integrate_reference(k, h, w, legacy, variant="plain", consistent=False, grid="default"):
    """the float64 and float32 restatements of one GPU case, computed once and shared (read-only) -> dict(inputs..., sums, weight,
    border, sums32, weight32).  ``consistent``: the maps are the fused depths of the float64 consistency restatement with their
    counts, min_consistent = min(2, K - 1), no opacity - what fusion.mesh feeds the integrator."""
    s = F.scene(k, h, w, legacy, variant)
    origin, voxel, dims, trunc = grid_of(k, grid)
    rgb = scene_colours(k, h, w)
    depth, opacity, counts, min_consistent = s["depth"], s["opacity"], None, 0
    if consistent:
        refs = F.reference(k, h, w, legacy, variant)
        depth = np.stack([r["fused"] for r in refs]).astype(np.float32)
        counts = np.stack([r["count"] for r in refs]).astype(np.int32)
        opacity, min_consistent = None, min(2, k - 1)
    args = dict(n_consistent=counts, min_consistent=min_consistent)
    sums, weight, border = integrate(s["cams"], h, w, legacy, depth, opacity, rgb, origin, voxel, dims, trunc, **args)
    sums32, weight32, _ = integrate(s["cams"], h, w, legacy, depth, opacity, rgb, origin, voxel, dims, trunc, dtype=np.float32, **args)
    return dict(cams=s["cams"], depth=depth, opacity=opacity, rgb=rgb, counts=counts, min_consistent=min_consistent, origin=origin,
                voxel=voxel, dims=dims, trunc=trunc, sums=sums, weight=weight, border=border, sums32=sums32, weight32=weight32)


def integrate_cases():
    """every case the GPU test integrates: (k, h, w, legacy, variant, consistent, grid)"""
    cases = [(k, h, w, legacy, variant, consistent, "default") for (k, h, w, legacy) in INTEGRATE_CASES
             for variant in (VARIANTS if k == 3 else ("plain",)) for consistent in (False, True)]
    return cases + [(20, 24, 32, False, "plain", False, "default"), (3, 24, 32, False, "plain", False, "single"),
                    (3, 24, 32, True, "plain", True, "half_outside")]


def vertex_distance(got, want, extent):
    """rows x y z w | r g b 0 -> the largest difference: positions relative to the grid's extent, the weight relative to the
    largest weight, colours absolute (they lie in [0, 1])"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if not len(want):
        return 0.0
    diff = np.abs(got - want)
    return float(max(diff[:, :3].max() / extent, diff[:, 3].max() / max(1.0, np.abs(want[:, 3]).max()), diff[:, 4:].max()))


def volume_distance(sums, weight, want_sums, want_weight, keep):
    """the largest |difference| of S and of RGB per unit of weight (a sum of `weight` terms of magnitude <= 1) over the voxels of
    ``keep`` whose weights agree -> (S, RGB)"""
    same = keep & (weight == want_weight)
    scale = np.maximum(1.0, want_weight.astype(np.float64))[same]
    diff = np.abs(sums.astype(np.float64) - want_sums.astype(np.float64))[same]
    if not same.any():
        return 0.0, 0.0
    return float((diff[:, 0] / scale).max()), float((diff[:, 1:] / scale[:, None]).max())


# ------------------------------------------------------------------------------------------------ b. mesher
def mesh(sums, weight, origin, voxel, min_weight, dtype=np.float64):
    """-> dict(vertices [V, 8] dtype, faces [T, 3] int32, vertex_key [V, 2] (owner's linear index, direction), face_key [T, 3]
    (cell's linear index among the cells, tet, triangle), cell_valid [nz-1, ny-1, nx-1])"""
    nz, ny, nx = weight.shape
    w = weight.astype(dtype)
    s = sums.astype(dtype)
    valid = w >= dtype(min_weight)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = s[..., 0] / w
        colour = s[..., 1:] / w[..., None]
        inside = valid & (d < 0)
    cz, cy, cx = max(nz - 1, 0), max(ny - 1, 0), max(nx - 1, 0)
    cell_valid = np.ones((cz, cy, cx), bool)
    for c in range(8):
        cell_valid &= valid[(c >> 2):(c >> 2) + cz, (c >> 1 & 1):(c >> 1 & 1) + cy, (c & 1):(c & 1) + cx]
    padded = np.zeros((nz + 1, ny + 1, nx + 1), bool)  # cell (k, j, i) at [k + 1, j + 1, i + 1]; no cell on the borders
    padded[1:cz + 1, 1:cy + 1, 1:cx + 1] = cell_valid
    live = np.zeros((nz, ny, nx, 7), bool)
    for e in range(1, 8):
        ex, ey, ez = e & 1, e >> 1 & 1, e >> 2
        used = np.zeros((nz, ny, nx), bool)
        for f in range(8):
            if f & e:
                continue
            fx, fy, fz = f & 1, f >> 1 & 1, f >> 2
            used |= padded[1 - fz:1 - fz + nz, 1 - fy:1 - fy + ny, 1 - fx:1 - fx + nx]
        differ = np.zeros((nz, ny, nx), bool)
        differ[:nz - ez, :ny - ey, :nx - ex] = inside[:nz - ez, :ny - ey, :nx - ex] != inside[ez:, ey:, ex:]
        live[..., e - 1] = used & differ
    kz, ky, kx, kd = np.nonzero(live)  # ascending (linear index, direction)
    vid = np.full((nz, ny, nx, 7), -1, np.int64)
    vid[kz, ky, kx, kd] = np.arange(len(kz))
    p = centres(origin, voxel, (nx, ny, nz), dtype)
    ez_, ey_, ex_ = (kd + 1) >> 2, (kd + 1) >> 1 & 1, (kd + 1) & 1
    a, b = (kz, ky, kx), (kz + ez_, ky + ey_, kx + ex_)
    da, db = d[a], d[b]
    t = (da / (da - db))[:, None]
    rows_a = np.concatenate([p[a], w[a][:, None], colour[a]], 1)
    rows_b = np.concatenate([p[b], w[b][:, None], colour[b]], 1)
    vertices = np.concatenate([rows_a + t * (rows_b - rows_a), np.zeros((len(kz), 1), dtype)], 1).astype(dtype)
    vertex_key = np.stack([(kz * ny + ky) * nx + kx, kd], 1)

    code = np.zeros((cz, cy, cx), np.int64)
    for c in range(8):
        code |= inside[(c >> 2):(c >> 2) + cz, (c >> 1 & 1):(c >> 1 & 1) + cy, (c & 1):(c & 1) + cx].astype(np.int64) << c
    tri = np.full((cz, cy, cx, 6, 2, 3), -1, np.int64)
    oz, oy, ox = np.meshgrid(np.arange(cz), np.arange(cy), np.arange(cx), indexing="ij")
    for t_ in range(6):
        corner = tet_corners(t_)
        tcode = sum((code >> corner[k] & 1) << k for k in range(4))
        for case in range(1, 15):
            sel = cell_valid & (tcode == case)
            if not sel.any():
                continue
            for n_, triangle in enumerate(tet_case(case)):
                if TET_ODD[t_]:
                    triangle = [triangle[0], triangle[2], triangle[1]]
                for m, (lo, hi) in enumerate(triangle):
                    c_lo, c_hi = corner[lo], corner[hi]
                    tri[..., t_, n_, m][sel] = vid[oz[sel] + (c_lo >> 2), oy[sel] + (c_lo >> 1 & 1), ox[sel] + (c_lo & 1),
                                                   (c_hi ^ c_lo) - 1]
    flat = tri.reshape(-1, 3)
    keep = flat[:, 0] >= 0
    assert (flat[keep] >= 0).all()  # every triangle vertex is a live edge
    cell, tet, n_ = np.unravel_index(np.flatnonzero(keep), (cz * cy * cx, 6, 2))
    return dict(vertices=vertices, faces=flat[keep].astype(np.int32), vertex_key=vertex_key, face_key=np.stack([cell, tet, n_], 1),
                cell_valid=cell_valid)


@functools.lru_cache(maxsize=None)
def sphere_mesh(dims, open_octant=False, dtype=np.float64):
    """the restatement's mesh of the sphere volume (min_weight 2), computed once and shared (read-only)"""
    vol = sphere_volume(dims, open_octant)
    return mesh(vol["sums"], vol["weight"], vol["origin"], vol["voxel"], 2.0, dtype)


# ------------------------------------------------------------------------------------------------ mesh properties
def edge_uses(faces):
    """directed edges of the faces -> (the undirected edges [E, 2], uses forward [E], uses backward [E])"""
    f = np.asarray(faces, np.int64)
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    lo, hi, forward = np.minimum(a, b), np.maximum(a, b), a < b
    und, which = np.unique(np.stack([lo, hi], 1), axis=0, return_inverse=True)
    which = which.reshape(-1)
    return und, np.bincount(which[forward], minlength=len(und)), np.bincount(which[~forward], minlength=len(und))


def assert_closed_sphere(vertices, faces, voxel):
    """watertight and consistently wound, Euler characteristic 2, every vertex used, outward normals, on the sphere -> area"""
    v, f = np.asarray(vertices, np.float64)[:, :3], np.asarray(faces, np.int64)
    assert (v[:, 0] == v[:, 0]).all() and f.min() >= 0 and f.max() < len(v)
    und, forward, backward = edge_uses(f)
    assert (forward == 1).all() and (backward == 1).all(), "an edge is not shared by exactly two triangles, once in each direction"
    assert len(v) - len(und) + len(f) == 2, (len(v), len(und), len(f))
    assert len(np.unique(f)) == len(v)
    normal = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    centroid = v[f].mean(1) - np.array(SPHERE_C)
    dots = (normal * centroid).sum(1)
    area = 0.5 * np.linalg.norm(normal, axis=1)
    assert (dots[area > 1e-12 * voxel * voxel] > 0).all(), "a triangle faces inwards"
    off = np.abs(np.linalg.norm(v - np.array(SPHERE_C), axis=1) - SPHERE_R)
    assert off.max() < voxel * voxel / SPHERE_R, (off.max(), voxel * voxel / SPHERE_R)
    return float(area.sum())


def assert_open_surface(result_faces, face_cells, cell_valid):
    """no triangle in an invalid cell; every edge in one or two triangles, never twice in one direction; a boundary exists"""
    assert cell_valid.reshape(-1)[face_cells].all()
    und, forward, backward = edge_uses(result_faces)
    assert (forward <= 1).all() and (backward <= 1).all()
    assert ((forward + backward) == 1).any() and ((forward + backward) == 2).any()


# ------------------------------------------------------------------------------------------------ argument refusals
def assert_refusals(hip):
    """every MNERF_E_* the header names for the two entry points, from fake addresses: each call fails its checks, or has nothing
    to launch, before any HIP call"""
    import ctypes as C
    lib = hip.load()
    fake, odd = C.c_void_p(0x10000), C.c_void_p(0x10004)
    fake_i32 = C.cast(fake, C.POINTER(C.c_int32))
    views = hip.view_array([hip.make_view(c["extr"], c["intr"], c["near"], c["far"]) for c in F.arc_cameras(3, 8, 8)])
    singular = hip.view_array([hip.make_view(np.zeros((3, 4), np.float32), c["intr"], c["near"], c["far"]) for c in F.arc_cameras(1, 8, 8)])
    nan, inf = float("nan"), float("inf")

    def integrate(views=views, n_views=3, h=8, w=8, depth=fake, opacity=None, counts=None, rgb=fake, min_opacity=0.5, trunc=0.1,
                  origin=(0.0, 0.0, 0.0), voxel=0.1, dims=(4, 4, 4), sums=fake, weight=fake):
        return lib.mnerf_tsdf_integrate(views, n_views, h, w, 1, depth, opacity, counts, 1, rgb, min_opacity, trunc, *origin, voxel, *dims,
                                        sums, weight, None)

    r, n, a = hip.MNERF_E_RANGE, hip.MNERF_E_NULL, hip.MNERF_E_ALIGN
    for want, kwargs in [(r, dict(n_views=0)), (r, dict(n_views=hip.MNERF_MAX_VIEWS + 1)), (r, dict(h=0)), (r, dict(w=0)),
                         (r, dict(h=1 << 16, w=1 << 15)), (r, dict(trunc=0.0)), (r, dict(trunc=nan)), (r, dict(trunc=inf)),
                         (r, dict(opacity=fake, min_opacity=nan)), (r, dict(dims=(-1, 4, 4))), (r, dict(dims=(2048, 1024, 1024))),
                         (r, dict(voxel=0.0)), (r, dict(voxel=nan)), (r, dict(origin=(0.0, inf, 0.0))),
                         (r, dict(views=singular, n_views=1)), (n, dict(views=None)), (n, dict(depth=None)), (n, dict(rgb=None)),
                         (n, dict(sums=None)), (n, dict(weight=None)), (a, dict(sums=odd)), (a, dict(weight=C.c_void_p(0x10002))),
                         (hip.MNERF_OK, dict(dims=(4, 0, 4), sums=None, weight=None, depth=None))]:
        assert integrate(**kwargs) == want, (kwargs, lib.mnerf_last_error())

    def mesh(sums=fake, weight=fake, origin=(0.0, 0.0, 0.0), voxel=0.1, dims=(4, 4, 4), min_weight=1.0, vertices=fake, vcap=8,
             triangles=fake_i32, tcap=8, counts=fake, workspace=fake):
        return lib.mnerf_tsdf_mesh(sums, weight, *origin, voxel, *dims, min_weight, vertices, vcap, triangles, tcap, counts, workspace, None)

    odd_i32 = C.cast(C.c_void_p(0x10002), C.POINTER(C.c_int32))
    for want, kwargs in [(r, dict(dims=(4, -1, 4))), (r, dict(dims=(1024, 1024, 256))), (r, dict(voxel=-1.0)), (r, dict(voxel=inf)),
                         (r, dict(origin=(nan, 0.0, 0.0))), (r, dict(min_weight=0.0)), (r, dict(min_weight=nan)), (r, dict(vcap=-1)),
                         (r, dict(tcap=-1)), (n, dict(sums=None)), (n, dict(weight=None)), (n, dict(counts=None)),
                         (n, dict(workspace=None)), (n, dict(vertices=None)), (n, dict(triangles=None)), (a, dict(sums=odd)),
                         (a, dict(vertices=odd)), (a, dict(counts=odd)), (a, dict(weight=C.c_void_p(0x10002))),
                         (a, dict(triangles=odd_i32)), (a, dict(workspace=C.c_void_p(0x10002))),
                         (hip.MNERF_OK, dict(dims=(0, 4, 4), sums=None, weight=None, counts=None, workspace=None, vertices=None,
                                             triangles=None))]:
        assert mesh(**kwargs) == want, (kwargs, lib.mnerf_last_error())
    # the workspace formula of the header
    for dims in ((1, 1, 1), (12, 11, 13), (64, 64, 64), (65, 64, 64), (256, 256, 256)):
        points = dims[0] * dims[1] * dims[2]
        blocks = -(-points // 256)
        tiles = -(-blocks // 1024)
        assert hip.tsdf_mesh_workspace_bytes(dims) == (4 * (points + 2 * blocks + 2 * tiles) + 2 * points + 15) // 16 * 16, dims
    assert hip.tsdf_mesh_workspace_bytes((0, 5, 5)) == 0 and hip.tsdf_mesh_workspace_bytes((-1, 5, 5)) == -1
    assert hip.tsdf_mesh_workspace_bytes((1024, 1024, 256)) == -1


# ------------------------------------------------------------------------------------------------ PLY
def read_ply(path):
    """-> (xyz float32 [M,3], rgb uint8 [M,3], faces int32 [T,3] or None) of a binary little-endian PLY of float xyz + uchar rgb
    vertices and, optionally, a face element of uchar-counted int lists (triangles only)"""
    with open(path, "rb") as f:
        blob = f.read()
    end = blob.index(b"end_header\n") + len(b"end_header\n")
    lines = blob[:end].decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0", lines[:2]
    elements = [l.split()[1:] for l in lines if l.startswith("element")]
    count = int(elements[0][1])
    assert elements[0][0] == "vertex" and len(elements) <= 2
    props = [l.split()[1:] for l in lines if l.startswith("property")]
    assert props[:6] == [["float", "x"], ["float", "y"], ["float", "z"], ["uchar", "red"], ["uchar", "green"], ["uchar", "blue"]], props
    body = np.frombuffer(blob[end:end + 15 * count], dtype=[("xyz", "<f4", 3), ("rgb", "u1", 3)])
    assert len(body) == count
    if len(elements) == 1:
        assert props[6:] == [] and len(blob) - end == 15 * count
        return body["xyz"].copy(), body["rgb"].copy(), None
    assert elements[1][0] == "face" and props[6:] == [["list", "uchar", "int", "vertex_indices"]], (elements, props[6:])
    n_faces = int(elements[1][1])
    faces = np.frombuffer(blob[end + 15 * count:], dtype=[("n", "u1"), ("v", "<i4", 3)])
    assert len(faces) == n_faces and len(blob) - end == 15 * count + 13 * n_faces and (faces["n"] == 3).all()
    return body["xyz"].copy(), body["rgb"].copy(), faces["v"].copy()
