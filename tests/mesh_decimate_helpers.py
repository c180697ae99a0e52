"""Mesh decimation (include/mnerf.h "mnerf_mesh_decimate") restated in numpy, operation by operation after the header's text: the fp32
cell index, the cell -> vertex rows, the float64 plane quadrics summed in the stated orders (a vertex's corners ascending, a cell's
members ascending), the regularised minimiser (numpy.linalg.solve in float64), the clamp to the cell, and the first-of-its-set rule
for the triangles through a dict.  Meshes and the adjacency's layout are those of tests/mesh_finish_helpers.py."""
import numpy as np

import mesh_finish_helpers as H

REG = 1.0 / 1000  # 1 / MNERF_DECIMATE_REG_INV


def corner_rows(faces, n_vertices):
    """offsets int32 [V + 1], corners int32 [<= 3 T] as mnerf_mesh_adjacency writes them: a corner whose index is outside [0, V) joins no
    row (for a mesh without such corners: the first two arrays of mesh_finish_helpers.adjacency)"""
    flat = np.asarray(faces, np.int64).reshape(-1)
    ids = np.nonzero((flat >= 0) & (flat < n_vertices))[0]
    corners = ids[np.argsort(flat[ids], kind="stable")]
    offsets = np.concatenate([[0], np.cumsum(np.bincount(flat[ids], minlength=n_vertices))])
    return offsets.astype(np.int32), corners.astype(np.int32)


def cell_index(vertices, origin, cell, dims):
    """the linear cell of every vertex, int64 [V]; -1 for a row with a non-finite x, y or z.  fp32: the subtraction and the division
    are rounded on their own; floor and clamp are exact"""
    p = np.asarray(vertices, np.float32)[:, :3]
    finite = np.isfinite(p).all(1)
    with np.errstate(over="ignore", invalid="ignore"):
        q = (p - np.asarray(origin, np.float32)) / np.float32(cell)
    assert q.dtype == np.float32
    f = np.where(finite[:, None], np.floor(q).astype(np.float64), 0.0)
    i = np.clip(f, 0.0, np.asarray(dims, np.float64) - 1.0).astype(np.int64)
    return np.where(finite, (i[:, 2] * int(dims[1]) + i[:, 1]) * int(dims[0]) + i[:, 0], -1)


def cell_centres(cells, origin, cell, dims):
    """float64 [n, 3]: origin + (index + 0.5) cell, from the fp32 arguments"""
    cells = np.asarray(cells, np.int64)
    ijk = np.stack([cells % dims[0], (cells // dims[0]) % dims[1], cells // (dims[0] * dims[1])], 1).astype(np.float64)
    return np.asarray(origin, np.float32).astype(np.float64) + (ijk + 0.5) * np.float64(np.float32(cell))


def decimate(vertices, faces, origin, cell, dims):
    """-> dict: vertices f32 [V', 8], faces int32 [T', 3], vertex_map int32 [V], cells int64 [V'] (the occupied cells, ascending), and
    what the tests of the representative read: centres, half, count, A [V', 3, 3], b, mean, x (float64, relative to the centres; x
    after the clamp)"""
    vertices = np.asarray(vertices, np.float32).reshape(-1, 8)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    n_vertices = len(vertices)
    dims = tuple(int(d) for d in dims)
    lin = cell_index(vertices, origin, cell, dims)
    cells, compact = np.unique(lin[lin >= 0], return_inverse=True)
    vertex_map = np.full(n_vertices, -1, np.int64)
    vertex_map[lin >= 0] = compact
    n_new = len(cells)
    centres = cell_centres(cells, origin, cell, dims)
    # the cell -> vertex rows: members ascending
    placed = np.nonzero(lin >= 0)[0]
    members = placed[np.argsort(vertex_map[placed], kind="stable")]
    cell_offsets = np.concatenate([[0], np.cumsum(np.bincount(vertex_map[placed], minlength=n_new))]).astype(np.int64)
    count = np.diff(cell_offsets)
    # the plane of every corner's triangle, relative to the centre of the CORNER'S VERTEX'S cell
    pos = vertices[:, :3].astype(np.float64)
    offsets, corners = (a.astype(np.int64) for a in corner_rows(faces, n_vertices))
    term = np.zeros((3 * len(faces), 9))
    in_range = ((faces >= 0) & (faces < n_vertices)).all(1)
    safe = np.where(in_range[:, None], faces, 0)
    usable = in_range & np.isfinite(pos[safe]).all((1, 2))
    for k in range(3):
        owner = safe[:, k]
        ok = usable & (lin[owner] >= 0)
        g = centres[vertex_map[owner[ok]]]
        p0, p1, p2 = (pos[safe[ok, j]] - g for j in range(3))
        u, t = p1 - p0, p2 - p0
        n = np.stack([u[:, 1] * t[:, 2] - u[:, 2] * t[:, 1], u[:, 2] * t[:, 0] - u[:, 0] * t[:, 2], u[:, 0] * t[:, 1] - u[:, 1] * t[:, 0]], 1)
        d = -((n[:, 0] * p0[:, 0] + n[:, 1] * p0[:, 1]) + n[:, 2] * p0[:, 2])
        rows = np.stack([n[:, 0] * n[:, 0], n[:, 0] * n[:, 1], n[:, 0] * n[:, 2], n[:, 1] * n[:, 1], n[:, 1] * n[:, 2], n[:, 2] * n[:, 2],
                         d * n[:, 0], d * n[:, 1], d * n[:, 2]], 1)
        term[3 * np.nonzero(ok)[0] + k] = rows
    lengths = np.diff(offsets)
    quadric = H._row_sum(offsets, lengths, corners, lin >= 0, lambda c: term[c], 9, np.float64)  # per vertex, corners ascending
    own = np.zeros((n_vertices, 7))
    own[placed, :3] = pos[placed] - centres[vertex_map[placed]]
    own[placed, 3:] = vertices[placed][:, 3:7].astype(np.float64)
    every = np.ones(n_new, bool)
    q = H._row_sum(cell_offsets, count, members, every, lambda v: quadric[v], 9, np.float64)  # per cell, members ascending
    s = H._row_sum(cell_offsets, count, members, every, lambda v: own[v], 7, np.float64)
    mean = s / count[:, None].astype(np.float64)
    a = q[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)
    b = q[:, 6:9]
    lam = REG * ((q[:, 0] + q[:, 3]) + q[:, 5])
    x = mean[:, :3].copy()
    solved = lam > 0
    if solved.any():
        lhs = a[solved] + lam[solved, None, None] * np.eye(3)
        x[solved] = np.linalg.solve(lhs, (lam[solved, None] * mean[solved, :3] - b[solved])[..., None])[..., 0]
    half = 0.5 * np.float64(np.float32(cell))
    x = np.fmin(np.fmax(x, -half), half)
    out = np.zeros((n_new, 8), np.float32)
    out[:, :3] = (centres + x).astype(np.float32)
    out[:, 3:7] = mean[:, 3:].astype(np.float32)
    # the triangles: candidates, the first of every set of new rows
    new = np.where(in_range[:, None], vertex_map[safe], -1)
    candidate = (new >= 0).all(1) & (new[:, 0] != new[:, 1]) & (new[:, 1] != new[:, 2]) & (new[:, 0] != new[:, 2])
    seen, kept = {}, []
    for t in np.nonzero(candidate)[0].tolist():
        key = tuple(sorted(new[t].tolist()))
        if key not in seen:
            seen[key] = t
            kept.append(t)
    return dict(vertices=out, faces=new[kept].astype(np.int32).reshape(-1, 3), vertex_map=vertex_map.astype(np.int32), cells=cells,
                centres=centres, half=half, count=count, A=a, b=b, mean=mean[:, :3], x=x, lam=lam)


def mean_edge(vertices, faces):
    """the mean edge length of the triangles whose indices are in range and whose vertices are finite"""
    vertices, faces = np.asarray(vertices, np.float64), np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((faces >= 0) & (faces < len(vertices))).all(1)
    p = vertices[faces[ok]][:, :, :3]
    e = np.linalg.norm(p - p[:, [1, 2, 0]], axis=2)
    return float(e[np.isfinite(e)].mean())


def grid_of(vertices, cell, pad=0.25):
    """a grid of `cell` over the finite bounding box, its origin `pad` cells below the box's corner -> (origin fp32 triple, cell, dims)"""
    p = np.asarray(vertices, np.float64)[:, :3]
    p = p[np.isfinite(p).all(1)]
    lo = (p.min(0) - pad * cell).astype(np.float32)
    dims = tuple(int(d) for d in np.maximum(1, np.floor((p.max(0) - lo.astype(np.float64)) / cell).astype(np.int64) + 1))
    return tuple(float(x) for x in lo), float(np.float32(cell)), dims


def one_ulp_apart(got, want):
    """boolean [..]: every fp32 component of `got` is `want` or one of its two neighbours"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    return (got == want) | (got == np.nextafter(want, np.float32(np.inf))) | (got == np.nextafter(want, np.float32(-np.inf)))


def workspace_bytes(n_vertices, n_triangles, dims):
    if n_vertices == 0:
        return 0
    n = int(dims[0]) * int(dims[1]) * int(dims[2])
    blocks = lambda k: -(-k // 256)
    tiles = lambda k: -(-blocks(k) // 1024)
    ints = 4 * n_vertices + 2 * n + 2 + 6 * n_triangles + sum(blocks(k) + tiles(k) for k in (n, n_vertices, n_triangles))
    return (16 + 4 * ints + n_triangles + 15) // 16 * 16


def lattice_strip(n_vertices=200, spacing=0.5):
    """the zigzag strip with every vertex ON a lattice point of `spacing` (seeded permutation of the rows): with a cell of half the
    spacing every vertex is alone in its cell -> (vertices, faces, (origin, cell, dims))"""
    vertices, faces = H.strip(n_vertices, 7)
    vertices = vertices.copy()
    vertices[:, :3] = np.round(vertices[:, :3] / spacing) * spacing + 0.0  # (+ 0.0: no negative zero, which no sum g + x returns)
    cell = 0.5 * spacing
    origin = tuple(float(x) for x in vertices[:, :3].min(0) - 0.25 * cell)
    dims = tuple(int(d) for d in np.floor((vertices[:, :3].max(0) - np.array(origin)) / cell).astype(np.int64) + 1)
    return vertices, faces, (origin, cell, dims)


def plane_patch(n=12, seed=3):
    """an n x n triangulated patch of the plane z = x / 2 + y / 4 + 3 / 8 over jittered multiples of 1 / 64: every fp32 row satisfies
    the equation EXACTLY -> (vertices, faces)"""
    rng = np.random.default_rng(seed)
    ij = np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 2) * 16 + rng.integers(0, 10, (n * n, 2))
    xy = ij / 64.0
    pos = np.concatenate([xy, 0.5 * xy[:, :1] + 0.25 * xy[:, 1:] + 0.375], 1)
    vertices = H.rows_of(pos, 5)
    assert np.array_equal(vertices[:, :3].astype(np.float64), pos)
    idx = np.arange(n * n).reshape(n, n)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    return vertices, np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]).astype(np.int32)


def cube_corner(n=4, side=1.0, seed=9):
    """three mutually orthogonal n x n faces of a cube that meet at `corner`, triangulated, welded along the shared edges; the corner
    is NOT a lattice point of the test's grid -> (vertices, faces, corner)"""
    corner = np.array([0.313, -0.207, 0.125])
    step = side / n
    index, pos, faces = {}, [], []

    def vertex(p):
        key = tuple(int(round(c)) for c in p)
        if key not in index:
            index[key] = len(pos)
            pos.append(corner + step * np.array(key, np.float64))
        return index[key]

    for axis in range(3):  # the face perpendicular to `axis`, through the corner, spanned by the other two axes
        e1, e2 = np.eye(3)[(axis + 1) % 3], np.eye(3)[(axis + 2) % 3]
        for i in range(n):
            for j in range(n):
                q = [vertex(i * e1 + j * e2), vertex((i + 1) * e1 + j * e2), vertex((i + 1) * e1 + (j + 1) * e2), vertex(i * e1 + (j + 1) * e2)]
                faces += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    return H.rows_of(np.array(pos), seed), np.array(faces, np.int32), corner


def dropped_case():
    """by hand: vertices 0 1 2 and 3 4 5 pairwise share three cells, 6 has a NaN, 7 sits in a fourth cell.  Faces: (0 1 2); (3 5 4), the
    same three cells with the opposite winding; (4 5 7); (0 1 9) with an index >= V; (0 6 2) with the dropped vertex; (0 3 1), two
    corners in one cell; (7 5 1), the set of (4 5 7) again"""
    pos = [(0.2, 0.2, 0.2), (1.2, 0.3, 0.2), (0.3, 1.2, 0.1), (0.4, 0.1, 0.3), (1.4, 0.2, 0.4), (0.1, 1.4, 0.3), (np.nan, 0.5, 0.5), (1.5, 1.5, 0.2)]
    vertices = H.rows_of(np.nan_to_num(np.array(pos)), 6)
    vertices[6, 0] = np.nan
    faces = np.array([[0, 1, 2], [3, 5, 4], [4, 5, 7], [0, 1, 9], [0, 6, 2], [0, 3, 1], [7, 5, 1]], np.int32)
    return vertices, faces, (0.0, 0.0, 0.0), 1.0, (2, 2, 1)


def assert_refusals(hip):
    """every MNERF_E_* the header names for mnerf_mesh_decimate, from fake addresses: each call fails its checks, or has nothing to
    launch, before any HIP call; and the workspace formula"""
    import ctypes as C
    lib = hip.load()
    fake, odd4, odd16 = C.c_void_p(0x10000), C.c_void_p(0x10002), C.c_void_p(0x10008)
    i32 = lambda p: None if p is None else C.cast(p, C.POINTER(C.c_int32))
    r, n, a, ok = hip.MNERF_E_RANGE, hip.MNERF_E_NULL, hip.MNERF_E_ALIGN, hip.MNERF_OK
    nan, inf = float("nan"), float("inf")
    big_v, big_t = 1 << 31, ((1 << 31) - 1) // 3 + 1

    def decimate(vert=fake, tri=fake, v=8, t=4, offsets=fake, corners=fake, origin=(0.0, 0.0, 0.0), cell=1.0, dims=(2, 2, 2), vout=fake,
                 vcap=8, tout=fake, tcap=4, vmap=fake, counts=fake, ws=fake):
        return lib.mnerf_mesh_decimate(vert, i32(tri), v, t, i32(offsets), i32(corners), *origin, cell, *dims, vout, vcap, i32(tout), tcap,
                                       i32(vmap), counts, ws, None)

    cases = [(r, dict(v=-1)), (r, dict(t=-1)), (r, dict(v=big_v)), (r, dict(t=big_t)), (r, dict(dims=(0, 2, 2))), (r, dict(dims=(2, -1, 2))),
             (r, dict(dims=(2, 2, 0))), (r, dict(dims=(2048, 1024, 1024))), (r, dict(dims=(65536, 65536, 1))), (r, dict(cell=0.0)),
             (r, dict(cell=-1.0)), (r, dict(cell=nan)), (r, dict(cell=inf)), (r, dict(origin=(nan, 0.0, 0.0))), (r, dict(origin=(0.0, inf, 0.0))),
             (r, dict(origin=(0.0, 0.0, -inf))), (r, dict(vcap=-1)), (r, dict(tcap=-1)),
             (r, dict(v=-1, vert=None)),  # RANGE precedes NULL
             (n, dict(vert=None)), (n, dict(counts=None)), (n, dict(ws=None)), (n, dict(offsets=None)), (n, dict(offsets=None, t=0)),
             (n, dict(tri=None)), (n, dict(corners=None)), (n, dict(vout=None)), (n, dict(tout=None)),
             (n, dict(vert=None, ws=odd16)),  # NULL precedes ALIGN
             (a, dict(vert=odd16)), (a, dict(vout=odd16)), (a, dict(ws=odd16)), (a, dict(tri=odd4)), (a, dict(offsets=odd4)),
             (a, dict(corners=odd4)), (a, dict(tout=odd4)), (a, dict(vmap=odd4)), (a, dict(counts=odd4)),
             (ok, dict(v=0, t=0, vert=None, tri=None, offsets=None, corners=None, vout=None, tout=None, vmap=None, counts=None, ws=None))]
    for want, kwargs in cases:
        assert decimate(**kwargs) == want, (kwargs, want, lib.mnerf_last_error())
    for v, t, dims in ((1, 0, (1, 1, 1)), (1, 1, (3, 1, 2)), (521, 1038, (7, 9, 5)), (255, 253, (257, 1, 1)), (H.SCAN_TILE + 1, H.SCAN_TILE - 1, (H.SCAN_TILE + 1, 1, 1)),
                       (10, 100000, (64, 64, 64)), (3, 715827882, (1, 1, 1)), (5, 2, (1290, 1290, 1290))):
        assert hip.mesh_decimate_workspace_bytes(v, t, dims) == workspace_bytes(v, t, dims), (v, t, dims)
    assert hip.mesh_decimate_workspace_bytes(0, 0, (4, 4, 4)) == 0
    for v, t, dims in ((-1, 0, (1, 1, 1)), (big_v, 0, (1, 1, 1)), (8, big_t, (1, 1, 1)), (8, 4, (0, 1, 1)), (8, 4, (1, 1, -1)), (8, 4, (2048, 1024, 1024)),
                       (0, 0, (0, 1, 1))):
        assert hip.mesh_decimate_workspace_bytes(v, t, dims) == -1, (v, t, dims)
