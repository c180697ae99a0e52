"""Mesh finishing (include/mnerf.h "MESH FINISHING") restated in numpy: adjacency, connected components, compaction, Taubin smoothing
and vertex normals, operation by operation after the header's text.  The integer results are exact; the float ones take ``dtype``
float64 (the reference) or float32 (the device's format, whose distance from float64 sizes the gates), always from the SAME fp32
vertex rows, with every sum in the header's order (a vertex's corners ascending).  Where the header says fma() the float32 run rounds
once (the product and sum formed in float64, which holds them to well below half an fp32 ulp).

The meshes of the tests are built here too: the mesher's spheres (tests/mesh_helpers.py), a volume of two spheres, and hand-built
meshes (a fan, strips, degenerate and non-manifold corners)."""
import functools

import numpy as np

import mesh_helpers as M

INTERIOR, BOUNDARY = 1, 0
LAMBDA, MU = 0.5, -0.53


# ------------------------------------------------------------------------------------------------ 1. adjacency
def corner_tables(faces):
    """-> (next vertex, prev vertex) of every corner 3 t + k"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return f[:, [1, 2, 0]].reshape(-1), f[:, [2, 0, 1]].reshape(-1)


def adjacency(faces, n_vertices):
    """-> offsets int32 [V + 1], corners int32 [3 T] (every row ascending), vertex_class uint8 [V]"""
    flat = np.asarray(faces, np.int64).reshape(-1)
    counts = np.bincount(flat, minlength=n_vertices)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    corners = np.argsort(flat, kind="stable").astype(np.int32)  # by vertex, corners ascending inside a vertex
    nxt, prv = corner_tables(faces)
    # interior: the row's next vertices and its prev vertices are the same SET and none repeats
    owner = flat[corners]
    a, b = nxt[np.lexsort((nxt, flat))], prv[np.lexsort((prv, flat))]
    bad = a != b
    bad[1:] |= (a[1:] == a[:-1]) & (owner[1:] == owner[:-1])
    flaws = np.bincount(owner, weights=bad, minlength=n_vertices)
    return offsets, corners, ((counts > 0) & (flaws == 0)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ 2. components
def components(faces, n_vertices, min_triangles=0, min_fraction=0.0):
    """plain union-find -> labels int32 [V] (the smallest vertex row of the component), keep uint8 [V], triangles per label [V]"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    parent = list(range(n_vertices))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b, c in f.tolist():
        for q in (b, c):
            ra, rb = find(a), find(q)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    labels = np.array([find(v) for v in range(n_vertices)], np.int64).reshape(-1)
    count = np.bincount(labels[f[:, 0]], minlength=n_vertices) if len(f) else np.zeros(n_vertices, np.int64)
    largest = int(count.max()) if n_vertices else 0
    n = count[labels]
    keep = (n >= int(min_triangles)) & (n.astype(np.float64) >= np.float64(min_fraction) * np.float64(largest))
    return labels.astype(np.int32), keep.astype(np.uint8), count


# ------------------------------------------------------------------------------------------------ 3. compaction
def compact(vertices, faces, keep):
    """-> (the kept rows, the kept faces re-numbered): a face is kept iff its first vertex is"""
    keep = np.asarray(keep).astype(bool)
    f = np.asarray(faces).reshape(-1, 3)
    new = np.cumsum(keep) - 1
    kept = f[keep[f[:, 0]]] if len(f) else f
    return np.asarray(vertices)[keep], new[kept].astype(np.int32).reshape(-1, 3)


# ------------------------------------------------------------------------------------------------ float helpers
def fma(a, b, c, dtype):
    if dtype is np.float32:
        return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)
    return a * b + c


def _row_sum(offsets, lengths, corners, select, term, width, dtype):
    """[V, width]: for every vertex of ``select`` the sum of term(corner ids) over its row, ascending"""
    s = np.zeros((len(lengths), width), dtype)
    for j in range(int(lengths[select].max()) if select.any() else 0):
        sel = select & (lengths > j)
        s[sel] = s[sel] + term(corners[offsets[:-1][sel] + j])
    return s


# ------------------------------------------------------------------------------------------------ 4. smoothing
def smooth(vertices, faces, adj, iterations, lam=LAMBDA, mu=MU, dtype=np.float64):
    """-> positions [V, 3] (dtype) after ``iterations`` rounds; the factors are the fp32 values the kernel is given"""
    offsets, corners, vclass = (np.asarray(x) for x in adj)
    offsets, corners = offsets.astype(np.int64), corners.astype(np.int64)
    lengths = np.diff(offsets)
    interior = vclass == INTERIOR
    nxt, prv = corner_tables(faces)
    p = np.asarray(vertices)[:, :3].astype(dtype)
    for _ in range(iterations):
        for factor in (lam, mu):
            factor = dtype(np.float32(factor))
            if factor == 0:
                continue
            s = _row_sum(offsets, lengths, corners, interior, lambda c: p[nxt[c]] + p[prv[c]], 3, dtype)
            m = s[interior] / (2 * lengths[interior]).astype(dtype)[:, None]
            q = p.copy()
            q[interior] = fma(factor, m - p[interior], p[interior], dtype)
            p = q
    return p


# ------------------------------------------------------------------------------------------------ 5. normals
def normals(vertices, faces, adj, dtype=np.float64):
    """-> [V, 4] (dtype): nx ny nz a"""
    offsets, corners = np.asarray(adj[0]).astype(np.int64), np.asarray(adj[1]).astype(np.int64)
    lengths = np.diff(offsets)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    p = np.asarray(vertices)[:, :3].astype(dtype)
    n_vertices = len(p)
    if len(f):
        u, v = p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]]
        cross = np.stack([fma(u[:, a], v[:, b], -(u[:, b] * v[:, a]), dtype) for a, b in ((1, 2), (2, 0), (0, 1))], 1)
        norm = np.sqrt(fma(cross[:, 2], cross[:, 2], fma(cross[:, 1], cross[:, 1], cross[:, 0] * cross[:, 0], dtype), dtype))
        term = np.concatenate([cross, norm[:, None]], 1).astype(dtype)
    else:
        term = np.zeros((0, 4), dtype)
    s = _row_sum(offsets, lengths, corners, np.ones(n_vertices, bool), lambda c: term[c // 3], 4, dtype)
    length = np.sqrt(fma(s[:, 2], s[:, 2], fma(s[:, 1], s[:, 1], s[:, 0] * s[:, 0], dtype), dtype))
    out = np.zeros((n_vertices, 4), dtype)
    ok = length > 0
    out[ok, :3] = s[ok, :3] / length[ok, None]
    out[:, 3] = s[:, 3] / dtype(6)
    return out


def normal_distance(got, want):
    """-> (the largest difference of a component of n, the largest difference of a relative to the largest a)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if not len(want):
        return 0.0, 0.0
    return float(np.abs(got[:, :3] - want[:, :3]).max()), float(np.abs(got[:, 3] - want[:, 3]).max() / max(want[:, 3].max(), 1e-300))


def position_distance(got, want, extent):
    return float(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max() / extent) if len(want) else 0.0


def extent_of(vertices):
    p = np.asarray(vertices, np.float64)[:, :3]
    return float((p.max(0) - p.min(0)).max())


# ------------------------------------------------------------------------------------------------ meshes
def rows_of(positions, seed=0):
    """positions [V, 3] -> fp32 rows x y z w | r g b 0 with seeded weights and colours"""
    positions = np.asarray(positions, np.float64).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    rows = np.zeros((len(positions), 8), np.float32)
    rows[:, :3] = positions
    rows[:, 3] = 2.0 + rng.random(len(positions))
    rows[:, 4:7] = rng.random((len(positions), 3))
    return rows


@functools.lru_cache(maxsize=None)
def sphere(dims, open_octant=False):
    """the restatement's sphere mesh as fp32 rows -> (vertices [V, 8] f32, faces [T, 3] int32, voxel)"""
    m = M.sphere_mesh(dims, open_octant)
    return m["vertices"].astype(np.float32), m["faces"], M.sphere_grid(dims)[1]


TWO_SPHERES = dict(dims=M.DIMS, origin=(0.0, 0.0, 0.0), voxel=0.1, big=((0.83, 0.87, 0.77), 0.41), small=((0.91, 0.79, 1.76), 0.153))


@functools.lru_cache(maxsize=None)
def two_sphere_volume():
    """two spheres that do not touch, radii of about 4 and 1.5 voxels, on the 19 x 17 x 23 grid: d = the smaller of the two distances
    -> dict(sums, weight, origin, voxel) as mesh_helpers.sphere_volume"""
    t = TWO_SPHERES
    p = M.centres(t["origin"], t["voxel"], t["dims"], np.float64)
    d = np.minimum(*[np.linalg.norm(p - (np.array(c) + 0.01 * np.array(M.SPHERE_C)), axis=-1) - r for c, r in (t["big"], t["small"])])
    colour = 0.5 + 0.5 * np.sin(3.0 * p)
    sums = np.concatenate([(3.0 * d / (4.0 * t["voxel"]))[..., None], 3.0 * colour], -1).astype(np.float32)
    assert (sums[..., 0] != 0).all()
    return dict(sums=sums, weight=np.full(d.shape, 3.0, np.float32), origin=t["origin"], voxel=t["voxel"])


@functools.lru_cache(maxsize=None)
def two_spheres():
    """the restatement's mesh of the two-sphere volume -> (vertices f32, faces)"""
    vol = two_sphere_volume()
    m = M.mesh(vol["sums"], vol["weight"], vol["origin"], vol["voxel"], 2.0)
    return m["vertices"].astype(np.float32), m["faces"]


def fan(n=40):
    """n triangles round vertex 0, closed: the centre is interior with valence n, the rim is boundary"""
    angle = 2 * np.pi * np.arange(n) / n
    rim = np.stack([np.cos(angle), np.sin(angle), 0.1 * np.sin(3 * angle)], 1)
    faces = np.array([[0, 1 + i, 1 + (i + 1) % n] for i in range(n)], np.int32)
    return rows_of(np.concatenate([[[0.013, -0.021, 0.3]], rim]), 1), faces


@functools.lru_cache(maxsize=None)
def strip(n_vertices, seed=None, segments=False):
    """a zigzag strip over n_vertices vertices, consistently wound.  ``seed``: the vertex rows are a seeded permutation of the order
    along the strip (deep union-find chains).  ``segments``: the strip is cut into pieces of 3..60 vertices (seeded): components of
    many sizes."""
    i = np.arange(n_vertices - 2)
    tri = np.stack([i, np.where(i % 2 == 0, i + 1, i + 2), np.where(i % 2 == 0, i + 2, i + 1)], 1)
    rng = np.random.default_rng(0 if seed is None else seed)
    if segments:
        ends = np.cumsum(rng.integers(3, 61, n_vertices // 3 + 1))  # a piece ends before vertex `end`
        piece = np.searchsorted(ends, np.arange(n_vertices), side="right")
        tri = tri[piece[tri[:, 0]] == piece[tri[:, 0] + 2]]
    k = np.arange(n_vertices)
    pos = np.stack([0.5 * k, (k % 2) * 1.0 + 0.05 * np.sin(0.37 * k), 0.2 * np.cos(0.11 * k)], 1)
    if seed is not None:
        perm = rng.permutation(n_vertices)
        tri = perm[tri]
        placed = np.zeros_like(pos)
        placed[perm] = pos
        pos = placed
    return rows_of(pos, 2), tri.astype(np.int32)


def degenerate():
    """two real triangles; the zero-area triangle (1 4 5) of three collinear points, whose vertices 4 and 5 have no other triangle; the
    unreferenced vertex 6"""
    pos = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0.25), (2, 0, 0), (3, 0, 0), (5, 5, 5)]
    return rows_of(pos, 3), np.array([[0, 1, 2], [1, 3, 2], [1, 4, 5]], np.int32)


def non_manifold():
    """two triangles that share the edge 0 -> 1 in the same direction"""
    pos = [(0, 0, 0), (1, 0, 0), (0.5, 1, 0), (0.5, -0.2, 1)]
    return rows_of(pos, 4), np.array([[0, 1, 2], [0, 1, 3]], np.int32)


SCAN_BLOCK, SCAN_TILE = 256, 256 * 1024  # vertices per workgroup / per tile of the compaction's scan
BOUNDARY_SIZES = (SCAN_BLOCK - 1, SCAN_BLOCK + 1, SCAN_TILE - 1, SCAN_TILE + 1)


def small_meshes():
    """name -> (vertices, faces): every mesh the integer results are compared on, but for the large strips"""
    out = {"sphere": sphere((12, 11, 13))[:2], "sphere_open": sphere((12, 11, 13), True)[:2], "sphere24": sphere((24, 24, 24))[:2],
           "two_spheres": two_spheres(), "fan": fan(), "strip5000": strip(5002, 11), "degenerate": degenerate(),
           "non_manifold": non_manifold()}
    for n in BOUNDARY_SIZES[:2]:
        out[f"strip{n}"] = strip(n, None, True)
    return out


def radial_rms(positions, voxel):
    """the RMS distance from the restatement's sphere, in voxels"""
    r = np.linalg.norm(np.asarray(positions, np.float64)[:, :3] - np.array(M.SPHERE_C), axis=1) - M.SPHERE_R
    return float(np.sqrt((r * r).mean()) / voxel)


def noisy_sphere(dims, sigma=0.3, seed=5):
    """the sphere mesh with every vertex moved along its radius by seeded normal noise of ``sigma`` voxels"""
    vertices, faces, voxel = sphere(dims)
    radial = vertices[:, :3].astype(np.float64) - np.array(M.SPHERE_C)
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    out = vertices.copy()
    out[:, :3] = (vertices[:, :3] + radial * (sigma * voxel * np.random.default_rng(seed).standard_normal(len(vertices)))[:, None])
    return out, faces, voxel


# ------------------------------------------------------------------------------------------------ the workspace formula
def workspace_bytes(n_vertices, n_triangles):
    if n_vertices == 0:
        return 0
    bv, bt = -(-n_vertices // 256), -(-n_triangles // 256)
    tv, tt = -(-bv // 1024), -(-bt // 1024)
    return 16 + (max(4 * (n_vertices + bv + tv + bt + tt), 32 * n_vertices) + 15) // 16 * 16


# ------------------------------------------------------------------------------------------------ PLY with normals
def read_ply(path):
    """-> (xyz f32 [M, 3], normals f32 [M, 3] or None, rgb u8 [M, 3], faces int32 [T, 3] or None), the header's counts asserted
    against the body"""
    with open(path, "rb") as f:
        blob = f.read()
    end = blob.index(b"end_header\n") + len(b"end_header\n")
    lines = blob[:end].decode("ascii").splitlines()
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"], lines[:2]
    elements = [l.split()[1:] for l in lines if l.startswith("element")]
    props = [l.split()[1:] for l in lines if l.startswith("property")]
    xyz = [["float", n] for n in "xyz"]
    nrm = [["float", n] for n in ("nx", "ny", "nz")]
    rgb = [["uchar", n] for n in ("red", "green", "blue")]
    has_normals = props[3:6] == nrm
    n_vertex_props = 9 if has_normals else 6
    assert props[:n_vertex_props] == xyz + (nrm if has_normals else []) + rgb, props
    dtype = [("xyz", "<f4", 3)] + ([("n", "<f4", 3)] if has_normals else []) + [("rgb", "u1", 3)]
    count, size = int(elements[0][1]), np.dtype(dtype).itemsize
    assert elements[0][0] == "vertex" and size == (27 if has_normals else 15)
    body = np.frombuffer(blob[end:end + size * count], dtype=dtype)
    assert len(body) == count
    faces = None
    if len(elements) == 2:
        assert elements[1][0] == "face" and props[n_vertex_props:] == [["list", "uchar", "int", "vertex_indices"]]
        rec = np.frombuffer(blob[end + size * count:], dtype=[("n", "u1"), ("v", "<i4", 3)])
        assert len(rec) == int(elements[1][1]) and len(blob) - end == size * count + 13 * len(rec) and (rec["n"] == 3).all()
        faces = rec["v"].copy()
    else:
        assert len(elements) == 1 and props[n_vertex_props:] == [] and len(blob) - end == size * count
    return body["xyz"].copy(), body["n"].copy() if has_normals else None, body["rgb"].copy(), faces


# ------------------------------------------------------------------------------------------------ argument refusals
def assert_refusals(hip):
    """every MNERF_E_* the header names for the six entry points, from fake addresses: each call fails its checks, or has nothing to
    launch, before any HIP call"""
    import ctypes as C
    lib = hip.load()
    fake, odd4, odd16 = C.c_void_p(0x10000), C.c_void_p(0x10002), C.c_void_p(0x10008)
    i32 = lambda p: None if p is None else C.cast(p, C.POINTER(C.c_int32))
    r, n, a, ok = hip.MNERF_E_RANGE, hip.MNERF_E_NULL, hip.MNERF_E_ALIGN, hip.MNERF_OK
    nan, inf = float("nan"), float("inf")
    big_v, big_t = 1 << 31, ((1 << 31) - 1) // 3 + 1
    sizes = [(r, dict(v=-1)), (r, dict(t=-1)), (r, dict(v=big_v)), (r, dict(t=big_t))]

    def run(call, cases):
        for want, kwargs in cases:
            assert call(**kwargs) == want, (call.__name__, kwargs, want, lib.mnerf_last_error())

    def adjacency(tri=fake, v=8, t=4, offsets=fake, corners=fake, vclass=fake, ws=fake):
        return lib.mnerf_mesh_adjacency(i32(tri), v, t, i32(offsets), i32(corners), vclass, ws, None)

    run(adjacency, sizes + [(n, dict(offsets=None)), (n, dict(vclass=None)), (n, dict(ws=None)), (n, dict(tri=None)), (n, dict(corners=None)),
                            (a, dict(tri=odd4)), (a, dict(offsets=odd4)), (a, dict(corners=odd4)), (a, dict(ws=odd16)),
                            (ok, dict(v=0, t=0, tri=None, offsets=None, corners=None, vclass=None, ws=None))])

    def components(tri=fake, v=8, t=4, min_t=0, frac=0.0, labels=fake, keep=fake, ws=fake):
        return lib.mnerf_mesh_components(i32(tri), v, t, min_t, frac, i32(labels), keep, ws, None)

    run(components, sizes + [(r, dict(min_t=-1)), (r, dict(frac=-0.1)), (r, dict(frac=1.5)), (r, dict(frac=nan)), (r, dict(frac=inf)),
                             (n, dict(labels=None)), (n, dict(keep=None)), (n, dict(ws=None)), (n, dict(tri=None)),
                             (a, dict(tri=odd4)), (a, dict(labels=odd4)), (a, dict(ws=odd16)),
                             (ok, dict(v=0, t=0, tri=None, labels=None, keep=None, ws=None))])

    def compact(vert=fake, tri=fake, v=8, t=4, keep=fake, vout=fake, vcap=8, tout=fake, tcap=4, counts=fake, ws=fake):
        return lib.mnerf_mesh_compact(vert, i32(tri), v, t, keep, vout, vcap, i32(tout), tcap, counts, ws, None)

    run(compact, sizes + [(r, dict(vcap=-1)), (r, dict(tcap=-1)), (n, dict(vert=None)), (n, dict(keep=None)), (n, dict(counts=None)),
                          (n, dict(ws=None)), (n, dict(tri=None)), (n, dict(vout=None)), (n, dict(tout=None)), (a, dict(vert=odd16)),
                          (a, dict(vout=odd16)), (a, dict(ws=odd16)), (a, dict(tri=odd4)), (a, dict(tout=odd4)), (a, dict(counts=odd4)),
                          (ok, dict(v=0, t=0, vert=None, tri=None, keep=None, vout=None, tout=None, counts=None, ws=None))])

    def smooth(vin=fake, v=8, tri=fake, t=4, offsets=fake, corners=fake, vclass=fake, it=1, lam=0.5, mu=-0.53, vout=fake, ws=fake):
        return lib.mnerf_mesh_smooth(vin, v, i32(tri), t, i32(offsets), i32(corners), vclass, it, lam, mu, vout, ws, None)

    run(smooth, sizes + [(r, dict(it=-1)), (r, dict(lam=0.0)), (r, dict(lam=-0.5)), (r, dict(lam=1.5)), (r, dict(lam=nan)),
                         (r, dict(mu=0.1)), (r, dict(mu=nan)), (r, dict(mu=-inf)), (n, dict(vin=None)), (n, dict(vout=None)),
                         (n, dict(offsets=None)), (n, dict(vclass=None)), (n, dict(ws=None)), (n, dict(tri=None)), (n, dict(corners=None)),
                         (a, dict(vin=odd16)), (a, dict(vout=odd16)), (a, dict(ws=odd16)), (a, dict(tri=odd4)), (a, dict(offsets=odd4)),
                         (a, dict(corners=odd4)),
                         (ok, dict(v=0, t=0, vin=None, tri=None, offsets=None, corners=None, vclass=None, vout=None, ws=None))])

    def normals(vert=fake, v=8, tri=fake, t=4, offsets=fake, corners=fake, out=fake):
        return lib.mnerf_mesh_normals(vert, v, i32(tri), t, i32(offsets), i32(corners), out, None)

    run(normals, sizes + [(n, dict(vert=None)), (n, dict(offsets=None)), (n, dict(out=None)), (n, dict(tri=None)), (n, dict(corners=None)),
                          (a, dict(vert=odd16)), (a, dict(out=odd16)), (a, dict(tri=odd4)), (a, dict(offsets=odd4)), (a, dict(corners=odd4)),
                          (ok, dict(v=0, t=0, vert=None, tri=None, offsets=None, corners=None, out=None))])

    for v, t in ((1, 0), (1, 1), (521, 1038), (255, 253), (257, 255), (SCAN_TILE + 1, SCAN_TILE - 1), (10, 100000), (3, 715827882)):
        assert hip.mesh_finish_workspace_bytes(v, t) == workspace_bytes(v, t), (v, t)
    assert hip.mesh_finish_workspace_bytes(0, 0) == 0 and hip.mesh_finish_workspace_bytes(-1, 0) == -1
    assert hip.mesh_finish_workspace_bytes(big_v, 0) == -1 and hip.mesh_finish_workspace_bytes(8, big_t) == -1
