"""Mesh texture (include/mnerf.h "MESH TEXTURE") restated in numpy, operation by operation after the header's text, and the scene the
tests bake: the plane and the box of tests/fusion_helpers.py seen from the arc cameras, meshed by the restatements of
tests/mesh_helpers.py, coloured by an analytic world colour field.

``dtype`` selects the arithmetic (float64: the reference; float32: the same chain in the device's format, whose distance from
float64 shows that the GPU gate is reachable).  In float64 ``accumulate`` also marks the BORDERLINE texels, whose discrete decisions
fp32 may take differently: a camera-z within 1e-6 of 0, a projection within 1e-3 px of the frame rectangle or of a texel boundary
across which the validity of the four taps changes, a tap on a value edge (fusion_helpers.values), a relative depth error within 1e-5
of vis_rel_tol, a cosine within 1e-6 of 0, and - in best mode - two largest weights within 1e-6 relative of each other."""
import functools

import numpy as np

import fusion_helpers as F
import mesh_finish_helpers as H
import mesh_helpers as M

BORDERLINE_CAP = F.BORDERLINE_CAP
RGB_GATE = 1e-4  # the project's RGB gate
LAYOUT_T, LAYOUT_B = (0, 1, 2, 3, 7, 512, 513), (4, 5, 8, 64)
VIS_REL_TOL, POWER = 0.02, 2
# (K, h, w, legacy, variant, consistent): the integrator's frame sizes (16 = MNERF_MAX_VIEWS), every variant; and one case on the
# fused depths and their counts, which is what fusion.mesh feeds the texture.  (16, 37, 53, legacy, "invalid") is REPLACED by the same
# views at 30 x 40: with 16 views and the variant's planted texels 1.2 - 1.8 % of its atlas lie within 1e-3 px of a change of tap
# validity in SOME view, above the cap of 1 %; at 30 x 40 (another draw of the planted texels) it is 0.3 - 0.6 %.
REPLACED = {(16, 37, 53, True, "invalid"): (16, 30, 40, True, "invalid")}
CASES = [REPLACED.get((k, h, w, legacy, variant), (k, h, w, legacy, variant)) + (False,) for (k, h, w) in ((3, 24, 32), (16, 37, 53))
         for legacy in (True, False) for variant in F.VARIANTS] + [(3, 24, 32, False, "plain", True)]
BLOCKS = (4, 5, 8)


# ------------------------------------------------------------------------------------------------ 1. the atlas
def atlas_size(n_triangles, block):
    """-> (W, H, nbx, nby)"""
    nb = -(-n_triangles // 2)
    nbx = 0
    while nbx * nbx < nb:
        nbx += 1
    nby = -(-nb // nbx) if nbx else 0
    return nbx * block, nby * block, nbx, nby


def layout(n_triangles, block):
    """-> dict(W, H, owner int64 [H, W] (-1: none), i, j int64 [H, W]: the local texel the owner uses)"""
    width, height, nbx, _ = atlas_size(n_triangles, block)
    y, x = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    bx, by = x // block, y // block
    i, j = x - bx * block, y - by * block
    upper = i + j >= block
    owner = 2 * (by * nbx + bx) + upper
    i, j = np.where(upper, block - 1 - i, i), np.where(upper, block - 1 - j, j)
    return dict(W=width, H=height, owner=np.where(owner < n_triangles, owner, -1).astype(np.int64), i=i.astype(np.int64), j=j.astype(np.int64))


def corners(n_triangles, block):
    """the corners of every triangle's UV triangle in TEXEL units, float64 [T, 3, 2] (half-integers: exact)"""
    _, _, nbx, _ = atlas_size(n_triangles, block)
    t = np.arange(n_triangles)
    p = t // 2
    origin = np.stack([(p % max(nbx, 1)) * block, (p // max(nbx, 1)) * block], 1).astype(np.float64)
    b = float(block)
    lower = np.array([[0.5, 0.5], [b - 2.5, 0.5], [0.5, b - 2.5]])
    upper = np.array([[b - 0.5, b - 0.5], [2.5, b - 0.5], [b - 0.5, 2.5]])
    return origin[:, None, :] + np.where((t % 2 == 0)[:, None, None], lower[None], upper[None])


def uv(n_triangles, block):
    """-> float32 [T, 3, 2]: one fp32 division of exact numerators"""
    width, height, _, _ = atlas_size(n_triangles, block)
    c = corners(n_triangles, block).astype(np.float32)
    if n_triangles == 0:
        return c
    return np.stack([c[..., 0] / np.float32(width), c[..., 1] / np.float32(height)], -1)


def bary(block, i, j, dtype):
    span = dtype(block - 3)
    a, b = i.astype(dtype) / span, j.astype(dtype) / span
    s = a + b
    over = s > 1
    safe = np.where(over, s, dtype(1))
    return np.where(over, a / safe, a), np.where(over, b / safe, b)


def blend(a, b, q0, q1, q2, dtype):
    """fma(b, q2 - q0, fma(a, q1 - q0, q0))"""
    return H.fma(b, q2 - q0, H.fma(a, q1 - q0, q0, dtype), dtype)


def fetch(atlas, uv_points):
    """bilinear fetch of atlas [H, W, C] (float64) at normalised uv [N, 2] (origin top-left), as a renderer does it (clamped)"""
    height, width = atlas.shape[:2]
    x, y = uv_points[:, 0] * width - 0.5, uv_points[:, 1] * height - 0.5
    x0, y0 = np.clip(np.floor(x), 0, width - 2).astype(np.int64), np.clip(np.floor(y), 0, height - 2).astype(np.int64)
    ax, ay = (x - x0)[:, None], (y - y0)[:, None]
    a = atlas.astype(np.float64)
    top = a[y0, x0] + ax * (a[y0, x0 + 1] - a[y0, x0])
    bot = a[y0 + 1, x0] + ax * (a[y0 + 1, x0 + 1] - a[y0 + 1, x0])
    return top + ay * (bot - top)


# ------------------------------------------------------------------------------------------------ 2. accumulate
def proj(inv, world, dtype):
    """proj() in the device's order: every row a k-ordered FMA chain (common.hpp: dot4h_chain, dot3_chain) -> u, v, camera-z"""
    x, y, z = world[:, 0], world[:, 1], world[:, 2]
    e, k = inv["extr"], inv["intr"]
    c = [(H.fma(z, e[i, 2], H.fma(y, e[i, 1], x * e[i, 0], dtype), dtype) + e[i, 3]).astype(dtype) for i in range(3)]
    q = [H.fma(c[2], k[i, 2], H.fma(c[1], k[i, 1], c[0] * k[i, 0], dtype), dtype).astype(dtype) for i in range(3)]
    with np.errstate(divide="ignore", invalid="ignore"):
        return q[0] / q[2], q[1] / q[2], q[2]


def triangles_of(vertices, faces, dtype):
    """-> dict(valid [T], idx [T, 3] (0 where out of range), p [T, 3, 3], n [T, 3], len [T]) in dtype"""
    vertices = np.asarray(vertices, np.float32).reshape(-1, 8)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    in_range = ((faces >= 0) & (faces < len(vertices))).all(1)
    idx = np.where(in_range[:, None], faces, 0)
    if len(vertices) == 0:
        z = np.zeros((len(faces), 3), dtype)
        return dict(valid=np.zeros(len(faces), bool), idx=idx, p=np.zeros((len(faces), 3, 3), dtype), n=z, len=z[:, 0])
    p = vertices[:, :3].astype(dtype)[idx]
    with np.errstate(invalid="ignore", over="ignore"):
        u, v = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
        finite = np.isfinite(p).all((1, 2)) & np.isfinite(u).all(1) & np.isfinite(v).all(1)
        u, v = np.where(finite[:, None], u, 0), np.where(finite[:, None], v, 0)
        n = np.stack([H.fma(u[:, 1], v[:, 2], -(u[:, 2] * v[:, 1]), dtype), H.fma(u[:, 2], v[:, 0], -(u[:, 0] * v[:, 2]), dtype),
                      H.fma(u[:, 0], v[:, 1], -(u[:, 1] * v[:, 0]), dtype)], 1).astype(dtype)
        length = np.sqrt(H.fma(n[:, 2], n[:, 2], H.fma(n[:, 1], n[:, 1], n[:, 0] * n[:, 0], dtype), dtype)).astype(dtype)
    return dict(valid=in_range & finite & (length > 0), idx=idx, p=np.where(finite[:, None, None], p, 0).astype(dtype), n=n, len=length)


def accumulate(vertices, faces, block, cams, h, w, legacy, depth, opacity, rgb, n_consistent=None, min_consistent=0,
               min_opacity=F.MIN_OPACITY, vis_rel_tol=VIS_REL_TOL, power=POWER, best=False, dtype=np.float64, accum=None):
    """-> accum [H, W, 4] (dtype; continued from ``accum``), borderline [H, W] bool (float64 only; else all False)"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    lay = layout(len(faces), block)
    out = np.zeros((lay["H"], lay["W"], 4), dtype) if accum is None else np.array(accum, dtype)
    border = np.zeros((lay["H"], lay["W"]), bool)
    tri = triangles_of(vertices, faces, dtype)
    owned = lay["owner"] >= 0
    owned[owned] = tri["valid"][lay["owner"][owned]]
    ty, tx = np.nonzero(owned)
    if not len(ty):
        return out, border
    t = lay["owner"][ty, tx]
    a, b = bary(block, lay["i"][ty, tx], lay["j"][ty, tx], dtype)
    p0, p1, p2 = (tri["p"][t, k] for k in range(3))
    point = np.stack([blend(a, b, p0[:, c], p1[:, c], p2[:, c], dtype) for c in range(3)], 1).astype(dtype)
    n, nlen = tri["n"][t], tri["len"][t]
    inv = F.inverse_cameras(cams, dtype)
    z_all, valid_all, edge_all = F.values(cams, depth, opacity, min_opacity, dtype)
    if n_consistent is not None:
        valid_all = valid_all & (np.asarray(n_consistent).reshape(valid_all.shape) >= min_consistent)
    colour = np.asarray(rgb).reshape(len(cams), h, w, 3).astype(dtype)
    off = dtype(0.0 if legacy else 0.5)
    u_hi, v_hi = dtype(w - 1) + off, dtype(h - 1) + off
    acc = out[ty, tx].copy()
    mark = np.zeros(len(ty), bool)
    first, second = np.zeros(len(ty)), np.zeros(len(ty))  # the two largest weights of the accepted views (best mode's ties)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for k in range(len(cams)):
            e = inv[k]["c2w"][:, 3] - point
            elen = np.sqrt(H.fma(e[:, 2], e[:, 2], H.fma(e[:, 1], e[:, 1], e[:, 0] * e[:, 0], dtype), dtype))
            cos = (H.fma(n[:, 2], e[:, 2], H.fma(n[:, 1], e[:, 1], n[:, 0] * e[:, 0], dtype), dtype) / (nlen * elen)).astype(dtype)
            facing = cos > 0
            u, v, zc = proj(inv[k], point, dtype)
            inside = facing & (zc > 0) & (u >= off) & (u <= u_hi) & (v >= off) & (v <= v_hi)
            fx, fy = np.where(inside, u - off, dtype(0)), np.where(inside, v - off, dtype(0))
            x0, y0, x1, y1 = F.taps(fx, fy, h, w)

            def all_valid(x0, y0, x1, y1):
                return valid_all[k][y0, x0] & valid_all[k][y0, x1] & valid_all[k][y1, x0] & valid_all[k][y1, x1]

            ok = inside & all_valid(x0, y0, x1, y1)
            ax, ay = fx - x0.astype(dtype), fy - y0.astype(dtype)
            zt = np.where(valid_all[k], z_all[k], dtype(1.0))

            def bilinear(m):
                top = H.fma(ax, m[y0, x1] - m[y0, x0], m[y0, x0], dtype)
                bot = H.fma(ax, m[y1, x1] - m[y1, x0], m[y1, x0], dtype)
                return H.fma(ay, bot - top, top, dtype)

            d = bilinear(zt)
            rel = np.abs(d - zc)
            seen = ok & (rel <= dtype(vis_rel_tol) * zc)
            c = np.stack([bilinear(colour[k][..., ch]) for ch in range(3)], 1).astype(dtype)
            weight = np.ones(len(ty), dtype)
            for _ in range(int(power)):
                weight = weight * cos
            if best:
                take = seen & (weight > acc[:, 3])
                acc[take] = np.concatenate([c, weight[:, None]], 1)[take]
            else:
                add = np.concatenate([H.fma(weight[:, None], c, acc[:, :3], dtype), (acc[:, 3] + weight)[:, None]], 1).astype(dtype)
                acc[seen] = add[seen]
            if dtype is np.float64:
                mark |= np.abs(cos) < 1e-6
                front = facing  # what follows is decided only for views that face the texel
                mark |= front & (np.abs(zc) < 1e-6)
                near_frame = (np.minimum(np.abs(u - off), np.abs(u - u_hi)) < 1e-3) | (np.minimum(np.abs(v - off), np.abs(v - v_hi)) < 1e-3)
                mark |= front & (zc > 0) & near_frame
                tap_edge = edge_all[k][y0, x0] | edge_all[k][y0, x1] | edge_all[k][y1, x0] | edge_all[k][y1, x1]
                for sx in (-1e-3, 1e-3):  # the tap set an fp32 projection may pick instead
                    for sy in (-1e-3, 1e-3):
                        moved = F.taps(np.clip(fx + sx, 0, w - 1), np.clip(fy + sy, 0, h - 1), h, w)
                        tap_edge |= all_valid(*moved) != all_valid(x0, y0, x1, y1)
                mark |= inside & tap_edge
                mark |= ok & (np.abs(rel / zc - vis_rel_tol) < 1e-5)
                wk = np.where(seen, weight, 0.0)
                second = np.where(wk > first, first, np.maximum(second, wk))
                first = np.maximum(first, wk)
    if best and dtype is np.float64:
        mark |= (first > 0) & (first - second <= 1e-6 * first)
    out[ty, tx] = acc
    border[ty, tx] = mark
    return out, border


# ------------------------------------------------------------------------------------------------ 3. resolve
def resolve(vertices, faces, block, accum, best=False, dtype=np.float64):
    """-> atlas [H, W, 4] dtype"""
    vertices = np.asarray(vertices, np.float32).reshape(-1, 8)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    lay = layout(len(faces), block)
    acc = np.asarray(accum).astype(dtype)
    out = np.zeros((lay["H"], lay["W"], 4), dtype)
    tri = triangles_of(vertices, faces, dtype)
    owned = lay["owner"] >= 0
    owned[owned] = tri["valid"][lay["owner"][owned]]
    ty, tx = np.nonzero(owned)
    if not len(ty):
        return out
    t = lay["owner"][ty, tx]
    a, b = bary(block, lay["i"][ty, tx], lay["j"][ty, tx], dtype)
    c0, c1, c2 = (vertices[:, 4:7].astype(dtype)[tri["idx"][t, k]] for k in range(3))
    fallback = np.stack([blend(a, b, c0[:, ch], c1[:, ch], c2[:, ch], dtype) for ch in range(3)], 1).astype(dtype)
    texel = acc[ty, tx]
    seen = texel[:, 3] > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = texel[:, :3] if best else texel[:, :3] / np.where(seen, texel[:, 3], dtype(1))[:, None]
    out[ty, tx, :3] = np.where(seen[:, None], mean, fallback)
    out[ty, tx, 3] = seen.astype(dtype)
    return out


# ------------------------------------------------------------------------------------------------ the scene
PHASES = ((0.3, 1.1, 2.0), (1.7, 0.2, 0.9), (2.9, 2.3, 0.4))


def colour_field(p, voxel):
    """world points [..., 3] -> rgb [..., 3] in [0, 1]: per channel a product of sinusoids with a period of 2 voxels - a colour per
    voxel aliases, a colour per pixel of the test frames does not"""
    p = np.asarray(p, np.float64)
    om = np.pi / voxel
    return np.stack([0.5 + 0.5 * np.sin(om * p[..., 0] + a) * np.sin(om * p[..., 1] + b) * np.sin(om * p[..., 2] + c)
                     for a, b, c in PHASES], -1)


def view_colours(cams, h, w, legacy, depth, opacity, voxel):
    """the field at every pixel's lifted point -> float32 [K, h*w, 3] (0.5 where the pixel has no finite point)"""
    inv = F.inverse_cameras(cams, np.float64)
    x, y = F.pixel_centres(h, w, legacy)
    out = np.zeros((len(cams), h * w, 3), np.float32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        z = depth.astype(np.float64) if opacity is None else depth.astype(np.float64) / opacity.astype(np.float64)
        for k in range(len(cams)):
            c = colour_field(F.lift(inv[k], x, y, z[k]), voxel).reshape(-1, 3)
            out[k] = np.where(np.isfinite(c), c, 0.5)
    return out


@functools.lru_cache(maxsize=None)
def scene(k, h, w, legacy, variant="plain", consistent=False):
    """one case, computed once and shared (read-only) -> dict(cams, depth, opacity, counts, min_consistent, rgb [K, h*w, 3] f32, voxel,
    origin, dims, vertices f32 [V, 8], faces int32 [T, 3]): the maps of mesh_helpers.integrate_reference, the analytic colours of the
    views, and the restated mesh of the restated volume - its vertex colours integrated from those view colours"""
    r = M.integrate_reference(k, h, w, legacy, variant, consistent)
    rgb = view_colours(r["cams"], h, w, legacy, r["depth"], r["opacity"], r["voxel"])
    coloured, weight, _ = M.integrate(r["cams"], h, w, legacy, r["depth"], r["opacity"], rgb, r["origin"], r["voxel"], r["dims"], r["trunc"],
                                      n_consistent=r["counts"], min_consistent=r["min_consistent"])
    assert np.array_equal(weight, r["weight"]) and np.array_equal(coloured[..., 0], r["sums"][..., 0])  # the same geometry
    m = M.mesh(coloured.astype(np.float32), weight.astype(np.float32), r["origin"], r["voxel"], float(max(1, min(2, k - 1))))
    out = dict(r)
    out.update(rgb=rgb, vertices=m["vertices"].astype(np.float32), faces=m["faces"].astype(np.int32))
    return out


@functools.lru_cache(maxsize=None)
def baked(k, h, w, legacy, variant, consistent, block, best):
    """the float64 and float32 restatements of one case -> dict(atlas, border, atlas32, accum32)"""
    s = scene(k, h, w, legacy, variant, consistent)
    args = (s["vertices"], s["faces"], block, s["cams"], h, w, legacy, s["depth"], s["opacity"], s["rgb"])
    kwargs = dict(n_consistent=s["counts"], min_consistent=s["min_consistent"], best=best)
    acc, border = accumulate(*args, **kwargs)
    acc32, _ = accumulate(*args, dtype=np.float32, **kwargs)
    return dict(atlas=resolve(s["vertices"], s["faces"], block, acc, best), border=border, accum32=acc32,
                atlas32=resolve(s["vertices"], s["faces"], block, acc32, best, np.float32))


def atlas_distance(got, want, border):
    """atlas [H, W, 4] against the float64 one -> (the largest rgb difference over the non-borderline texels, the number of those
    whose alpha differs, the share of the OWNED texels that is borderline)"""
    keep = ~border
    rgb = np.abs(np.asarray(got, np.float64)[..., :3] - want[..., :3])[keep]
    alpha = int((np.asarray(got)[..., 3][keep] != want[..., 3][keep]).sum())
    return float(rgb.max()) if rgb.size else 0.0, alpha, float(border.mean())


# ------------------------------------------------------------------------------------------------ the purpose
def surface_samples(vertices, faces, n, seed=0):
    """n random points on the triangles (uniform over the triangles' COUNT, as the atlas spends its texels) -> triangle [n], barycentric
    (a, b) [n, 2] float64, world points [n, 3]"""
    rng = np.random.default_rng(seed)
    tri = triangles_of(vertices, faces, np.float64)
    t = rng.choice(np.nonzero(tri["valid"])[0], n)
    ab = rng.random((n, 2))
    ab = np.where((ab.sum(1) > 1)[:, None], 1 - ab, ab)
    p = tri["p"][t]
    return t, ab, p[:, 0] + ab[:, :1] * (p[:, 1] - p[:, 0]) + ab[:, 1:] * (p[:, 2] - p[:, 0])


def colour_errors(vertices, faces, block, atlas, voxel, n=20000):
    """RMS error against the colour field of (the atlas fetched bilinearly at the samples' uv, the vertex colours interpolated at
    them), over samples whose atlas texels were all seen (alpha 1)"""
    vertices, faces = np.asarray(vertices, np.float32), np.asarray(faces, np.int64)
    t, ab, world = surface_samples(vertices, faces, n)
    c = uv(len(faces), block).astype(np.float64)[t]
    at = c[:, 0] + ab[:, :1] * (c[:, 1] - c[:, 0]) + ab[:, 1:] * (c[:, 2] - c[:, 0])
    texel = fetch(np.asarray(atlas, np.float64), at)
    seen = texel[:, 3] >= 1.0
    vc = vertices[:, 4:7].astype(np.float64)[faces[t]]
    lerp = vc[:, 0] + ab[:, :1] * (vc[:, 1] - vc[:, 0]) + ab[:, 1:] * (vc[:, 2] - vc[:, 0])
    truth = colour_field(world, voxel)
    rms = lambda x: float(np.sqrt(np.mean((x[seen] - truth[seen]) ** 2)))
    return rms(texel[:, :3]), rms(lerp), float(seen.mean())


# ------------------------------------------------------------------------------------------------ hand-made meshes
def hand_mesh(kind):
    """-> (vertices f32 [V, 8], faces int32 [T, 3]) in the scene of (3, 24, 32): ``facing``: one triangle on the box's front face
    (z = -0.6), wound towards the cameras; ``back``: the same wound away; ``occluded``: on the plane z = 0 behind the box, wound
    towards the cameras; ``broken``: a good triangle, a degenerate one, one with an index >= V, one with a NaN vertex, another good one"""
    rng = np.random.default_rng(11)
    front = np.array([[-0.2, -0.1, -0.6], [-0.2, 0.15, -0.6], [0.1, -0.1, -0.6]])  # n = (p1 - p0) x (p2 - p0) = (0, 0, -0.075): -z
    rows = lambda pos: np.concatenate([pos, np.ones((len(pos), 1)), rng.random((len(pos), 3)), np.zeros((len(pos), 1))], 1).astype(np.float32)
    if kind == "facing":
        return rows(front), np.array([[0, 1, 2]], np.int32)
    if kind == "back":
        return rows(front), np.array([[0, 2, 1]], np.int32)
    if kind == "occluded":
        return rows(front * np.array([0.5, 0.5, 0.0])), np.array([[0, 1, 2]], np.int32)
    assert kind == "broken"
    vertices = rows(np.concatenate([front, front + np.array([0.05, 0.02, 0.0]), [[0.0, 0.0, -0.6]]]))
    vertices[6, 1] = np.nan
    return vertices, np.array([[0, 1, 2], [0, 1, 1], [0, 1, 7], [3, 6, 5], [3, 4, 5]], np.int32)


# ------------------------------------------------------------------------------------------------ refusals
def assert_atlas_refusals(hip):
    """mnerf_mesh_texture_atlas: host only, needs no GPU"""
    import ctypes as C
    lib = hip.load()
    size = (C.c_int32 * 2)()
    r, n, ok = hip.MNERF_E_RANGE, hip.MNERF_E_NULL, hip.MNERF_OK
    for t, b, want in ((-1, 8, r), (10, 3, r), (10, 65, r), (10, 0, r), (((1 << 31) - 1) // 3 + 1, 8, r), (2 * 4096 * 4096 + 1, 4, r),
                       (2 * 4096 * 4096, 4, ok), (2 * 256 * 256 + 1, 64, r), (2 * 256 * 256, 64, ok), (0, 8, ok), (1, 4, ok)):
        assert lib.mnerf_mesh_texture_atlas(t, b, size) == want, (t, b, want, lib.mnerf_last_error())
        if want == ok:
            assert (size[0], size[1]) == atlas_size(t, b)[:2], (t, b)
    assert lib.mnerf_mesh_texture_atlas(10, 8, None) == n
    assert lib.mnerf_mesh_texture_atlas(-1, 8, None) == r  # RANGE precedes NULL


def assert_refusals(hip):
    """every MNERF_E_* the header names for the three device entry points, from fake addresses: each call fails its checks, or has
    nothing to launch, before any HIP call"""
    import ctypes as C
    lib = hip.load()
    assert_atlas_refusals(hip)
    fake, odd4, odd16 = C.c_void_p(0x10000), C.c_void_p(0x10002), C.c_void_p(0x10008)
    i32 = lambda p: None if p is None else C.cast(p, C.POINTER(C.c_int32))
    r, n, a, ok = hip.MNERF_E_RANGE, hip.MNERF_E_NULL, hip.MNERF_E_ALIGN, hip.MNERF_OK
    nan, inf = float("nan"), float("inf")
    big_v, big_t = 1 << 31, ((1 << 31) - 1) // 3 + 1
    cams = F.arc_cameras(2, 8, 8)
    good = hip.view_array([hip.make_view(c["extr"], c["intr"], c["near"], c["far"]) for c in cams])
    singular = hip.view_array([hip.make_view(cams[0]["extr"], np.zeros((3, 3)), 0.5, 6.0)] * 2)
    flat = hip.view_array([hip.make_view(np.zeros((3, 4)), cams[0]["intr"], 0.5, 6.0)] * 2)

    def uv(t=4, block=8, out=fake):
        return lib.mnerf_mesh_texture_uv(t, block, out, None)

    for want, kwargs in ((r, dict(t=-1)), (r, dict(t=big_t)), (r, dict(block=3)), (r, dict(block=65)), (r, dict(t=2 * 4096 * 4096 + 1, block=4)),
                         (r, dict(t=-1, out=None)), (n, dict(out=None)), (a, dict(out=odd4)), (ok, dict(t=0, out=None))):
        assert uv(**kwargs) == want, ("uv", kwargs, want, lib.mnerf_last_error())

    def accumulate(vert=fake, tri=fake, v=8, t=4, block=8, views=good, k=2, h=8, w=8, depth=fake, opacity=None, counts=None, rgb=fake,
                   min_opacity=0.5, tol=0.02, power=2, best=0, accum=fake):
        return lib.mnerf_mesh_texture_accumulate(vert, i32(tri), v, t, block, views, k, h, w, 0, depth, opacity, i32(counts), 1, rgb,
                                                 min_opacity, tol, power, best, accum, None)

    cases = [(r, dict(v=-1)), (r, dict(v=big_v)), (r, dict(t=-1)), (r, dict(t=big_t)), (r, dict(block=3)), (r, dict(block=65)),
             (r, dict(t=2 * 4096 * 4096 + 1, block=4)), (r, dict(k=0)), (r, dict(k=17)), (r, dict(h=0)), (r, dict(w=0)), (r, dict(h=65536, w=32768)),
             (r, dict(opacity=fake, min_opacity=nan)), (r, dict(tol=0.0)), (r, dict(tol=-1.0)), (r, dict(tol=nan)), (r, dict(tol=inf)),
             (r, dict(power=-1)), (r, dict(power=9)), (r, dict(views=singular)), (r, dict(views=flat)),
             (r, dict(power=9, vert=None)),  # RANGE precedes NULL
             (n, dict(vert=None)), (n, dict(tri=None)), (n, dict(views=None)), (n, dict(depth=None)), (n, dict(rgb=None)), (n, dict(accum=None)),
             (n, dict(accum=None, vert=odd16)),  # NULL precedes ALIGN
             (a, dict(vert=odd16)), (a, dict(accum=odd16)), (a, dict(tri=odd4)), (a, dict(depth=odd4)), (a, dict(opacity=odd4)),
             (a, dict(counts=odd4)), (a, dict(rgb=odd4)),
             (ok, dict(t=0, vert=None, tri=None, views=None, depth=None, rgb=None, accum=None))]
    for want, kwargs in cases:
        assert accumulate(**kwargs) == want, ("accumulate", kwargs, want, lib.mnerf_last_error())

    def resolve(vert=fake, tri=fake, v=8, t=4, block=8, best=0, accum=fake, atlas=fake):
        return lib.mnerf_mesh_texture_resolve(vert, i32(tri), v, t, block, best, accum, atlas, None)

    cases = [(r, dict(v=-1)), (r, dict(v=big_v)), (r, dict(t=-1)), (r, dict(t=big_t)), (r, dict(block=3)), (r, dict(block=65)),
             (r, dict(t=2 * 256 * 256 + 1, block=64)), (r, dict(t=-1, atlas=None)),
             (n, dict(vert=None)), (n, dict(tri=None)), (n, dict(accum=None)), (n, dict(atlas=None)), (n, dict(atlas=None, accum=odd16)),
             (a, dict(vert=odd16)), (a, dict(accum=odd16)), (a, dict(atlas=odd16)), (a, dict(tri=odd4)),
             (ok, dict(t=0, vert=None, tri=None, accum=None, atlas=None))]
    for want, kwargs in cases:
        assert resolve(**kwargs) == want, ("resolve", kwargs, want, lib.mnerf_last_error())
