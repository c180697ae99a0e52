"""Mesh raster (include/mnerf.h "MESH RASTER") restated in numpy, operation by operation after the header's text: raster + resolve
(``raster``) and shade (``shade``), and the cases the tests run them on.

``dtype`` selects the arithmetic (float64: the reference; float32: the same chain in the device's format with mesh_finish_helpers.fma,
whose distance from float64 sizes the depth and bary gates).  In float64 ``raster`` also marks the BORDERLINE pixels, whose discrete
decisions fp32 may take differently.  With d_k = E_k / (the length of edge k) the distance in pixels of the centre from edge k, a
triangle NEARLY COVERS a pixel when every d_k > -EPS_PX.  A pixel is borderline when
  some triangle that nearly covers it has a |d_k| < EPS_PX (it lies on an edge, to within what fp32 can tell), or a |screen area|
  below EPS_AREA px^2 (its orientation, and with it every sign, is uncertain), or a depth within EPS_REL of near_ or far_;
  the two smallest depths over it lie within EPS_REL (relative) of each other;
  the winner's |screen area| is below EPS_AREA px^2 (its weights are ill-conditioned: an error e of an edge value is e / (2 area)
  in a weight);
  a vertex of a triangle whose bounding box meets the pixel has a camera-z within EPS_REL of 0."""
import functools

import numpy as np

import fusion_helpers as F
import mesh_decimate_helpers as D
import mesh_finish_helpers as H
import mesh_helpers as M
import mesh_texture_helpers as X

BORDERLINE_CAP = F.BORDERLINE_CAP
RGB_GATE = X.RGB_GATE
EPS_PX, EPS_REL, EPS_AREA = 1e-4, 1e-5, 1e-3
# The largest distance of the float32 restatement from the float64 one over the non-borderline pixels of every case below
# (tests/test_mesh_raster_cpu.py asserts that it is not exceeded): relative for the depth, absolute for the weights.  The device is
# gated at 4 x these - the margin covers a division or a reciprocal rounded otherwise.  The figures were measured with one numpy on
# one host; the CPU test allows the restatement F32_HEADROOM x them, for a libm or a summation that rounds otherwise elsewhere.
F32_DEPTH_REL, F32_BARY = 5.3e-6, 4.8e-4
F32_HEADROOM = 1.25
DEPTH_GATE, BARY_GATE = 4 * F32_DEPTH_REL, 4 * F32_BARY
SPHERE_DIMS = (64, 64, 64)
FRAMES = ((3, 24, 32), (16, 37, 53))
# (mesh, decimated, K, h, w, legacy)
CASES = [(mesh, dec, k, h, w, legacy) for mesh in ("sphere", "scene") for dec in (False, True) for (k, h, w) in FRAMES for legacy in (True, False)]
DECIMATE_CELL = 3  # voxels


# ------------------------------------------------------------------------------------------------ raster + resolve
def project(cam, vertices, dtype):
    """proj() of every vertex -> u, v, z [V] in dtype"""
    inv = F.inverse_cameras([cam], dtype)[0]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        return X.proj(inv, np.asarray(vertices, np.float32)[:, :3].astype(dtype), dtype)


def edge_value(au, av, bu, bv, px, py, dtype):
    """value(a -> b, P) and the gradient's components before the orientation's sign"""
    swap = (bu < au) | ((bu == au) & (bv < av))
    fu, fv, su, sv = np.where(swap, bu, au), np.where(swap, bv, av), np.where(swap, au, bu), np.where(swap, av, bv)
    dx, dy = su - fu, sv - fv
    e = H.fma(dx, py - fv, -(dy * (px - fu)), dtype)
    e = np.where(((px == fu) & (py == fv)) | ((px == su) & (py == sv)), dtype(0), e).astype(dtype)
    return np.where(swap, -e, e), np.where(swap, dy, -dy), np.where(swap, -dx, dx)


def setup(vertices, faces, cam, dtype):
    """-> dict(valid [T], u, v, z [T, 3], sign [T], area [T]) in dtype: the triangles as the raster kernel sets them up"""
    vertices = np.asarray(vertices, np.float32).reshape(-1, 8)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    in_range = ((faces >= 0) & (faces < len(vertices))).all(1)
    idx = np.where(in_range[:, None], faces, 0)
    if len(vertices) == 0:
        z = np.zeros((len(faces), 3), dtype)
        return dict(valid=np.zeros(len(faces), bool), idx=idx, u=z, v=z, z=z, sign=z[:, 0], area=z[:, 0])
    pu, pv, pz = project(cam, vertices, dtype)
    finite = np.isfinite(vertices[:, :3]).all(1) & np.isfinite(pu) & np.isfinite(pv) & np.isfinite(pz)
    with np.errstate(invalid="ignore"):
        ok = finite & (pz > 0)
    u, v, z = pu[idx], pv[idx], pz[idx]
    valid = in_range & ok[idx].all(1)
    u, v, z = (np.where(valid[:, None], q, dtype(1)) for q in (u, v, z))
    area, _, _ = edge_value(u[:, 1], v[:, 1], u[:, 2], v[:, 2], u[:, 0], v[:, 0], dtype)
    valid = valid & (area != 0)
    return dict(valid=valid, idx=idx, u=u, v=v, z=z, sign=np.where(area > 0, dtype(1), dtype(-1)), area=area)


def pairs(tri, h, w, legacy):
    """the (triangle, pixel) pairs that can be covered or nearly covered: the pixels whose centres lie in the triangles' bounding
    boxes grown by 2 EPS_PX (the kernel walks more pixels; they fail the same coverage test) -> t, x, y"""
    off = 0.0 if legacy else 0.5
    t = np.flatnonzero(tri["valid"])
    u, v = tri["u"][t].astype(np.float64), tri["v"][t].astype(np.float64)
    x0, x1 = np.maximum(np.ceil(u.min(1) - off - 2 * EPS_PX), 0), np.minimum(np.floor(u.max(1) - off + 2 * EPS_PX), w - 1)
    y0, y1 = np.maximum(np.ceil(v.min(1) - off - 2 * EPS_PX), 0), np.minimum(np.floor(v.max(1) - off + 2 * EPS_PX), h - 1)
    keep = (x0 <= x1) & (y0 <= y1)
    t, x0, x1, y0, y1 = t[keep], x0[keep].astype(np.int64), x1[keep].astype(np.int64), y0[keep].astype(np.int64), y1[keep].astype(np.int64)
    nx, ny = x1 - x0 + 1, y1 - y0 + 1
    count = nx * ny
    which = np.repeat(np.arange(len(t)), count)
    local = np.arange(count.sum()) - np.repeat(np.cumsum(count) - count, count)
    return t[which], x0[which] + local % nx[which], y0[which] + local // nx[which]


def evaluate(tri, t, px, py, dtype):
    """the coverage quantities of the pairs -> covered [N], E [N, 3], z, b1, b2 [N], d [N, 3] (E / edge length)"""
    u, v, zv, s = tri["u"][t], tri["v"][t], tri["z"][t], tri["sign"][t]
    inside = np.ones(len(t), bool)
    E, d = np.zeros((len(t), 3), dtype), np.zeros((len(t), 3), dtype)
    for k in range(3):
        a, b = (k + 1) % 3, (k + 2) % 3
        e, gx, gy = edge_value(u[:, a], v[:, a], u[:, b], v[:, b], px, py, dtype)
        E[:, k] = s * e
        gx, gy = s * gx, s * gy
        owns = (gx > 0) | ((gx == 0) & (gy > 0))
        inside &= (E[:, k] > 0) | ((E[:, k] == 0) & owns)
        d[:, k] = E[:, k] / np.maximum(np.hypot(gx, gy), np.finfo(dtype).tiny)
    total = (E[:, 0] + E[:, 1]) + E[:, 2]
    positive = total > 0
    safe = np.where(positive, total, dtype(1))
    q = [(E[:, k] / safe) / zv[:, k] for k in range(3)]
    wsum = (q[0] + q[1]) + q[2]
    with np.errstate(divide="ignore", invalid="ignore"):
        z = dtype(1) / wsum
        b1, b2 = q[1] / wsum, q[2] / wsum
    return inside & positive, E, z.astype(dtype), b1.astype(dtype), b2.astype(dtype), d


def raster(vertices, faces, cam, h, w, legacy, dtype=np.float64):
    """mnerf_mesh_raster -> dict(face int32 [h, w], depth, bary [h, w, 2] in dtype, border bool [h, w] (float64 only; else False))"""
    tri = setup(vertices, faces, cam, dtype)
    face = np.full(h * w, -1, np.int32)
    depth, bary = np.zeros(h * w, dtype), np.zeros((h * w, 2), dtype)
    border = np.zeros(h * w, bool)
    t, x, y = pairs(tri, h, w, legacy)
    if len(t):
        off = dtype(0.0 if legacy else 0.5)
        pix = y * w + x
        covered, E, z, b1, b2, d = evaluate(tri, t, x.astype(dtype) + off, y.astype(dtype) + off, dtype)
        near, far = dtype(cam["near"]), dtype(cam["far"])
        with np.errstate(invalid="ignore"):
            hit = covered & (z > 0) & (z >= near) & (z <= far)
        order = np.lexsort((t[hit], z[hit], pix[hit]))
        sel = np.flatnonzero(hit)[order]
        first = np.ones(len(sel), bool)
        first[1:] = pix[sel][1:] != pix[sel][:-1]
        win = sel[first]
        face[pix[win]], depth[pix[win]] = t[win], z[win]
        bary[pix[win], 0], bary[pix[win], 1] = b1[win], b2[win]
        if dtype is np.float64:
            nearly = (d > -EPS_PX).all(1)
            small = np.abs(tri["area"][t]) < EPS_AREA
            with np.errstate(invalid="ignore"):
                at_range = (np.abs(z - near) < EPS_REL * near) | (np.abs(z - far) < EPS_REL * far)
            mark = nearly & ((np.abs(d) < EPS_PX).any(1) | small | at_range)
            mark |= (np.abs(tri["z"][t]) < EPS_REL).any(1)
            border[pix[mark]] = True
            border[pix[win[small[win]]]] = True
            second = sel[~first]  # every hit but the winner: the runner-up is the first of them per pixel
            if len(second):
                lead = np.ones(len(second), bool)
                lead[1:] = pix[second][1:] != pix[second][:-1]
                runner = second[lead]
                close = z[runner] - depth[pix[runner]] <= EPS_REL * depth[pix[runner]]
                border[pix[runner[close]]] = True
    # triangles the kernel drops for a camera-z that fp32 may see on the other side of 0 are not modelled: no case has one
    return dict(face=face.reshape(h, w), depth=depth.reshape(h, w), bary=bary.reshape(h, w, 2), border=border.reshape(h, w))


# ------------------------------------------------------------------------------------------------ shade
def shade(vertices, faces, face, bary, cam, atlas=None, block=0, dtype=np.float64):
    """mnerf_mesh_shade -> rgba [h, w, 4], normal [h, w, 4] in dtype"""
    vertices = np.asarray(vertices, np.float32).reshape(-1, 8)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    h, w = face.shape
    rgba, normal = np.zeros((h * w, 4), dtype), np.zeros((h * w, 4), dtype)
    f = np.asarray(face, np.int64).reshape(-1)
    ok = (f >= 0) & (f < len(faces))
    ok[ok] = ((faces[f[ok]] >= 0) & (faces[f[ok]] < len(vertices))).all(1)
    i = np.flatnonzero(ok)
    if not len(i):
        return rgba.reshape(h, w, 4), normal.reshape(h, w, 4)
    t = f[i]
    b1, b2 = (np.asarray(bary).reshape(-1, 2)[i, c].astype(dtype) for c in range(2))
    corner = faces[t]
    if atlas is None:
        c0, c1, c2 = (vertices[corner[:, k], 4:7].astype(dtype) for k in range(3))
        rgb = np.stack([X.blend(b1, b2, c0[:, ch], c1[:, ch], c2[:, ch], dtype) for ch in range(3)], 1)
    else:
        tex = np.asarray(atlas).astype(dtype)
        height, width = tex.shape[:2]
        c = X.corners(len(faces), block).astype(dtype)[t]  # half-integers below 2^15: exact in either format
        tu = X.blend(b1, b2, c[:, 0, 0], c[:, 1, 0], c[:, 2, 0], dtype)
        tv = X.blend(b1, b2, c[:, 0, 1], c[:, 1, 1], c[:, 2, 1], dtype)
        fx, fy = (tu - dtype(0.5)).astype(dtype), (tv - dtype(0.5)).astype(dtype)
        x0, y0, x1, y1 = F.taps(fx, fy, height, width)
        ax, ay = (fx - x0.astype(dtype)).astype(dtype), (fy - y0.astype(dtype)).astype(dtype)
        x1, y1 = np.where(ax == 0, x0, x1), np.where(ay == 0, y0, y1)
        _, _, nbx, _ = X.atlas_size(len(faces), block)
        upper = t % 2 == 1
        ox, oy = ((t // 2) % nbx) * block, ((t // 2) // nbx) * block
        ix, iy = np.where(upper, x1, x0), np.where(upper, y1, y0)

        def tap(x, y):
            li, lj = x - ox, y - oy
            owned = (li >= 0) & (li < block) & (lj >= 0) & (lj < block) & np.where(upper, li + lj >= block, li + lj <= block - 1)
            return tex[np.where(owned, y, iy), np.where(owned, x, ix), :3]

        t00, t10, t01, t11 = tap(x0, y0), tap(x1, y0), tap(x0, y1), tap(x1, y1)
        top = H.fma(ax[:, None], t10 - t00, t00, dtype)
        bot = H.fma(ax[:, None], t11 - t01, t01, dtype)
        rgb = H.fma(ay[:, None], bot - top, top, dtype)
    rgba[i, :3], rgba[i, 3] = rgb, 1
    p0, p1, p2 = (vertices[corner[:, k], :3].astype(dtype) for k in range(3))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        a, b = p1 - p0, p2 - p0
        n = np.stack([H.fma(a[:, 1], b[:, 2], -(a[:, 2] * b[:, 1]), dtype), H.fma(a[:, 2], b[:, 0], -(a[:, 0] * b[:, 2]), dtype),
                      H.fma(a[:, 0], b[:, 1], -(a[:, 1] * b[:, 0]), dtype)], 1).astype(dtype)
        length = np.sqrt(H.fma(n[:, 2], n[:, 2], H.fma(n[:, 1], n[:, 1], n[:, 0] * n[:, 0], dtype), dtype)).astype(dtype)
        good = (length > 0) & np.isfinite(length)
        e = F.inverse_cameras([cam], dtype)[0]["c2w"][:, 3] - p0
        towards = H.fma(n[:, 2], e[:, 2], H.fma(n[:, 1], e[:, 1], n[:, 0] * e[:, 0], dtype), dtype)
        s = np.where(towards < 0, dtype(-1), dtype(1))
        unit = s[:, None] * (n / np.where(good, length, dtype(1))[:, None])
    normal[i[good], :3] = unit[good]
    return rgba.reshape(h, w, 4), normal.reshape(h, w, 4)


# ------------------------------------------------------------------------------------------------ hand-made meshes
def pixel_camera(near=0.5, far=100.0):
    """a camera whose arithmetic is exact on small integers: identity pose and intrinsics, so that the world point (x z, y z, z)
    projects to the pixel coordinates (x, y) at camera-z z exactly when z is a power of two"""
    return dict(extr=np.eye(3, 4, dtype=np.float32), intr=np.eye(3, dtype=np.float32), near=near, far=far)


def rows(pixels, z=2.0, seed=3):
    """vertices [V, 8] whose projections under pixel_camera are the given pixel coordinates, at camera-z ``z`` (a scalar or [V])"""
    pixels = np.asarray(pixels, np.float64).reshape(-1, 2)
    z = np.broadcast_to(np.asarray(z, np.float64), (len(pixels),))
    rng = np.random.default_rng(seed)
    pos = np.stack([pixels[:, 0] * z, pixels[:, 1] * z, z], 1)
    return np.concatenate([pos, np.ones((len(pos), 1)), rng.random((len(pos), 3)), np.zeros((len(pos), 1))], 1).astype(np.float32)


def hand_mesh(kind):
    """-> (vertices f32 [V, 8], faces int32 [T, 3]) for pixel_camera, legacy coordinates (pixel centres on the integers)"""
    tri = lambda *f: np.array(f, np.int32).reshape(-1, 3)
    if kind == "quad":  # [0, 8]^2, the diagonal through the pixel centres (k, k)
        return rows([(0, 0), (8, 0), (8, 8), (0, 8)]), tri((0, 1, 2), (0, 2, 3))
    if kind == "quad_unwelded":
        return rows([(0, 0), (8, 0), (8, 8), (0, 0), (8, 8), (0, 8)]), tri((0, 1, 2), (3, 4, 5))
    if kind == "fan":  # six triangles around the pixel centre (10, 9), mixed windings
        ring = [(16, 9), (14, 15), (5, 16), (3, 9), (6, 2), (15, 3)]
        faces = [(0, 1 + k, 1 + (k + 1) % 6) if k % 2 == 0 else (0, 1 + (k + 1) % 6, 1 + k) for k in range(6)]
        return rows([(10, 9)] + ring), tri(*faces)
    if kind == "coincident":
        # (the same corners in the same order, once through other vertex rows: any other order sums the weights otherwise and may
        # differ in the last bit of z)
        return rows([(2, 2), (12, 3), (4, 13)] * 2), tri((0, 1, 2), (0, 1, 2), (3, 4, 5))
    if kind == "huge":
        return rows([(-200, -100), (300, -100), (-200, 400)]), tri((0, 1, 2))
    if kind == "nothing":  # outside the frame, behind the camera, crossing the camera plane, zero area
        v = np.concatenate([rows([(-30, -30), (-20, -30), (-30, -20)]), rows([(2, 2), (12, 3), (4, 13)], z=-2.0),
                            rows([(2, 2), (12, 3), (4, 13)], z=[2.0, 2.0, -2.0]), rows([(2, 2), (6, 6), (10, 10)])])
        return v, tri((0, 1, 2), (3, 4, 5), (6, 7, 8), (9, 10, 11))
    assert kind == "broken"  # a good triangle, an index >= V, a negative index, a NaN vertex, another good one
    v = rows([(1, 1), (9, 2), (3, 10), (12, 12), (20, 13), (14, 21), (5, 5)])
    v[6, 1] = np.nan
    return v, tri((0, 1, 2), (0, 1, 7), (0, -1, 2), (0, 6, 2), (3, 4, 5))


def top_left_set(x0, y0, x1, y1, h, w):
    """the pixels (legacy centres) of the axis-aligned rectangle [x0, x1] x [y0, y1] under the top-left rule: left and top edges in"""
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return (x >= x0) & (x < x1) & (y >= y0) & (y < y1)


# ------------------------------------------------------------------------------------------------ the cases
def look_at(centre, eye, h, w, near, far):
    fwd = (centre - eye) / np.linalg.norm(centre - eye)
    right = np.cross(np.array([0.0, 1.0, 0.0]), fwd)
    right /= np.linalg.norm(right)
    rot = np.stack([right, np.cross(fwd, right), fwd])
    intr = np.array([[0.9 * w, 0, 0.5 * w], [0, 0.9 * w, 0.5 * h], [0, 0, 1]], np.float32)
    return dict(extr=np.concatenate([rot, (-rot @ eye)[:, None]], 1).astype(np.float32), intr=intr, near=near, far=far)


def sphere_cameras(k, h, w):
    """K cameras outside the sphere of mesh_helpers on a spiral around it, looking at its centre from 1.5, 2.2 and 3.2 radii in turn:
    a cap that fills the frame, the sphere cut by the frame's border, the whole silhouette.  (At 64^3 the triangles are a tenth of a
    pixel wide from 3.2 radii, and the share of pixel centres within EPS_PX of an edge grows with the edge length per pixel: from
    3.2 radii alone the three views of 24 x 32 have 1.0 - 1.1 % borderline pixels, above the cap.)"""
    c = np.array(M.SPHERE_C)
    cams = []
    for j in range(k):
        a, e = 2.399963 * j + 0.3, 0.9 * np.sin(1.7 * j + 0.4)  # (no pose looks along the y axis)
        eye = c + (1.5, 2.2, 3.2)[j % 3] * M.SPHERE_R * np.array([np.cos(e) * np.sin(a), np.sin(e), -np.cos(e) * np.cos(a)])
        cams.append(look_at(c, eye, h, w, 0.2, 6.0))
    return cams


@functools.lru_cache(maxsize=None)
def mesh_of(name, decimated, k, h, w, legacy):
    """-> dict(vertices f32 [V, 8], faces int32 [T, 3], cams, voxel, and for the scene its maps): the sphere at 64^3 from the spiral
    cameras, or the plane + box scene of mesh_texture_helpers from its arc cameras; ``decimated``: with cells of 3 voxels on the
    volume's grid"""
    if name == "sphere":
        vol = M.sphere_volume(SPHERE_DIMS)
        m = M.sphere_mesh(SPHERE_DIMS)
        out = dict(vertices=m["vertices"].astype(np.float32), faces=m["faces"].astype(np.int32), cams=sphere_cameras(k, h, w),
                   voxel=vol["voxel"], origin=vol["origin"], dims=SPHERE_DIMS)
    else:
        out = dict(X.scene(k, h, w, legacy, "plain", False))
    if decimated:
        cell = DECIMATE_CELL * out["voxel"]
        dims = tuple(int(np.ceil(d / DECIMATE_CELL)) for d in out["dims"])
        m = D.decimate(out["vertices"], out["faces"], out["origin"], cell, dims)
        out.update(vertices=m["vertices"].astype(np.float32), faces=m["faces"].astype(np.int32))
    return out


@functools.lru_cache(maxsize=None)
def rastered(name, decimated, k, h, w, legacy):
    """the float64 and float32 restatements of every view of a case -> [dict(face, depth, bary, border, face32, depth32, bary32)]"""
    m = mesh_of(name, decimated, k, h, w, legacy)
    out = []
    for cam in m["cams"]:
        r = raster(m["vertices"], m["faces"], cam, h, w, legacy)
        r32 = raster(m["vertices"], m["faces"], cam, h, w, legacy, np.float32)
        r.update(face32=r32["face"], depth32=r32["depth"], bary32=r32["bary"])
        out.append(r)
    return out


SPHERE_BLOCK, SCENE_BLOCK = 4, 8


@functools.lru_cache(maxsize=None)
def atlas_of(name, decimated, k, h, w, legacy):
    """-> (atlas float32 [H, W, 4], block): the scene's atlas baked from its views by the float32 restatement of MESH TEXTURE; the
    sphere, which has no views' maps, gets what resolve leaves of an empty accumulation buffer - the vertex colours' blend, a = 0"""
    m = mesh_of(name, decimated, k, h, w, legacy)
    if name == "sphere":
        width, height, _, _ = X.atlas_size(len(m["faces"]), SPHERE_BLOCK)
        acc, block = np.zeros((height, width, 4), np.float32), SPHERE_BLOCK
    else:
        acc, _ = X.accumulate(m["vertices"], m["faces"], SCENE_BLOCK, m["cams"], h, w, legacy, m["depth"], m["opacity"], m["rgb"],
                              dtype=np.float32)
        block = SCENE_BLOCK
    return X.resolve(m["vertices"], m["faces"], block, acc, dtype=np.float32).astype(np.float32), block


def frame_distance(got_depth, got_bary, want, keep):
    """-> (largest relative depth error, largest weight error) over the pixels of ``keep`` that the reference hit"""
    on = keep & (want["face"] >= 0)
    if not on.any():
        return 0.0, 0.0
    rel = np.abs(np.asarray(got_depth, np.float64)[on] - want["depth"][on]) / want["depth"][on]
    return float(rel.max()), float(np.abs(np.asarray(got_bary, np.float64)[on] - want["bary"][on]).max())


def sphere_hits(cam, h, w, legacy, shrink):
    """the pixels whose float64 ray hits the analytic sphere shrunk by ``shrink`` -> bool [h, w]"""
    inv = F.inverse_cameras([cam], np.float64)[0]
    x, y = F.pixel_centres(h, w, legacy)
    d = (np.stack([x, y, np.ones_like(x)], -1) @ inv["kinv"].T) @ inv["c2w"][:, :3].T
    o = inv["c2w"][:, 3] - np.array(M.SPHERE_C)
    a, b, c = (d * d).sum(-1), (d * o).sum(-1), (o * o).sum() - (M.SPHERE_R - shrink) ** 2
    return b * b - a * c > 0


# ------------------------------------------------------------------------------------------------ refusals
def assert_refusals(hip):
    """every MNERF_E_* the header names for the two entry points and the workspace size, from fake addresses: each call fails its
    checks before any HIP call"""
    import ctypes as C
    lib = hip.load()
    fake, odd4, odd8, odd16 = C.c_void_p(0x10000), C.c_void_p(0x10002), C.c_void_p(0x10004), C.c_void_p(0x10008)
    i32 = lambda p: None if p is None else C.cast(p, C.POINTER(C.c_int32))
    r, n, a = hip.MNERF_E_RANGE, hip.MNERF_E_NULL, hip.MNERF_E_ALIGN
    big_v, big_t = 1 << 31, ((1 << 31) - 1) // 3 + 1
    cam = F.arc_cameras(2, 8, 8)[0]
    good = hip.make_view(cam["extr"], cam["intr"], cam["near"], cam["far"])
    singular = hip.make_view(cam["extr"], np.zeros((3, 3)), 0.5, 6.0)
    flat = hip.make_view(np.zeros((3, 4)), cam["intr"], 0.5, 6.0)
    for hw, want in (((0, 8), -1), ((8, 0), -1), ((-1, 8), -1), ((65536, 32768), -1), ((8, 8), 512), ((1, 1), 8), ((37, 53), 8 * 37 * 53),
                     ((32768, 65535), 8 * 32768 * 65535)):
        assert hip.mesh_raster_workspace_bytes(*hw) == want, hw

    def raster(vert=fake, tri=fake, v=8, t=4, view=good, h=8, w=8, face=fake, depth=fake, bary=fake, ws=fake, ws_bytes=512):
        return lib.mnerf_mesh_raster(vert, i32(tri), v, t, None if view is None else C.byref(view), h, w, 0, i32(face), depth, bary, ws,
                                     ws_bytes, None)

    cases = [(r, dict(v=-1)), (r, dict(v=big_v)), (r, dict(t=-1)), (r, dict(t=big_t)), (r, dict(h=0)), (r, dict(w=0)),
             (r, dict(h=65536, w=32768, ws_bytes=1 << 62)), (r, dict(ws_bytes=511)), (r, dict(ws_bytes=-1)), (r, dict(view=singular)),
             (r, dict(view=flat)), (r, dict(ws_bytes=0, face=None)),  # RANGE precedes NULL
             (n, dict(view=None)), (n, dict(face=None)), (n, dict(depth=None)), (n, dict(bary=None)), (n, dict(ws=None)), (n, dict(vert=None)),
             (n, dict(tri=None)), (n, dict(t=0, face=None)), (n, dict(face=None, vert=odd16)),  # NULL precedes ALIGN
             (a, dict(vert=odd16)), (a, dict(ws=odd8)), (a, dict(tri=odd4)), (a, dict(face=odd4)), (a, dict(depth=odd4)), (a, dict(bary=odd4))]
    for want, kwargs in cases:
        assert raster(**kwargs) == want, ("raster", kwargs, want, lib.mnerf_last_error())

    aw, ah = X.atlas_size(4, 8)[:2]

    def shade(vert=fake, tri=fake, v=8, t=4, face=fake, bary=fake, h=8, w=8, atlas=None, ah=ah, aw=aw, block=8, view=good, rgba=fake,
              normal=None):
        return lib.mnerf_mesh_shade(vert, i32(tri), v, t, i32(face), bary, h, w, atlas, ah, aw, block, None if view is None else C.byref(view),
                                    rgba, normal, None)

    cases = [(r, dict(v=-1)), (r, dict(v=big_v)), (r, dict(t=-1)), (r, dict(t=big_t)), (r, dict(h=0)), (r, dict(w=0)), (r, dict(h=65536, w=32768)),
             (r, dict(atlas=fake, block=3)), (r, dict(atlas=fake, block=65)), (r, dict(atlas=fake, aw=aw + 8)), (r, dict(atlas=fake, ah=ah - 8)),
             (r, dict(atlas=fake, block=4)), (r, dict(atlas=fake, t=2 * 4096 * 4096 + 1, block=4, aw=16388, ah=16384)),
             (r, dict(view=singular)), (r, dict(view=flat)), (r, dict(h=0, rgba=None)),
             (n, dict(view=None)), (n, dict(face=None)), (n, dict(bary=None)), (n, dict(rgba=None)), (n, dict(vert=None)), (n, dict(tri=None)),
             (n, dict(rgba=None, vert=odd16)),
             (a, dict(vert=odd16)), (a, dict(atlas=odd16)), (a, dict(rgba=odd16)), (a, dict(normal=odd16)), (a, dict(tri=odd4)),
             (a, dict(face=odd4)), (a, dict(bary=odd4))]
    for want, kwargs in cases:
        assert shade(**kwargs) == want, ("shade", kwargs, want, lib.mnerf_last_error())


# ------------------------------------------------------------------------------------------------ visibility against the mesh
VISIBILITY_CASE = (3, 24, 32, False)  # K, h, w, legacy of the plane + box scene


def open_cameras(cams):
    """the cameras with the depth range fusion.mesh_depths gives them: nothing the mesh shows is clipped, 0 (no hit) is not VALID"""
    return [dict(c, near=float(np.finfo(np.float32).tiny), far=3.0e38) for c in cams]


def dilate(depth):
    """fusion.mesh_depths' fill: a pixel without a hit (0) takes the smallest hit depth of its eight neighbours, 0 if none has one"""
    d = np.asarray(depth)
    big = np.where(d > 0, d, np.inf)
    pad = np.pad(big, ((0, 0), (1, 1), (1, 1)), constant_values=np.inf)
    h, w = d.shape[1:]
    near = np.min([pad[:, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy in (-1, 0, 1) for dx in (-1, 0, 1)], 0)
    return np.where(d > 0, d, np.where(np.isfinite(near), near, 0)).astype(d.dtype)


@functools.lru_cache(maxsize=None)
def visibility_shares(cell=DECIMATE_CELL, block=SCENE_BLOCK):
    """the decimated plane + box mesh textured with both visibility tests by the float64 restatements -> dict(views=(share of the owned
    texels with a = 1, colour RMS of mesh_texture_helpers.colour_errors), mesh=the same, vertices, faces, scene)"""
    k, h, w, legacy = VISIBILITY_CASE
    s = X.scene(k, h, w, legacy, "plain", False)
    dims = tuple(int(np.ceil(d / cell)) for d in s["dims"])
    m = D.decimate(s["vertices"], s["faces"], s["origin"], cell * s["voxel"], dims)
    vertices, faces = m["vertices"].astype(np.float32), m["faces"].astype(np.int32)
    owned = X.layout(len(faces), block)["owner"] >= 0
    out = dict(vertices=vertices, faces=faces, scene=s)
    mesh_depth = np.stack([raster(vertices, faces, dict(c, near=0.0, far=3.0e38), h, w, legacy)["depth"] for c in s["cams"]]).astype(np.float32)
    mesh_depth = dilate(mesh_depth)
    for mode, cams, depth in (("views", s["cams"], s["depth"]), ("mesh", open_cameras(s["cams"]), mesh_depth)):
        acc, _ = X.accumulate(vertices, faces, block, cams, h, w, legacy, depth, None, s["rgb"])
        atlas = X.resolve(vertices, faces, block, acc)
        out[mode] = (float(atlas[..., 3][owned].mean()), X.colour_errors(vertices, faces, block, atlas, s["voxel"])[0])
    return out
