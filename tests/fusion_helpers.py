"""Geometry export (include/mnerf.h "GEOMETRY EXPORT") restated in numpy, and the analytic scene the tests run it on.

``consistency`` / ``point_rows`` / ``colormap`` follow the header's text operation by operation; ``dtype`` selects the arithmetic
(float64: the reference; float32: the same restatement in the device's format, whose distance from float64 sizes the gate of the
fused depth).  In float64 ``consistency`` also marks the BORDERLINE pixels, whose count may legitimately differ in fp32:
a reprojection error within 1e-3 px of px_tol, a relative depth error within 1e-5 of rel_tol, a projection within 1e-3 px of the
frame border (or a camera-z within 1e-6 of 0), within 1e-3 px of a texel boundary across which the validity of the four taps
changes, or a value within 1e-4 of near / far or an opacity within 1e-6 of min_opacity."""
import functools

import numpy as np

PX_TOL, REL_TOL, MIN_OPACITY = 1.0, 0.01, 0.5
BORDERLINE_CAP = 0.01  # share of a case's pixels that the GPU comparison may leave out
# (K, h, w): 24 x 32 = 3 workgroups of 256; 37 x 53 = 1961 pixels, odd sizes, the last wave ragged; 16 = MNERF_MAX_VIEWS
GPU_CASES = [(k, h, w, legacy) for (k, h, w) in ((2, 24, 32), (3, 24, 32), (5, 24, 32), (16, 37, 53)) for legacy in (True, False)]
VARIANTS = ("plain", "opacity", "invalid")


# ------------------------------------------------------------------------------------------------ analytic scene
def arc_cameras(k, h, w):
    """K pinhole cameras on an arc of radius 2.2 around the origin (angles linspace(-0.35, 0.35, K), a small height wobble), looking
    at the origin; f = 0.9 w, near / far = 0.5 / 6.  -> [dict(extr [3,4] f32, intr [3,3] f32, near, far)]"""
    cams = []
    for a in np.linspace(-0.35, 0.35, k):
        c = 2.2 * np.array([np.sin(a), 0.08 * np.sin(3.0 * a + 0.5), -np.cos(a)])
        fwd = -c / np.linalg.norm(c)
        right = np.cross(np.array([0.0, 1.0, 0.0]), fwd)
        right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        rot = np.stack([right, down, fwd])
        extr = np.concatenate([rot, (-rot @ c)[:, None]], 1).astype(np.float32)
        intr = np.array([[0.9 * w, 0, 0.5 * w], [0, 0.9 * w, 0.5 * h], [0, 0, 1]], np.float32)
        cams.append(dict(extr=extr, intr=intr, near=0.5, far=6.0))
    return cams


def inverse_cameras(cams, dtype):
    """what the library's host side does: kinv and [R^-1 | -R^-1 t] in double, then cast"""
    out = []
    for c in cams:
        e, k = c["extr"].astype(np.float64), c["intr"].astype(np.float64)
        ri = np.linalg.inv(e[:, :3])
        out.append(dict(kinv=np.linalg.inv(k).astype(dtype), c2w=np.concatenate([ri, (-ri @ e[:, 3])[:, None]], 1).astype(dtype),
                        extr=c["extr"].astype(dtype), intr=c["intr"].astype(dtype)))
    return out


def pixel_centres(h, w, legacy, dtype=np.float64):
    off = 0.0 if legacy else 0.5
    y, x = np.meshgrid(np.arange(h, dtype=dtype) + dtype(off), np.arange(w, dtype=dtype) + dtype(off), indexing="ij")
    return x, y


def raycast(cam, h, w, legacy):
    """float64 camera-z depth of the plane z = 0 plus the box [-0.4, 0.3] x [-0.3, 0.35] x [-0.6, 0], through the camera as the
    device sees it (its float32 matrices)"""
    inv = inverse_cameras([cam], np.float64)[0]
    x, y = pixel_centres(h, w, legacy)
    d_cam = np.stack([x, y, np.ones_like(x)], -1) @ inv["kinv"].T  # camera-z = 1: the ray parameter is the depth
    d = d_cam @ inv["c2w"][:, :3].T
    o = inv["c2w"][:, 3]
    depth = -o[2] / d[..., 2]
    lo, hi = np.array([-0.4, -0.3, -0.6]), np.array([0.3, 0.35, 0.0])
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (lo - o) / d, (hi - o) / d
    enter, leave = np.minimum(t0, t1).max(-1), np.maximum(t0, t1).min(-1)
    hit = (enter <= leave) & (enter > 0)
    return np.where(hit, np.minimum(enter, depth), depth)


@functools.lru_cache(maxsize=None)
def scene(k, h, w, legacy, variant="plain"):
    """-> dict(cams, depth [K,h,w] f32, opacity [K,h,w] f32 or None, outliers [h,w] bool: the planted pixels of view 0)"""
    rng = np.random.default_rng(1000 * k + h + (1 if legacy else 0))
    cams = arc_cameras(k, h, w)
    depth = np.stack([raycast(c, h, w, legacy) for c in cams]).astype(np.float32)
    outliers = rng.random((h, w)) < 0.05
    depth[0][outliers] *= np.float32(1.1)
    opacity = None
    if variant == "opacity":  # the maps carry opacity-weighted depth; a stripe of view 1 is nearly transparent
        opacity = rng.uniform(0.8, 1.0, depth.shape).astype(np.float32)
        opacity[1 % k, :, w // 3:w // 3 + 4] = np.float32(0.2)
        depth = depth * opacity
    if variant == "invalid":
        for value in (np.nan, np.inf, -np.inf, 0.0, -1.0, 0.25, 7.0):  # non-finite, non-positive, below near, beyond far
            sel = rng.random(depth.shape) < 0.005
            depth[sel] = np.float32(value)
    return dict(cams=cams, depth=depth, opacity=opacity, outliers=outliers)


# ------------------------------------------------------------------------------------------------ a. consistency
def lift(inv, x, y, z):
    cam = np.stack([x, y, np.ones_like(x)], -1) @ inv["kinv"].T * z[..., None]
    return cam @ inv["c2w"][:, :3].T + inv["c2w"][:, 3]


def proj(inv, world):
    q = (world @ inv["extr"][:, :3].T + inv["extr"][:, 3]) @ inv["intr"].T
    with np.errstate(divide="ignore", invalid="ignore"):
        return q[..., 0] / q[..., 2], q[..., 1] / q[..., 2], q[..., 2]


def values(cams, depth, opacity, min_opacity, dtype):
    """-> z [K,h,w], valid [K,h,w], edge [K,h,w] (validity decided by a margin fp32 may not respect)"""
    z = depth.astype(dtype)
    valid = np.ones(depth.shape, bool)
    edge = np.zeros(depth.shape, bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        if opacity is not None:
            o = opacity.astype(dtype)
            valid &= o >= dtype(min_opacity)
            edge |= np.abs(o - min_opacity) < 1e-6
            z = z / o
        for k, c in enumerate(cams):
            valid[k] &= np.isfinite(z[k]) & (z[k] >= dtype(c["near"])) & (z[k] <= dtype(c["far"]))
            edge[k] |= (np.abs(z[k] - c["near"]) < 1e-4) | (np.abs(z[k] - c["far"]) < 1e-4)
    return z, valid, edge


def taps(fx, fy, h, w):
    x0 = np.clip(np.minimum(np.floor(fx), w - 2), 0, None).astype(np.int64)
    y0 = np.clip(np.minimum(np.floor(fy), h - 2), 0, None).astype(np.int64)
    return x0, y0, np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)


def consistency(cams, ref, h, w, legacy, depth, opacity=None, px_tol=PX_TOL, rel_tol=REL_TOL, min_opacity=MIN_OPACITY,
                dtype=np.float64):
    """-> fused [h,w] (dtype), n_consistent [h,w] int32, borderline [h,w] bool"""
    inv = inverse_cameras(cams, dtype)
    z_all, valid_all, edge_all = values(cams, depth, opacity, min_opacity, dtype)
    off = dtype(0.0 if legacy else 0.5)
    x, y = pixel_centres(h, w, legacy, dtype)
    ok_ref = valid_all[ref]
    z = np.where(ok_ref, z_all[ref], dtype(1.0))
    world = lift(inv[ref], x, y, z)
    count = np.zeros((h, w), np.int32)
    total = z.copy()
    border = edge_all[ref].copy()
    u_hi, v_hi = dtype(w - 1) + off, dtype(h - 1) + off
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(len(cams)):
            if j == ref:
                continue
            u, v, zj = proj(inv[j], world)
            inside = (zj > 0) & (u >= off) & (u <= u_hi) & (v >= off) & (v <= v_hi)
            near_frame = (np.abs(zj) < 1e-6) | (np.minimum(np.abs(u - off), np.abs(u - u_hi)) < 1e-3) | \
                (np.minimum(np.abs(v - off), np.abs(v - v_hi)) < 1e-3)
            fx, fy = np.where(inside, u - off, dtype(0)), np.where(inside, v - off, dtype(0))
            x0, y0, x1, y1 = taps(fx, fy, h, w)

            def all_valid(x0, y0, x1, y1):
                return valid_all[j][y0, x0] & valid_all[j][y0, x1] & valid_all[j][y1, x0] & valid_all[j][y1, x1]

            ok = inside & all_valid(x0, y0, x1, y1)
            tap_edge = edge_all[j][y0, x0] | edge_all[j][y0, x1] | edge_all[j][y1, x0] | edge_all[j][y1, x1]
            for sx in (-1e-3, 1e-3):  # the tap set an fp32 projection may pick instead
                for sy in (-1e-3, 1e-3):
                    moved = taps(np.clip(fx + sx, 0, w - 1), np.clip(fy + sy, 0, h - 1), h, w)
                    tap_edge |= all_valid(*moved) != all_valid(x0, y0, x1, y1)
            ax, ay = fx - x0.astype(dtype), fy - y0.astype(dtype)
            zt = np.where(valid_all[j], z_all[j], dtype(1.0))
            top = zt[y0, x0] + ax * (zt[y0, x1] - zt[y0, x0])
            bot = zt[y1, x0] + ax * (zt[y1, x1] - zt[y1, x0])
            dj = top + ay * (bot - top)
            xr, yr, dr = proj(inv[ref], lift(inv[j], u, v, dj))
            err = np.hypot(xr - x, yr - y)
            rel = np.abs(dr - z)
            good = ok & ok_ref & (err < dtype(px_tol)) & (rel < dtype(rel_tol) * z)
            count += good
            total = total + np.where(good, dr, dtype(0))
            border |= ok_ref & (near_frame | (inside & tap_edge) |
                                (ok & ((np.abs(err - px_tol) < 1e-3) | (np.abs(rel / z - rel_tol) < 1e-5))))
    fused = np.where(ok_ref, total / (1 + count).astype(dtype), dtype(0))
    return fused, np.where(ok_ref, count, 0).astype(np.int32), border & ok_ref


@functools.lru_cache(maxsize=None)
def reference(k, h, w, legacy, variant="plain"):
    """the float64 and float32 restatements of every view of a scene as the reference view -> [dict(fused, count, border,
    fused32, count32)] * K; computed once and shared (read-only)"""
    s = scene(k, h, w, legacy, variant)
    out = []
    for ref in range(k):
        fused, count, border = consistency(s["cams"], ref, h, w, legacy, s["depth"], s["opacity"])
        fused32, count32, _ = consistency(s["cams"], ref, h, w, legacy, s["depth"], s["opacity"], dtype=np.float32)
        out.append(dict(fused=fused, count=count, border=border, fused32=fused32, count32=count32))
    return out


# ------------------------------------------------------------------------------------------------ b. point cloud
def point_rows(cam, h, w, legacy, depth, rgb, n_consistent, min_consistent, dtype=np.float64):
    """the selected pixels in pixel order -> (index [M], rows [M, 8] dtype)"""
    d = np.asarray(depth).reshape(-1)
    with np.errstate(invalid="ignore"):
        keep = np.isfinite(d) & (d > 0)
    keep &= np.asarray(n_consistent).reshape(-1) >= min_consistent
    idx = np.flatnonzero(keep)
    x, y = pixel_centres(h, w, legacy, dtype)
    inv = inverse_cameras([cam], dtype)[0]
    xyz = lift(inv, x.reshape(-1)[idx], y.reshape(-1)[idx], d[idx].astype(dtype))
    n = np.asarray(n_consistent).reshape(-1)[idx]
    return idx, np.concatenate([xyz, d[idx, None].astype(dtype), np.asarray(rgb).reshape(-1, 3)[idx].astype(dtype),
                                n[:, None].astype(dtype)], 1)


# ------------------------------------------------------------------------------------------------ c. colour map
def colormap(depth, lo, hi, dtype=np.float64):
    """visualize_depth's arithmetic with the index clamped, then JET as the header's formula -> uint8 [..., 3]"""
    d = np.nan_to_num(np.asarray(depth).astype(dtype), nan=0.0, posinf=np.finfo(dtype).max, neginf=-np.finfo(dtype).max)
    with np.errstate(over="ignore"):
        t = dtype(255) * ((d - dtype(lo)) / dtype(float(hi) - float(lo) + 1e-8))
    index = np.clip(np.trunc(np.clip(t, 0, 255)), 0, 255).astype(np.int64)
    return np.stack([np.clip(383 - np.abs(4 * index - c), 0, 255) for c in (765, 510, 255)], -1).astype(np.uint8)


def jet_float(index):
    """the same map from its real-valued statement: 255 clamp(1.5 - |4 s - c|) rounded half up, with exact rationals"""
    from fractions import Fraction
    out = np.zeros((len(index), 3), np.uint8)
    for r, i in enumerate(index):
        s = Fraction(int(i), 255)
        for ch, c in enumerate((3, 2, 1)):
            v = min(max(Fraction(3, 2) - abs(4 * s - c), 0), 1) * 255
            out[r, ch] = int(v + Fraction(1, 2))  # floor(v + 1/2)
    return out


# ------------------------------------------------------------------------------------------------ PLY
def read_ply(path):
    """-> (xyz float32 [M,3], rgb uint8 [M,3]) of a binary little-endian PLY with float xyz + uchar rgb vertices"""
    with open(path, "rb") as f:
        blob = f.read()
    end = blob.index(b"end_header\n") + len(b"end_header\n")
    lines = blob[:end].decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0", lines[:2]
    count = int(next(l for l in lines if l.startswith("element vertex")).split()[-1])
    props = [l.split()[1:] for l in lines if l.startswith("property")]
    assert props == [["float", "x"], ["float", "y"], ["float", "z"], ["uchar", "red"], ["uchar", "green"], ["uchar", "blue"]], props
    body = np.frombuffer(blob[end:], dtype=[("xyz", "<f4", 3), ("rgb", "u1", 3)])
    assert len(body) == count and len(blob) - end == 15 * count, (len(body), count)
    return body["xyz"].copy(), body["rgb"].copy()
