"""Shared by the target-grid tests: the CPU oracle's building blocks composed with the TARGET grid as a parameter (O.render_rays
takes the views' size for it), the golden scenes on the device, and the float32 restatement of the box filter."""
import numpy as np
import torch
import torch.nn.functional as F

from gpu_helpers import images_rgba, pair_feats_to_pair_major, ref_layout_to_pair_major
from helpers import golden_case, split_poses
from oracle import matchnerf_oracle as O

SCENES = ("c1_default", "nonlegacy")  # the smallest committed scene of each pixel convention (legacy / pixel centres at +0.5)


def _fma(a, b, c):
    """fl32(a * b + c) with ONE rounding: the product of two float32 is exact in x87 extended precision (64-bit significand), the
    sum rounds there once more only in cases of probability 2^-40 per operation"""
    return (a.astype(np.longdouble) * np.longdouble(b) + c.astype(np.longdouble)).astype(np.float32)


def project_to_view_chain(pts, extr, intr, width, height, near, far):
    """O.project_to_view with its two tiny contractions ([N,4]@[4,3], [N,3]@[3,3]) evaluated as the k-ordered FMA chain
    acc = x0 w0; acc = fma(xk, wk, acc) - the arithmetic of the reference's CPU path that the goldens record and the kernels pin
    (csrc/common.hpp), every other operation as the oracle writes it.  torch's CPU matmul gives exactly this on some hosts and a
    differently rounded sum on others (an ulp in a quarter of the values), and an ulp of (u, v, z) is a 1e-4-class change of the
    positional encoding's sin / cos at 2^9 pi and flips a visibility mask at the image border: expected values must not depend on
    the host that computes them."""
    x = pts.detach().numpy().astype(np.float32)
    e, k = extr.numpy().astype(np.float32), intr.numpy().astype(np.float32)
    x0, x1, x2 = x[..., 0], x[..., 1], x[..., 2]
    cam = [(_fma(x2, e[r, 2], _fma(x1, e[r, 1], x0 * e[r, 0])) + e[r, 3]).astype(np.float32) for r in range(3)]
    q = [_fma(cam[2], k[r, 2], _fma(cam[1], k[r, 1], cam[0] * k[r, 0])) for r in range(3)]
    q = [torch.from_numpy(v) for v in q]
    u = q[0] / q[2] / (width - 1)
    v = q[1] / q[2] / (height - 1)
    z = (q[2] - near) / (far - near)
    return torch.stack([u, v, z], -1)


def target_rays_chain(height, width, extr_t, intr_t, legacy=True):
    """O.target_rays with its contractions ([HW,3]@[3,3] pixel -> camera, [HW,4]@[4,3] camera -> world) as the same k-ordered FMA
    chain (see ``project_to_view_chain``; the host's BLAS changes its summation with the row count: 8192 pixels round differently
    from 4623 on the same machine); the pixel grid, the inverse intrinsics and the camera -> world matrix as the oracle builds them."""
    off = 0.0 if legacy else 0.5
    ys = torch.arange(height, dtype=torch.float32) + off
    xs = torch.arange(width, dtype=torch.float32) + off
    gy, gx = torch.meshgrid(ys, xs, indexing="ij")
    x, y = gx.reshape(-1).numpy(), gy.reshape(-1).numpy()
    kinv = intr_t.inverse().numpy().astype(np.float32)
    if legacy:
        sq = torch.eye(4)
        sq[:3] = extr_t
        c2w = sq.double().inverse()[:3].float()
    else:
        rot_inv = extr_t[:, :3].t()
        c2w = torch.cat([rot_inv, -(rot_inv @ extr_t[:, 3:])], 1)
    c2w = c2w.numpy().astype(np.float32)
    cam = [(_fma(y, kinv[r, 1], x * kinv[r, 0]) + kinv[r, 2]).astype(np.float32) for r in range(3)]  # [x y 1] . kinv[r]
    world = [(_fma(cam[2], c2w[r, 2], _fma(cam[1], c2w[r, 1], cam[0] * c2w[r, 0])) + c2w[r, 3]).astype(np.float32) for r in range(3)]
    center = np.broadcast_to(c2w[:, 3], (height * width, 3)).copy()  # [0 0 0 1] . c2w[r]
    ray = np.stack(world, -1) - center
    return torch.from_numpy(center), torch.from_numpy(ray)


def oracle_frame(cfg, sd, batch, pair_feats, tgt_hw, tgt_intr, ray_idx=None, setbg_opaque=False, chunk=None, chain=False):
    """O.render_rays with the target grid made a parameter: rays of a (h', w') grid with intrinsics ``tgt_intr``; everything that
    reads the SOURCE views (cost volume, projection into view 0) keeps their size.  ``chunk``: rays per pass (memory only).
    ``chain``: the target rays and the projections into the source views through ``target_rays_chain`` /
    ``project_to_view_chain`` (host-independent bits) instead of O.target_rays / O.project_to_view
    (tests/test_target_grid_cpu.py holds each pair together)."""
    if chain:
        plain = O.project_to_view, O.target_rays
        O.project_to_view, O.target_rays = project_to_view_chain, target_rays_chain
        try:
            return oracle_frame(cfg, sd, batch, pair_feats, tgt_hw, tgt_intr, ray_idx, setbg_opaque, chunk)
        finally:
            O.project_to_view, O.target_rays = plain
    te, _, tn, se, si, sn = split_poses(batch)
    v = cfg.n_src_views
    src_images = batch["images"][0, :v]
    height, width = src_images.shape[-2:]
    center, ray = O.target_rays(tgt_hw[0], tgt_hw[1], te, tgt_intr, cfg.legacy_coord)  # (module attribute: see ``chain``)
    if ray_idx is not None:
        center, ray = center[ray_idx], ray[ray_idx]
    n = ray.shape[0]
    parts = []
    for c in range(0, n, chunk or n):
        ce, r = center[c:c + (chunk or n)], ray[c:c + (chunk or n)]
        d = O.depth_samples(cfg, tn[0], tn[1], r.shape[0])
        pts = ce[:, None] + r[:, None] * d[..., None]
        cond, mask = O.cost_volume_cond(cfg, pts, se, si, sn, src_images, pair_feats, height, width)
        x_ref = O.project_to_view(pts, se[0], si[0], width, height, sn[0, 0], sn[0, 1])  # (module attribute: see ``chain``)
        dir_ref = F.normalize(r, dim=-1) @ se[0][:, :3].t()
        rgb_s, sigma = O.decoder(cfg, sd, x_ref, dir_ref, cond, mask)
        rgb, depth, opacity, _ = O.composite(cfg, r, rgb_s, sigma, d, setbg_opaque)
        parts.append(dict(rgb=rgb, depth=depth, opacity=opacity, cond=cond, x_ref=x_ref, rgb_samples=rgb_s, sigma=sigma,
                          depth_samples=d, pts=pts))
    return {k: torch.cat([p[k] for p in parts], 0) for k in parts[0]}


_CASES = {}


def case(name):
    """-> (golden, cfg, state dict, batch, pair-major maps [P,2,h,w,128] per scale on the host, oracle-layout pair_feats); cached"""
    if name not in _CASES:
        g, cfg, sd, batch = golden_case(name)
        v = cfg.n_src_views
        if "feat_scale0" in g:
            feats_pm = [ref_layout_to_pair_major(torch.from_numpy(g[f"feat_scale{i}"]), v) for i in range(2)]
        else:
            with torch.no_grad():
                feats_pm = pair_feats_to_pair_major(O.encode_pairs(cfg, sd, batch["images"][0, :v]))
        pair_feats = [(f[:, 0].permute(0, 3, 1, 2).contiguous(), f[:, 1].permute(0, 3, 1, 2).contiguous()) for f in feats_pm]
        _CASES[name] = (g, cfg, sd, batch, feats_pm, pair_feats)
    return _CASES[name]


def sizes(name):
    """tag -> (h', w') in the order the tests run them: smaller than the source first, then the ones with more pixels"""
    _, _, _, batch, _, _ = case(name)
    h, w = batch["images"].shape[-2:]
    return {"half": (h // 2, w // 2), "tiny": (5, 7), "zoom": (h // 2, w // 2), "plus": (h + 3, w + 5), "tall": (2 * h, w)}


def target_intrinsics(name, tag):
    """the batch's target camera on the grid ``tag`` (camera.resize_intrinsics); "zoom": an unrelated K' - a zoomed, off-centre crop"""
    from matchnerf_amd import camera
    _, cfg, _, batch, _, _ = case(name)
    h, w = batch["images"].shape[-2:]
    th, tw = sizes(name)[tag]
    K = batch["intrinsics"][0, -1]
    if tag == "zoom":
        Kz = K.clone()
        Kz[0, 0], Kz[1, 1] = 1.75 * K[0, 0], 1.6 * K[1, 1]
        Kz[0, 2], Kz[1, 2] = 0.41 * tw, 0.63 * th
        return Kz
    return camera.resize_intrinsics(K, (h, w), (th, tw), cfg.legacy_coord)


_FRAMES = {}


def expected_rays(name, tag, limit=1536):
    """the target pixels the oracle evaluates: all of them for a small grid; for a larger one the frame's border (first / last row
    and column: where tile tails and a wrong stride show first) and a regular lattice of the rest (an odd stride: every column
    and every position inside an 8 x 4 tile occurs) - the oracle costs seconds per thousand rays on a CPU"""
    th, tw = sizes(name)[tag]
    n = th * tw
    if n <= limit:
        return torch.arange(n)
    pix = torch.arange(n)
    py, px = pix // tw, pix % tw
    border = (py == 0) | (py == th - 1) | (px == 0) | (px == tw - 1)
    stride = 2 * (n // 1600) + 5
    return pix[border | (pix % stride == 0)]


def expected(name, tag):
    """the oracle's values on the grid ``tag`` of scene ``name`` at ``expected_rays``: computed once, shared by the tests, never
    modified.  -> dict of stages + "idx" (the pixel indices, LongTensor)"""
    if (name, tag) not in _FRAMES:
        g, cfg, sd, batch, _, pair_feats = case(name)
        idx = expected_rays(name, tag)
        with torch.no_grad():
            out = oracle_frame(cfg, sd, batch, pair_feats, sizes(name)[tag], target_intrinsics(name, tag), ray_idx=idx,
                               setbg_opaque=g["meta"]["setbg_opaque"], chunk=1024, chain=True)
        out["idx"] = idx
        _FRAMES[name, tag] = out
    return _FRAMES[name, tag]


def scene_on_gpu(name):
    from gpu_helpers import make_scene_struct
    _, cfg, _, batch, feats_pm, _ = case(name)
    feats_gpu = [f.cuda() for f in feats_pm]
    img_gpu = images_rgba(batch["images"][0, :cfg.n_src_views]).cuda()
    return make_scene_struct(cfg, batch, feats_gpu, img_gpu), (feats_gpu, img_gpu)


def rays_struct(name, tag, n_rays=None, ray_begin=0, ray_idx_gpu=None, intr=None, tgt_hw=None):
    from matchnerf_amd import camera, hip
    _, cfg, _, batch, _, _ = case(name)
    h, w = batch["images"].shape[-2:]
    th, tw = tgt_hw or sizes(name)[tag]
    kinv, c2w = camera.target_ray_consts(batch["extrinsics"][0, -1, :3], target_intrinsics(name, tag) if intr is None else intr,
                                         cfg.legacy_coord)
    return hip.make_rays(th * tw if n_rays is None else n_rays, cfg.sample_intvs, h, w, kinv, c2w, float(batch["near_fars"][0, -1, 0]),
                         float(batch["near_fars"][0, -1, 1]), ray_begin=ray_begin, legacy=cfg.legacy_coord,
                         depth_inverse=(cfg.depth_param == "inverse"),
                         ray_idx_ptr=ray_idx_gpu.data_ptr() if ray_idx_gpu is not None else None, tgt_hw=(th, tw))


def box_downsample_f32(src, k):
    """mnerf_box_downsample restated in numpy float32: the k x k block summed in row-major order with sequential additions,
    times fp32(1 / k^2).  src [k h, k w, C] -> [h, w, C]."""
    src = np.asarray(src, np.float32)
    hk, wk, c = src.shape
    h, w = hk // k, wk // k
    blocks = src.reshape(h, k, w, k, c)
    acc = blocks[:, 0, :, 0].copy()
    for dy in range(k):
        for dx in range(k):
            if dy or dx:
                acc = acc + blocks[:, dy, :, dx]
    return acc * np.float32(1.0 / (k * k))
