"""The ray chunk's training backward (matchnerf_amd/autograd.py: _RayChunkFn) at the shapes training runs (1 024 random rays,
64 stratified samples: configs/train.yaml): the cost-volume backward on its own and the whole chunk; and the cost volume's forward
at odd feature-map sizes (756 x 1008 frames).

One reference rule throughout: ray geometry in float32 exactly as the oracle computes it (pinned bit-exact to the kernels by
test_hip_kernels.py::test_ray_geometry_is_bit_exact); from the bilinear taps on, float64 autograd through the oracle's own pieces
(O.bilinear_border, O.group_cosine, O.decoder, O.composite).

The cost-volume backward's walk (csrc/backward.hip: cost_volume_backward_walk_kernel) splits each ray's samples into segments and
loops over rounds when the grid is capped; every case names the (segments, rounds) regime it pins through ``walk_regime``, a mirror
of the launch arithmetic: if the heuristic is retuned the case fails loudly instead of quietly testing another regime.
"""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from gpu_helpers import ReluKinks, images_rgba, make_rays_struct, make_scene_struct
from helpers import golden_case, linf, split_poses
from matchnerf_amd import camera, synthetic as syn
from oracle import matchnerf_oracle as O
from test_hip_kernels import _case_on_gpu

pytestmark = pytest.mark.gpu

GATE = 2e-5  # cost volume (forward cosines, backward map gradients per scale): tests/test_hip_kernels.py's gate


@pytest.fixture(scope="module")
def hip():
    from matchnerf_amd import hip as h
    h.load()
    assert torch.cuda.is_available(), "the gpu-marked tests need a GPU"
    return h


def walk_regime(n_rays, n_views, n_scales, n_samples, segs=0):
    """-> (segments per ray, rounds of the grid-stride loop) of the walk; mirrors the launch arithmetic of
    mnerf_cost_volume_backward (csrc/backward.hip, the ``if (walk)`` branch) and the loop bound of
    cost_volume_backward_walk_kernel.  ``segs``: the MNERF_CV_BWD_SEGS override."""
    items = n_rays * (n_views * (n_views - 1) // 2) * n_scales
    n_seg = segs if segs > 0 else (16 * 1536 + items - 1) // items
    n_seg = max(1, min(n_seg, n_samples // 8))
    items *= n_seg
    blocks = min((items + 15) // 16, 8192)
    slots = blocks * 256 // 16
    return n_seg, (items + slots - 1) // slots


# ----------------------------------------------------------------------------- scenes


def _synthetic(height, width, n_views, seed):
    """syn.make_scene poses and images with random feature maps at 1/8 and 1/4 of the frame (ceil: the encoder's stride-2 sizes,
    odd for a 756 x 1008 frame) -> (cfg, batch, pair-major maps [P,2,h,w,128] per scale, source images [V,3,H,W])"""
    batch = {k: torch.from_numpy(v) for k, v in syn.make_scene(height, width, n_views, seed=seed).items()}
    cfg = O.OracleConfig(n_src_views=n_views)
    gen = torch.Generator().manual_seed(seed)
    n_pairs = n_views * (n_views - 1) // 2
    feats = [torch.randn(n_pairs, 2, -(-height // f), -(-width // f), 128, generator=gen) for f in (8, 4)]
    return cfg, batch, feats, batch["images"][0, :n_views]


def _scene(spec):
    if spec[0] == "syn":
        return _synthetic(*spec[1:])
    g, cfg, sd, batch, feats_gpu, _ = _case_on_gpu(spec)
    return cfg, batch, [f.cpu() for f in feats_gpu], batch["images"][0, :cfg.n_src_views]


def _grids(cfg, batch, idx, u):
    """float32 geometry exactly as O.render_rays / O.cost_volume_cond form it -> (per-view normalised grids [R,S,2] and
    in-frustum masks [R,S], both float32; sample depths [R,S]; ray origins and directions [R,3]; points [R,S,3])"""
    te, ti, tn, se, si, sn = split_poses(batch)
    h, w = batch["images"].shape[-2:]
    center, ray = O.target_rays(h, w, te, ti, cfg.legacy_coord)
    center, ray = center[idx], ray[idx]
    d = O.depth_samples(cfg, tn[0], tn[1], idx.numel(), u)
    pts = center[:, None] + ray[:, None] * d[..., None]
    grids, masks = [], []
    for v in range(cfg.n_src_views):
        g = O.project_to_view(pts, se[v], si[v], w, h, sn[v, 0], sn[v, 1])[..., :2] * 2.0 - 1.0
        grids.append(g)
        masks.append(((g[..., 0] > -1.0) & (g[..., 0] < 1.0) & (g[..., 1] > -1.0) & (g[..., 1] < 1.0)).float())
    return grids, masks, d, ray, pts


def _cond64(cfg, grids, masks, images, pair_feats):
    """O.cost_volume_cond from the float32 grids on, in float64: pair_feats = per scale (f0, f1) [P,C,h,w] float64"""
    pairs = O.pair_list(cfg.n_src_views)
    g64 = [g.double() for g in grids]
    colors = [O.bilinear_border(images[v].double(), g[..., 0], g[..., 1]) for v, g in enumerate(g64)]
    feats = []
    for scale, (f0, f1) in enumerate(pair_feats):
        acc = 0
        for p, (a, b) in enumerate(pairs):
            fa = O.bilinear_border(f0[p], g64[a][..., 0], g64[a][..., 1])
            fb = O.bilinear_border(f1[p], g64[b][..., 0], g64[b][..., 1])
            acc = acc + O.group_cosine(fa, fb, cfg.cos_n_group[scale])
        feats.append(acc / len(pairs))
    mask = torch.stack(masks, -1).double()
    return torch.cat([torch.cat(feats, 0).permute(1, 2, 0), torch.cat(colors, 0).permute(1, 2, 0), mask], -1), mask


def _map_grads(cfg, grids, feats, g_cond, dtype=torch.float64, chunk=1 << 15):
    """gradient of sum(cond[..., cosines] * g_cond) w.r.t. both maps of every pair and scale -> [P,2,h,w,128] per scale, evaluated in
    ``dtype`` from the float32 grids on (float32: the fp32 oracle's own arithmetic).
    One (scale, pair) and at most ``chunk`` samples at a time: a pair's cosines depend on its own two maps only."""
    n, s = grids[0].shape[:2]
    pairs = O.pair_list(cfg.n_src_views)
    g64 = [g.to(dtype) for g in grids]
    g = g_cond.to(dtype)[:, :sum(cfg.cos_n_group)].reshape(n, s, -1)
    step, off, out = max(1, chunk // s), 0, []
    for scale, f in enumerate(feats):
        n_g = cfg.cos_n_group[scale]
        per_pair = []
        for p, (a, b) in enumerate(pairs):
            f0, f1 = (f[p, k].permute(2, 0, 1).to(dtype).requires_grad_(True) for k in (0, 1))
            for r0 in range(0, n, step):
                r = slice(r0, r0 + step)
                fa = O.bilinear_border(f0, g64[a][r, :, 0], g64[a][r, :, 1])
                fb = O.bilinear_border(f1, g64[b][r, :, 0], g64[b][r, :, 1])
                cos = O.group_cosine(fa, fb, n_g)                                        # [G, r, S]
                (cos * g[r, :, off:off + n_g].permute(2, 0, 1)).sum().div(len(pairs)).backward()
            per_pair.append(torch.stack([f0.grad, f1.grad], 0))
        out.append(torch.stack(per_pair, 0).permute(0, 1, 3, 4, 2))
        off += n_g
    return out


# ----------------------------------------------------------------------------- 1. cost-volume backward vs float64

# name: (scene, rays, samples, stratified, (segments, rounds)); rays=None: the golden's own stage rays
CASES = {
    "train_shape": ("c1_default", 1024, 64, True, (4, 1)),
    "two_segments": ("c1_default", 2048, 64, False, (2, 1)),
    "one_segment_whole_image": ("c1_default", 4096, 64, True, (1, 1)),
    "uneven_segments_S33": ("c1_default", 24, 33, False, (4, 1)),       # 8, 8, 8, 9 samples
    "25_segments_S200": ("c1_default", 24, 200, True, (25, 1)),
    "two_rounds": ("c1_default", 24576, 8, False, (1, 2)),              # 147 456 items > 8 192 x 16 slots; pixels repeated
    "nonlegacy": ("nonlegacy", None, 32, True, (4, 1)),
    "inverse_depth": ("inverse_depth", None, 32, True, (4, 1)),
    "v4_six_pairs": ("v4", None, 32, False, (4, 1)),
    "ten_views": (("syn", 64, 64, 10, 3), 1024, 16, False, (1, 1)),    # 45 pairs: the pair decode past V = 4
    "training_maps": (("syn", 512, 640, 3, 5), 1024, 64, True, (4, 1)),  # maps 64 x 80 / 128 x 160
    "odd_maps": (("syn", 756, 1008, 3, 6), 1024, 64, True, (4, 1)),      # maps 95 x 126 / 189 x 252
    "short_focal": ("c1_default", 1024, 64, False, (4, 1)),             # border clamps: texels repeated within a cell
}


@pytest.mark.parametrize("case", list(CASES))
def test_cost_volume_backward_matches_float64(hip, case):
    """hip.cost_volume_backward on a random g_cond vs the float64 gradient of both maps of every pair and scale.
    Gate: 2e-5 of the largest float64 magnitude of that scale.  Under MNERF_CV_BWD_WALK=0 / MNERF_CV_BWD_SEGS (the child runs
    of test_cost_volume_backward_knobs) the per-sample kernel / the forced segment count run instead."""
    spec, n, s, stratified, regime = CASES[case]
    cfg, batch, feats, images = _scene(spec)
    cfg.sample_intvs = s
    h, w = batch["images"].shape[-2:]
    gen = torch.Generator().manual_seed(len(case))
    if case == "short_focal":  # neighbouring target pixels land many texels apart; samples beside the sources clamp at the border
        batch = {k: t.clone() for k, t in batch.items()}
        batch["intrinsics"][0, -1] = torch.tensor([[6.0, 0.0, w / 2.0], [0.0, 6.0, h / 2.0], [0.0, 0.0, 1.0]])
    if n is None:
        idx = torch.from_numpy(golden_case(spec)[0]["stage_rays"]).long()
        n = idx.numel()
    elif n > h * w:
        idx = torch.arange(h * w).repeat(-(-n // (h * w)))[:n]
    else:
        idx = torch.randperm(h * w, generator=gen)[:n]
    u = torch.rand(n, s, generator=gen) if stratified else None
    v = cfg.n_src_views
    walk = os.environ.get("MNERF_CV_BWD_WALK", "1")[:1] != "0"
    segs = int(os.environ.get("MNERF_CV_BWD_SEGS", "0") or 0)
    if walk and not segs:
        assert walk_regime(n, v, len(feats), s) == regime, walk_regime(n, v, len(feats), s)

    feats_gpu = [f.cuda() for f in feats]
    img_gpu = images_rgba(images).cuda()
    sc = make_scene_struct(cfg, batch, feats_gpu, img_gpu)
    idx_gpu = idx.int().cuda()
    rays = make_rays_struct(cfg, batch, n, ray_idx_gpu=idx_gpu)
    u_gpu = u.cuda() if u is not None else None
    rays.strat_u = u_gpu.data_ptr() if u is not None else None
    dc = sum(cfg.cos_n_group) + 4 * v
    cs = ((dc + 1 + 7) // 8) * 8
    g_cond = torch.zeros(n * s, cs)
    g_cond[:, :dc] = torch.randn(n * s, dc, generator=gen)
    got = hip.cost_volume_backward(sc, rays, cs, g_cond.cuda(), [torch.zeros_like(f) for f in feats_gpu])
    torch.cuda.synchronize()

    grids, masks, _, _, _ = _grids(cfg, batch, idx, u)
    if case == "short_focal":  # most samples project beyond a source frame (clamped cells), some stay inside
        inside = float(torch.stack(masks).mean())
        assert 0.0 < inside < 0.1, inside
    ref = _map_grads(cfg, grids, feats, g_cond)
    # maps beyond 16 x 16 (training-size and odd maps): texel coordinates up to ~250 in fp32 - the fp32 oracle's own error against
    # float64 grows to 8.2e-6 there (the kernel's: 2.6e-5), so the gate is the larger of 2e-5 and 8 x the fp32 oracle's error, with
    # the oracle's error itself capped at 2e-5
    big = max(max(f.shape[2:4]) for f in feats) > 16
    ref32 = _map_grads(cfg, grids, feats, g_cond, torch.float32) if big else [None] * len(ref)
    errs, e32s = [], []
    for s_i, (r, r32) in enumerate(zip(ref, ref32)):
        scale = float(r.abs().max())
        assert scale > 0
        errs.append(float((got[s_i].cpu().double() - r).abs().max()) / scale)
        e32s.append(float((r32.double() - r).abs().max()) / scale if big else 0.0)
    print(f"{case}: regime {walk_regime(n, v, len(feats), s, segs)}, error / max|ref| per scale "
          + ", ".join(f"{e:.2e}" for e in errs) + ("; fp32 oracle " + ", ".join(f"{e:.2e}" for e in e32s) if big else ""))
    assert all(e32 < 2e-5 and e < max(GATE, 8 * e32) for e, e32 in zip(errs, e32s)), (errs, e32s)


@pytest.mark.parametrize("knob,value", [("MNERF_CV_BWD_WALK", "0"), ("MNERF_CV_BWD_SEGS", "3")])
def test_cost_volume_backward_knobs(knob, value):
    """The per-sample kernel (MNERF_CV_BWD_WALK=0) and a forced segment count that does not divide S (MNERF_CV_BWD_SEGS=3 at S = 64:
    segments of 21, 21 and 22 samples) on the training shape.  The knobs are read once per process, hence a child process."""
    if knob == "MNERF_CV_BWD_SEGS":
        assert walk_regime(1024, 3, 2, 64, segs=int(value)) == (3, 1)
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(here, "test_ray_chunk_backward_gpu.py"), "-q", "-x", "-s", "-m", "gpu",
                        "-k", "test_cost_volume_backward_matches_float64 and train_shape"],
                       env=dict(os.environ, **{knob: value}), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "1 passed" in r.stdout, f"{knob}={value}:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}"
    print(next((line for line in r.stdout.splitlines() if "train_shape:" in line), ""))


# ----------------------------------------------------------------------------- 2. forward at odd map sizes


def test_cost_volume_forward_at_odd_map_sizes(hip):
    """A 756 x 1008 frame (the IBRNet recipe) gives maps of 95 x 126 and 189 x 252: odd heights, which the matrix form packs in
    row pairs (csrc/cost_volume_mm.hip: nrp = (fh + 1) / 2 + 1).  Contiguous target rows at the top, middle and bottom of the
    frame (the matrix form takes contiguous ranges): matrix form = walk to 5e-6 on the cosines (tests/test_cost_volume_mm.py),
    colours and masks identical; both = the float64 rows to the larger of 2e-5 and 8 x the fp32 oracle's own error on the same
    rows, that error capped at 2e-5 (random maps, texel coordinates up to ~250: the oracle's error is 9.7e-6 ... 1.3e-5 there,
    the kernels' 5.0e-5)."""
    cfg, batch, feats, images = _synthetic(756, 1008, 3, seed=6)
    assert [tuple(f.shape[2:4]) for f in feats] == [(95, 126), (189, 252)]
    cfg.sample_intvs = 32
    h, w = 756, 1008
    v, s = cfg.n_src_views, cfg.sample_intvs
    sum_g = sum(cfg.cos_n_group)
    dc = sum_g + 4 * v
    cs = ((dc + 1 + 7) // 8) * 8
    feats_gpu = [f.cuda() for f in feats]
    img_gpu = images_rgba(images).cuda()
    sc = make_scene_struct(cfg, batch, feats_gpu, img_gpu)
    ranges = [(0, 2 * w), (377 * w + 5, 2 * w), (h * w - 2 * w - 3, 2 * w + 3)]

    def rows(begin, n, mm):
        rays = make_rays_struct(cfg, batch, n, ray_begin=begin)
        with hip.knob("cv_mm", int(mm)):
            return hip.cost_volume(sc, rays, cs).reshape(n, s, cs)

    walks = [rows(b, n, 0) for b, n in ranges]
    keep = hip.cost_volume_operands(sc)  # noqa: F841  (sets sc.feat_op; the tensor must outlive the launches)
    assert sc.feat_op
    mms = [rows(b, n, 1) for b, n in ranges]
    torch.cuda.synchronize()
    pair_feats32 = [(f[:, 0].permute(0, 3, 1, 2), f[:, 1].permute(0, 3, 1, 2)) for f in feats]
    pair_feats = [(f0.double(), f1.double()) for f0, f1 in pair_feats32]
    worst = 0.0
    for (b, n), walk, mm in zip(ranges, walks, mms):
        assert float((mm[..., :sum_g] - walk[..., :sum_g]).abs().max()) < 5e-6
        assert torch.equal(mm[..., sum_g:], walk[..., sum_g:])
        grids, masks, _, _, pts = _grids(cfg, batch, torch.arange(b, b + n), None)
        with torch.no_grad():
            ref, _ = _cond64(cfg, grids, masks, images, pair_feats)
            ref32, _ = O.cost_volume_cond(cfg, pts, *split_poses(batch)[3:], images, pair_feats32, h, w)
        e32 = float((ref32.double() - ref).abs().max())
        assert e32 < 2e-5, e32
        for got in (walk, mm):
            err = float((got[..., :dc].cpu().double() - ref).abs().max())
            worst = max(worst, err)
            assert err < max(GATE, 8 * e32), (b, err, e32)
        assert float((walk[..., dc] - 1).abs().max()) == 0.0
        print(f"odd maps, rays {b}..{b + n}: |cond - float64| walk / matrix form max {worst:.2e}, fp32 oracle {e32:.2e}")


# ----------------------------------------------------------------------------- 4. the whole chunk with stratified samples


def _ray_chunk_gradients(hip, frame, n, overrides, gain, setbg):
    """The comparison of test_render_ray_chunk_gradients_match_float64 (its docstring) on a ``frame`` = (height, width) synthetic
    scene with random maps at 1/8 and 1/4 of it and ``n`` random rays; ``overrides``: dotted options on top of c1_default's;
    ``gain``: factor on the density head's last layer (it ends in a ReLU: sigma scales by exactly that); ``setbg``: white background."""
    from matchnerf_amd import autograd as ag
    from test_model_gpu import build_model
    from helpers import cfg_from_meta
    meta = dict(golden_case("c1_default")[0]["meta"])
    meta["opt_overrides"] = dict(meta["opt_overrides"], **overrides)
    cfg = cfg_from_meta(meta)
    opt, model = build_model(meta)
    assert bool(opt.nerf.wo_render_interval) == cfg.wo_render_interval and bool(opt.nerf.legacy_coord) == cfg.legacy_coord
    dec_m = model.nerf_dec
    s, v = cfg.sample_intvs, cfg.n_src_views
    assert s == 64 and opt.nerf.sample_intvs == 64
    gen = torch.Generator().manual_seed(12)
    with torch.no_grad():  # the goldens' zero biases and unit LayerNorm would hide their own gradients' paths
        for name, p in dec_m.named_parameters():
            if name.endswith("bias") or "layer_norm" in name:
                p.add_(0.1 * torch.randn(p.shape, generator=gen).to(p.device))
        for name, p in dec_m.named_parameters():
            if name.startswith("out_alpha_linear.2."):
                p.mul_(float(gain))
    h, w = frame
    _, batch, feats, images = _synthetic(h, w, 3, seed=5)
    te, ti, tn, se, si, sn = split_poses(batch)
    idx = torch.randperm(h * w, generator=gen)[:n]
    u = torch.rand(n, s, generator=gen)
    g_rgb, g_depth, g_op = torch.randn(n, 3, generator=gen), torch.randn(n, 1, generator=gen), torch.randn(n, 1, generator=gen)

    feats_gpu = [f.cuda().requires_grad_(True) for f in feats]
    img_gpu = images_rgba(images).cuda()
    idx_gpu, u_gpu = idx.cuda(), u.cuda()
    idx32 = idx_gpu.int()
    kinv, c2w = camera.target_ray_consts(te.numpy(), ti.numpy(), cfg.legacy_coord)

    def make_rays():
        r = make_rays_struct(cfg, batch, n, ray_idx_gpu=idx32)
        r.strat_u = u_gpu.data_ptr()
        return r, (idx32, u_gpu)

    dec = dec_m.decoder_struct(s, "cuda", setbg)
    make_scene = lambda fs: make_scene_struct(cfg, batch, [f.detach() for f in fs], img_gpu)  # noqa: E731
    with torch.no_grad():
        dc = sum(cfg.cos_n_group) + 4 * v
        cond_k = hip.cost_volume(make_scene(feats_gpu), make_rays()[0], dec.cond_stride).cpu()[:, :dc].reshape(n, s, dc).double()

    # float64 chain from the forward's rows, 256 rays at a time; a first pass without gradients finds the rays near a ReLU kink
    sd64 = {"nerf_dec." + k: p.detach().double().cpu().requires_grad_(True) for k, p in dec_m.named_parameters()}
    cond_ref = cond_k.clone().requires_grad_(True)
    grids, _, d_all, ray_all, pts_all = _grids(cfg, batch, idx, u)
    x_all = O.project_to_view(pts_all, se[0], si[0], w, h, sn[0, 0], sn[0, 1])
    view0 = hip.make_view(se[0].numpy(), si[0].numpy(), float(sn[0, 0]), float(sn[0, 1]))
    rays_k, keep_k = make_rays()
    _, x_k, d_k = hip.ray_samples(rays_k, view0)
    x_k, d_k = x_k.cpu().reshape(n, s, 3), d_k.cpu().reshape(n, s)
    print(f"sample coordinates: kernel vs oracle max |dx| {float((x_k - x_all).abs().max()):.1e}, "
          f"|dd| {float((d_k - d_all).abs().max()):.1e}")
    x_all, d_all = x_k.double(), d_k
    dir_all = (F.normalize(ray_all, dim=-1) @ se[0][:, :3].t()).double()

    def chain(r):
        rgb_s, sigma = O.decoder(cfg, sd64, x_all[r], dir_all[r], cond_ref[r], cond_ref[r][..., -v:])
        return O.composite(cfg, ray_all[r].double(), rgb_s, sigma, d_all[r].double(), setbg_opaque=setbg)[:3]

    keep = torch.empty(n)
    for r0 in range(0, n, 256):
        with torch.no_grad(), ReluKinks(min(256, n - r0)) as kinks:
            chain(slice(r0, r0 + 256))
        keep[r0:r0 + 256] = (kinks.margin >= 2e-6).float()
    g_rgb, g_depth, g_op = g_rgb * keep[:, None], g_depth * keep[:, None], g_op * keep[:, None]

    launch = ag.RayChunkLaunch(opt, dec_m, make_scene=make_scene, make_rays=make_rays, make_decoder=lambda: dec,
                               view0_extr=se[0].numpy(), kinv=kinv, c2w=c2w, ray_idx=idx_gpu, width=w, n_views=v,
                               setbg_opaque=setbg)
    rgb, depth, opacity = ag.render_ray_chunk(launch, feats_gpu)
    torch.autograd.backward([rgb, depth, opacity], [g_rgb.cuda(), g_depth.cuda(), g_op.cuda()])
    torch.cuda.synchronize()

    outs = []
    for r0 in range(0, n, 256):
        r = slice(r0, r0 + 256)
        out = chain(r)
        sum((o * gg[r].double()).sum() for o, gg in zip(out, (g_rgb, g_depth, g_op))).backward()
        outs.append([o.detach() for o in out])
    ref = [torch.cat([o[k] for o in outs], 0) for k in range(3)]
    assert linf(rgb, ref[0]) < 1e-4 and linf(opacity, ref[2]) < 1e-4 and linf(depth, ref[1]) < 3e-4
    map_ref = _map_grads(cfg, grids, feats, cond_ref.grad.reshape(n * s, dc))

    worst = {}
    for k, p in dec_m.named_parameters():
        r64 = sd64["nerf_dec." + k].grad
        worst[k] = float((p.grad.cpu().double() - r64).abs().max()) / (float(r64.abs().max()) + 1e-30)
    for s_i, (f, r64) in enumerate(zip(feats_gpu, map_ref)):
        worst[f"map{s_i}"] = float((f.grad.cpu().double() - r64).abs().max()) / float(r64.abs().max())
    print(f"rays within 2e-6 of a ReLU kink: {int((keep == 0).sum())} of {n}")
    print({k: f"{e:.1e}" for k, e in worst.items()})
    bad = {k: e for k, e in worst.items() if not e < 2e-4}
    assert len(worst) == 32 + 2 and not bad, bad
    return worst, ref


def test_render_ray_chunk_gradients_match_float64(hip):
    """autograd.render_ray_chunk (HIP forward; backward = composite -> decoder -> cost-volume backward kernels) on a 512 x 640 scene
    (random maps 64 x 80 / 128 x 160), 1 024 random rays, 64 samples with explicit stratified offsets, random upstream gradients of
    rgb, depth and opacity; vs float64 autograd through O.render_rays' chain (O.decoder, O.composite) on the same offsets, fed
    with what the backward kernels themselves start from: the forward kernel's conditioning rows (hip.cost_volume on the same scene
    and rays; judged against float64 by the cost-volume tests above) and sample coordinates / depths (hip.ray_samples, the bits
    the backward re-evaluates the decoder at).  The maps' reference gradient is the float64 cost-volume backward (``_map_grads``)
    of the float64 gradient of those rows.
    Why: with the oracle's own fp32 coordinates (here up to 2.4e-7 from the kernel's, depths identical) the legacy positional
    encoding's 2^9 frequency turns that into 1.2e-4 rad, enough to move ReLU arguments across their kinks all through the
    network: the gradients then land 1e-3 ... 9e-3 from float64, in the layers in front of a ReLU, with every kernel right.
    Rays within 2e-6 of a ReLU kink of the float64 chain get zero upstream gradient (gpu_helpers.ReluKinks), as in
    test_decoder_backward.py's training shapes.  Gates: the forward at tests/test_hip_kernels.py's rendered gates; every decoder
    tensor at test_decoder_backward.py's 2e-4 of its largest float64 magnitude; the map gradients at the same 2e-4 per scale
    (observed: 6e-6 and 2.2e-5)."""
    _ray_chunk_gradients(hip, (512, 640), 1024, {}, 1, False)


def test_render_ray_chunk_gradients_match_float64_with_intervals(hip):
    """The same comparison where nothing else reaches the interval form of the compositing backward: a 64 x 80 frame (random maps
    8 x 10 / 16 x 20), 128 rays, 64 samples, nerf.wo_render_interval = false (the last interval is 1e10), pixel-centre coordinates,
    the density head x 64 (rays that hit a surface next to empty ones), white background.  Same gates.  A residue of the suffix sum on
    a ray's last sample is multiplied by 1e10 |ray| and lands in the density head's gradients (out_alpha_linear.*) and in everything
    in front of it.  Measured on MI355X: every tensor <= 3.5e-06 of its largest float64 magnitude, maps 2.3e-06 / 2.4e-06; with the
    suffix formed as "total - prefix" the same figures were 2.7e+04 ... 5.3e+04 (colour branch: 8.6e-07) and 6.6e+03 / 3.7e+04."""
    worst, ref = _ray_chunk_gradients(hip, (64, 80), 128, {"nerf.wo_render_interval": False, "nerf.legacy_coord": False}, 64, True)
    opacity = ref[2].reshape(-1)
    assert int((opacity > 1 - 1e-6).sum()) > 0
