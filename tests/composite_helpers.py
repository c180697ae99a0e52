"""Inputs and float64 references for the compositing tests (test_composite_cpu.py, test_composite_gpu.py, and the strengthened
backward test of test_hip_kernels.py).

The quadrature (oracle: O.composite):
    sd_j = sigma_j * k_j,  k_j = 1 (wo_render_interval) or (d_{j+1} - d_j) * |ray|, the last interval 1e10
    T_j = exp(-sum_{i<j} sd_i),  w_j = T_j (1 - exp(-sd_j))
    rgb = sum w_j c_j (+ 1 - opacity with a white background), depth = sum w_j d_j, opacity = sum w_j, prob_j = w_j

Density profiles (``profiles``): the name says which regime of the quadrature a case is in; the rules are written once, here.
    fog         rand * 0.3 on a random half of the samples, 0 on the rest (what the older tests draw)
    wall        fog plus one sample per ray, at a random position, of magnitude 10^U(-0.5, 5.5)
    wall_first  fog with sample 0 = 50 (``wall_first_value``)
    wall_last   fog / 100 with the last sample = 1e4
    slab        fog with five consecutive samples (fewer where S < 5) of 3.0 (``slab_value``) at a random position
    all_huge    1e30 everywhere (finite in float32; with intervals the last sample's sd overflows to +inf, whose exp is 0)
    zero        0 everywhere
    tiny        1e-30 everywhere (1 - exp(-sd) rounds to 0)
    block_edge  only for S > 64: fog with sample 63 = 0.7 and sample 64 = 200: the carry between 64-lane blocks next to a wall

Transmittance "exactly 0 in float32": exp(-x) is below half the smallest float32 denormal from x = 103.98 on.  The tests take the
samples whose float64 prefix sum exceeds ``T_ZERO`` = 110: a float32 prefix sum is within 1e-5 of it, so every float32 evaluation
of T, on the host or on the device, flushed or not, gives 0 there.
"""
import functools

import torch

SAMPLE_COUNTS = (1, 2, 33, 64, 65, 100, 128, 200, 256)
BACKWARD_SAMPLE_COUNTS = (1, 33, 64, 65, 128, 200)
# (wo_render_interval, setbg_opaque)
MODES = ((True, False), (True, True), (False, False), (False, True))
N_RAYS = 67  # not a multiple of the 4 waves of a workgroup

# forward gates: those of test_hip_kernels.py::test_composite_matches_oracle
GATE_RGB, GATE_OPACITY, GATE_DEPTH, GATE_PROB = 2e-6, 2e-6, 1e-5, 2e-6
# backward gates, in that file's form: gate * max(1, max |reference|)
GATE_G_RGB, GATE_G_SD = 2e-6, 2e-5
T_ZERO = 110.0


def profiles(r, S, generator, wall_first_value=50.0, slab_value=3.0):
    """-> {name: sigma [r, S] float32}, in a fixed order"""
    g = generator

    def fog():
        return torch.rand(r, S, generator=g) * 0.3 * (torch.rand(r, S, generator=g) > 0.5)

    rows = torch.arange(r)
    out = {"fog": fog()}
    wall = fog()
    wall[rows, torch.randint(0, S, (r,), generator=g)] += 10.0 ** (torch.rand(r, generator=g) * 6.0 - 0.5)
    out["wall"] = wall
    first = fog()
    first[:, 0] = wall_first_value
    out["wall_first"] = first
    last = fog() / 100.0
    last[:, -1] = 1e4
    out["wall_last"] = last
    slab = fog()
    n_slab = min(5, S)
    start = torch.randint(0, S - n_slab + 1, (r,), generator=g)
    for i in range(n_slab):
        slab[rows, start + i] = slab_value
    out["slab"] = slab
    out["all_huge"] = torch.full((r, S), 1e30)
    out["zero"] = torch.zeros(r, S)
    out["tiny"] = torch.full((r, S), 1e-30)
    if S > 64:
        edge = fog()
        edge[:, 63], edge[:, 64] = 0.7, 200.0
        out["block_edge"] = edge
    return out


@functools.lru_cache(maxsize=None)
def case_inputs(S, r=N_RAYS, wall_first_value=50.0, slab_value=3.0):
    """Everything but the mode, seeded from the case's parameters; float32 CPU tensors, shared between tests (do not modify):
    sigma {profile: [r,S]}, rgb_s [r,S,3] in [0,1], depth [r,S] sorted in [2,4], ray [r,3], ray_len [r] (float32 norm, what the
    kernels are handed), upstream gradients g_rgb [r,3], g_depth [r], g_opacity [r]"""
    g = torch.Generator().manual_seed(100003 * S + r)
    inp = {"sigma": profiles(r, S, g, wall_first_value, slab_value),
           "rgb_s": torch.rand(r, S, 3, generator=g)}
    while True:  # no two equal depths on a ray: the normalised density gradient divides by the interval
        inp["depth"] = torch.sort(torch.rand(r, S, generator=g) * 2 + 2, dim=1).values
        if bool((inp["depth"][:, 1:] > inp["depth"][:, :-1]).all()):
            break
    inp["ray"] = torch.randn(r, 3, generator=g)
    inp["ray_len"] = inp["ray"].norm(dim=-1).contiguous()
    inp["g_rgb"], inp["g_depth"], inp["g_opacity"] = (torch.randn(r, 3, generator=g), torch.randn(r, generator=g),
                                                     torch.randn(r, generator=g))
    return inp


def interval_scale64(depth, ray_len, wo_interval):
    """k_j [R,S] in float64 from float32 (or float64) depths and ray lengths"""
    d = depth.double()
    if wo_interval:
        return torch.ones_like(d)
    intv = torch.cat([d[:, 1:] - d[:, :-1], torch.full_like(d[:, :1], 1e10)], 1)
    return intv * ray_len.double()[:, None]


def prefix64(sigma, depth, ray_len, wo_interval):
    """float64 exclusive prefix sum of sd [R,S]: T = exp(-prefix)"""
    sd = sigma.double() * interval_scale64(depth, ray_len, wo_interval)
    return torch.cat([torch.zeros_like(sd[:, :1]), sd[:, :-1]], 1).cumsum(1)


def composite64(rgb_s, sigma, depth, ray_len, wo_interval, setbg):
    """The quadrature in float64 (inputs of any float type; differentiable in rgb_s and sigma)
    -> rgb [R,3], depth [R], opacity [R], prob [R,S]"""
    sd = sigma.double() * interval_scale64(depth, ray_len, wo_interval)
    alpha = -torch.expm1(-sd)
    excl = torch.cat([torch.zeros_like(sd[:, :1]), sd[:, :-1]], 1).cumsum(1)
    w = torch.exp(-excl) * alpha
    rgb = (rgb_s.double() * w[..., None]).sum(1)
    opacity = w.sum(1)
    if setbg:
        rgb = rgb + (1 - opacity)[:, None]
    return rgb, (depth.double() * w).sum(1), opacity, w


def gradients64(inp, sigma, wo_interval, setbg):
    """float64 autograd through composite64 for the case's upstream gradients
    -> g_rgb_s [R,S,3], dL/dsd [R,S] (= g_sigma / k: the normalised density gradient), k [R,S]"""
    rgb_s = inp["rgb_s"].double().requires_grad_(True)
    sig = sigma.double().requires_grad_(True)
    rgb, depth, opacity, _ = composite64(rgb_s, sig, inp["depth"], inp["ray_len"], wo_interval, setbg)
    ((rgb * inp["g_rgb"].double()).sum() + (depth * inp["g_depth"].double()).sum()
     + (opacity * inp["g_opacity"].double()).sum()).backward()
    k = interval_scale64(inp["depth"], inp["ray_len"], wo_interval)
    assert bool((k > 0).all())
    return rgb_s.grad, sig.grad / k, k


def forward_errors(out, ref):
    """out: (rgb [R,3], depth [R] or [R,1], opacity [R] or [R,1], prob [R,S] or [R,S,1] or None) of any float type on any device;
    ref: composite64's tuple -> {"rgb", "depth", "opacity", "prob", "prob_sum"}: worst absolute error; raises on NaN / inf"""
    r = ref[0].shape[0]
    got = [None if t is None else t.detach().cpu().double() for t in out]
    for t in got:
        assert t is None or bool(torch.isfinite(t).all()), "NaN or inf in a composited output"
    err = {"rgb": float((got[0] - ref[0]).abs().max()), "depth": float((got[1].reshape(r) - ref[1]).abs().max()),
           "opacity": float((got[2].reshape(r) - ref[2]).abs().max())}
    if len(got) > 3 and got[3] is not None:
        prob = got[3].reshape(r, -1)
        err["prob"] = float((prob - ref[3]).abs().max())
        err["prob_sum"] = float((prob.sum(1) - got[2].reshape(r)).abs().max())
    return err


FORWARD_GATES = {"rgb": GATE_RGB, "depth": GATE_DEPTH, "opacity": GATE_OPACITY, "prob": GATE_PROB, "prob_sum": GATE_PROB}


def check_forward(err, what, fraction=1.0):
    for key, e in err.items():
        assert e < fraction * FORWARD_GATES[key], f"{what}: {key} error {e:.2e} >= {fraction * FORWARD_GATES[key]:.1e}"


def backward_errors(g_rgb_s, g_sigma, ref):
    """g_rgb_s [R,S,3], g_sigma [R,S] of any float type on any device; ref: gradients64's tuple
    -> (error of g_rgb_s, its gate, error of the normalised density gradient g_sigma / k, its gate), every column included"""
    ref_rgb, ref_sd, k = ref
    a, b = g_rgb_s.detach().cpu().double(), g_sigma.detach().cpu().double()
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()), "NaN or inf in a gradient"
    return (float((a - ref_rgb).abs().max()), GATE_G_RGB * max(1.0, float(ref_rgb.abs().max())),
            float((b / k - ref_sd).abs().max()), GATE_G_SD * max(1.0, float(ref_sd.abs().max())))
