"""The fused tail of a training iteration on the GPU (csrc/optim.hip through optim.FusedAdamW and autograd.l2_loss) against
float64 on the CPU, with torch's own fp32 path on the GPU as the measure of what fp32 can do.

Gate (per tensor):  max|x_fused - x64| <= 2 * max|x_torch32 - x64| + 2^-23 * max|x64|
- x_torch32: torch's foreach AdamW + clip_grad_norm_ (or its ((a - b) ** 2).mean()) in fp32 on the GPU from the same start;
- the factor 2 covers a different but equally rounded association of the same fp32 chain, the last term one unit in the
  last place of the largest element."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 5, 127, 128 * 128 + 1, 9 * 128 * 128)
LRS = (1e-3, 7e-4, 2e-3, 5e-4, 1.3e-3)


def gate_ok(name, fused, t32, x64, worst):
    x64 = x64.detach().double().cpu().reshape(-1)
    e_f = float((fused.detach().double().cpu().reshape(-1) - x64).abs().max())
    e_t = float((t32.detach().double().cpu().reshape(-1) - x64).abs().max())
    bound = 2 * e_t + 2.0 ** -23 * float(x64.abs().max())
    ratio = e_f / bound if bound > 0 else (0.0 if e_f == 0 else float("inf"))
    worst[name.split("[")[0]] = max(worst.get(name.split("[")[0], 0.0), ratio)
    print(f"  {name}: fused err {e_f:.3e}  torch32 err {e_t:.3e}  bound {bound:.3e}  ratio {ratio:.3f}")
    return e_f <= bound


def make_params(device, dtype, seed=0):
    """the tensors of the test on `device`: one of them a view at an odd storage offset, the last one never gets a gradient"""
    g = torch.Generator().manual_seed(seed)
    vals = [torch.randn(n, generator=g) * 0.1 for n in SIZES] + [torch.randn(33, generator=g)]
    ps = []
    for i, v in enumerate(vals):
        if i == 3:  # 127 elements starting at element 1 of a larger buffer: 4-byte aligned only
            base = torch.zeros(v.numel() + 8, device=device, dtype=dtype)
            t = base[1:1 + v.numel()]
            t.copy_(v.to(dtype))
            assert t.data_ptr() % 16 == 4 or device == "cpu"
            ps.append(t.requires_grad_())
        else:
            ps.append(v.to(device=device, dtype=dtype).requires_grad_())
    return ps


def make_grads(step, scale, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + step + 1)
    return [torch.randn(n, generator=g) * scale for n in SIZES]


def groups_of(ps):
    return [dict(params=[ps[0], ps[2], ps[3], ps[5]], lr=1e-3, weight_decay=1e-2),
            dict(params=[ps[1], ps[4], ps[6]], lr=5e-3, weight_decay=1e-4)]


def run_steps(kind, scale, max_norm, n_steps=5, state=None, lrs=LRS):
    """kind: 'fused' (GPU), 'torch32' (GPU, foreach + clip_grad_norm_), 'torch64' (CPU).  -> (params, optimizer, norms)"""
    from matchnerf_amd.optim import FusedAdamW
    device, dtype = ("cpu", torch.float64) if kind == "torch64" else ("cuda", torch.float32)
    ps = make_params(device, dtype)
    if kind == "fused":
        opt = FusedAdamW(groups_of(ps), betas=(0.9, 0.999), eps=1e-8)
    else:
        opt = torch.optim.AdamW(groups_of(ps), betas=(0.9, 0.999), eps=1e-8, foreach=(kind == "torch32"))
    if state is not None:
        with torch.no_grad():
            for p, v in zip(ps, state["params"]):
                p.copy_(v.to(device=device, dtype=dtype))
        sd = copy.deepcopy(state["optim"])
        opt.load_state_dict(sd)  # casts the state to the parameters' dtype and device
    if kind == "fused":
        opt.param_groups[0]["max_norm"] = max_norm  # after load_state_dict: torch's groups do not carry the key
    norms = []
    for i in range(n_steps):
        for k, gr in enumerate(opt.param_groups):
            gr["lr"] = lrs[i] * (1 if k == 0 else 5)
        opt.zero_grad(set_to_none=True)
        for p, g in zip(ps[:-1], make_grads(i, scale)):
            p.grad = g.to(device=device, dtype=dtype)
        if kind == "fused":
            opt.step()
            norms.append(opt.last_sumsq[0].sqrt())
        else:
            norms.append(torch.nn.utils.clip_grad_norm_(opt.param_groups[0]["params"], max_norm))
            opt.step()
    return ps, opt, norms


def compare_runs(f, t, d, worst):
    (pf, of, nf), (pt, ot, nt), (pd, od, nd) = f, t, d
    ok = True
    for i in range(len(SIZES)):
        ok &= gate_ok(f"param[{i}]", pf[i], pt[i], pd[i], worst)
        for k in ("exp_avg", "exp_avg_sq"):
            ok &= gate_ok(f"{k}[{i}]", of.state[pf[i]][k], ot.state[pt[i]][k], od.state[pd[i]][k], worst)
        ok &= gate_ok(f"grad[{i}]", pf[i].grad, pt[i].grad, pd[i].grad, worst)
        assert float(of.state[pf[i]]["step"]) == float(od.state[pd[i]]["step"])
    for a, b, c in zip(nf, nt, nd):
        ok &= gate_ok("norm", a, b, c, worst)
    return ok


@pytest.mark.parametrize("scale,clips", [(1e-2, True), (1e-6, False)])
def test_fused_step_matches_float64_as_well_as_torch_fp32(scale, clips):
    """Five steps, a different lr each, group 0 clipped at max_norm 1 (scale 1e-2: its norm is about 4, the gradients are scaled;
    scale 1e-6: the norm is far below max_norm, nothing is scaled), group 1 never.

    The test prints, per tensor, both errors, the bound and the ratio fused error / bound (1 = at the gate), and the worst ratio
    per quantity.  Measured on MI355X, worst ratio over all tensors:
      clipped:    param 0.39, exp_avg 0.40, exp_avg_sq 0.67, grad 0.29, norm 0.29
      unclipped:  param 0.40, exp_avg 0.29, exp_avg_sq 0.38, grad 0.00, norm 0.17
    (the chain's operations and roundings are torch's; what differs is the summation order of the norm)."""
    max_norm = 1.0
    worst = {}
    f = run_steps("fused", scale, max_norm)
    t = run_steps("torch32", scale, max_norm)
    d = run_steps("torch64", scale, max_norm)
    assert (float(d[2][0]) > max_norm) == clips
    ok = compare_runs(f, t, d, worst)
    print("worst ratios:", {k: round(v, 3) for k, v in worst.items()})
    assert ok, worst
    # clipped group: .grad holds the clipped values; unclipped tensors keep their gradient bit for bit
    g0 = make_grads(4, scale)
    assert torch.equal(f[0][1].grad.cpu(), g0[1]) and torch.equal(f[0][4].grad.cpu(), g0[4])
    if clips:
        assert not torch.equal(f[0][5].grad.cpu(), g0[5])
    else:
        assert torch.equal(f[0][5].grad.cpu(), g0[5])
    # the parameter without a gradient and its state are untouched
    lone = f[0][-1]
    assert torch.equal(lone.detach().cpu(), make_params("cpu", torch.float32)[-1].detach()) and lone not in f[1].state


def test_fused_step_is_bit_reproducible():
    a = run_steps("fused", 1e-2, 1.0)
    b = run_steps("fused", 1e-2, 1.0)
    for pa, pb in zip(a[0][:-1], b[0][:-1]):
        assert torch.equal(pa, pb) and torch.equal(pa.grad, pb.grad)
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(a[1].state[pa][k], b[1].state[pb][k])
    for na, nb in zip(a[2], b[2]):
        assert torch.equal(na, nb)


@pytest.mark.parametrize("first", ["fused", "torch32"])
def test_state_dict_moves_between_fused_and_torch(first):
    """Two steps with one implementation, its state_dict() loaded into the other over clones of the parameters; the third step
    of both (and of float64 from the same state) agrees under the gate of the first test."""
    second = "torch32" if first == "fused" else "fused"
    ps, opt, _ = run_steps(first, 1e-2, 1.0, n_steps=2)
    sd = opt.state_dict()
    assert all(set(s) == {"step", "exp_avg", "exp_avg_sq"} for s in sd["state"].values())
    state = dict(params=[p.detach().clone() for p in ps], optim=sd)
    third = LRS[2:3]
    runs = {kind: run_steps(kind, 1e-2, 1.0, n_steps=1, state=state, lrs=third) for kind in (first, second, "torch64")}
    for kind in (first, second):
        assert all(float(runs[kind][1].state[p]["step"]) == 3.0 for p in runs[kind][0][:-1])
    worst = {}
    assert compare_runs(runs["fused"], runs["torch32"], runs["torch64"], worst), worst


def test_version_bump_makes_the_next_forward_use_the_new_weights():
    """The kernels write through raw pointers; every weight-stream cache of the model is keyed on Parameter._version."""
    from matchnerf_amd import options, synthetic as syn
    from matchnerf_amd.edict import EasyDict
    from matchnerf_amd.models import models_dict
    from matchnerf_amd.optim import FusedAdamW

    def build():
        opt = options.load_options("configs/test.yaml", verbose=False)
        opt.device = "cuda"
        opt.nerf.sample_intvs = 32
        return models_dict[opt.model](opt).to("cuda").eval()

    model = build()
    model.load_state_dict(syn.to_torch(syn.seeded_state_dict(syn.state_dict_spec(), 1), "cuda"))
    scene = syn.make_scene(32, 32, 3, seed=4)
    batch = lambda: EasyDict({k: torch.from_numpy(v).cuda() for k, v in scene.items()})  # noqa: E731
    with torch.no_grad():
        before = model(batch(), mode="test").rgb.clone()
    versions = [p._version for p in model.parameters()]
    opt = FusedAdamW([dict(params=model.feat_enc.parameters(), lr=1e-3, max_norm=1.0), dict(params=model.nerf_dec.parameters(), lr=1e-2)])
    g = torch.Generator().manual_seed(0)
    for p in model.parameters():
        p.grad = (torch.randn(p.shape, generator=g) * 1e-2).cuda()
    opt.step()
    assert all(p._version > v for p, v in zip(model.parameters(), versions))
    with torch.no_grad():
        after = model(batch(), mode="test").rgb.clone()
    fresh = build()
    fresh.load_state_dict(model.state_dict())
    with torch.no_grad():
        want = fresh(batch(), mode="test").rgb
    assert torch.equal(after, want)
    assert not torch.equal(after, before) and float((after - before).abs().max()) > 1e-4


@pytest.mark.parametrize("shape", [(1, 1024, 3), (1, 96, 3), (7,), (4096, 3), (1, 1)])
def test_fused_l2_loss_value_gradient_and_reproducibility(shape):
    """Value and gradient against the float64 expression, torch's fp32 ((a - b) ** 2).mean() as the fp32 yardstick; two calls give the
    same bits.  Measured on MI355X, worst ratio error / bound over the shapes: value 0.31,
    gradient 0.25 (the fused errors equal torch's on four of the five shapes)."""
    from matchnerf_amd.autograd import l2_loss
    g = torch.Generator().manual_seed(sum(shape))
    a, b = torch.rand(shape, generator=g), torch.rand(shape, generator=g)
    a64 = a.double().requires_grad_()
    l64 = ((a64 - b.double()) ** 2).mean()
    l64.backward()
    at = a.cuda().requires_grad_()
    lt = ((at - b.cuda()) ** 2).mean()
    lt.backward()
    af = a.cuda().requires_grad_()
    lf = l2_loss(af, b.cuda())
    lf.backward()
    worst = {}
    ok = gate_ok("value", lf, lt, l64, worst)
    ok &= gate_ok("gradient", af.grad, at.grad, a64.grad, worst)
    assert ok, worst
    af2 = a.cuda().requires_grad_()
    lf2 = l2_loss(af2, b.cuda())
    (3.0 * lf2).backward()
    assert torch.equal(lf, lf2)
    assert torch.allclose(af2.grad, 3 * af.grad, rtol=1e-6, atol=0)
    af3 = a.cuda().requires_grad_()
    l2_loss(af3, b.cuda()).backward()
    assert torch.equal(af3.grad, af.grad)


def test_fused_l2_loss_refuses_cpu_tensors():
    from matchnerf_amd import hip
    from matchnerf_amd.autograd import l2_loss
    with pytest.raises(hip.MnerfError):
        l2_loss(torch.rand(4, 3, requires_grad=True), torch.rand(4, 3))
