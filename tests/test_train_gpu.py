"""Stand-alone training on the GPU: Coach.train_iteration against three optimizer steps of the reference model
(tests/golden/train_steps.npz, tools/gen_train_golden.py), a loss that falls on both optimizer paths, and train.py / test.py end
to end as child processes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden
from matchnerf_amd import options, synthetic as syn
from matchnerf_amd.coach import Coach
from matchnerf_amd.edict import EasyDict

pytestmark = pytest.mark.gpu


class StubLoader:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def make_coach(tmp_path, monkeypatch, name, fused, extra, n_train):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("MNERF_FUSED_OPTIM", "1" if fused else "0")
    cmd = options.parse_arguments(["--yaml=train", f"--name={name}", "--tb=false", f"--output_root={tmp_path}"] + list(extra))
    opt = options.set(cmd, verbose=False)
    c = Coach(opt)
    c.build_networks()
    c.model.load_state_dict(syn.to_torch(syn.seeded_state_dict(syn.state_dict_spec(n_src_views=3), 1), opt.device))
    c.train_loader = StubLoader(n_train)
    c.setup_optimizer()
    assert c.fused_optim == fused
    c.it, c.ep = 0, 0
    c.model.train()
    return c


def scene_batch(device, **kw):
    return EasyDict({k: torch.from_numpy(v).to(device) for k, v in syn.make_scene(**kw).items()})


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "torch"])
def test_three_iterations_follow_the_reference(tmp_path, monkeypatch, fused):
    """Three Coach.train_iteration's on the golden's scene, weights and ray lists (stratified sampling off) against the reference's
    own three steps in float64:
    - the lr pairs are equal;
    - each loss within 10 x the reference's own fp32-vs-float64 spread of that loss (floor 1e-6 relative);
    - per probe, q = (p3 - p0) / sum(lr):  |q - q_ref64| <= 3 * 1e-3 + the reference's own fp32-vs-float64 spread of q on that probe,
      over the elements whose float64 gradient exceeds 1e-5 at all three steps (at most 20 % of the probed elements left out).
      1e-3 is the gradient gate of test_train_mode_gradients_match_oracle_autograd, 3 the number of steps.
    Every figure is printed before anything is asserted.
    The probes are NOT typical elements: of each candidate parameter the generator keeps the 256-element slice on which the
    reference's own fp32 and float64 runs agree best and drops candidates whose best slice still differs by more than 3e-3
    (tools/gen_train_golden.py), so the gate covers well-conditioned elements; 11 probes are decoder tensors, 4 encoder tensors.

    Measured on MI355X (profiles/current/train_tests_gpu.log), fused / torch path: loss |diff| 1.3e-7, 9.6e-7, 8.7e-7 / 1.5e-7,
    9.9e-7, 8.9e-7 against bounds 1.3e-6, 9.4e-6, 1.25e-5; worst probe max|q - q64| 1.10e-3 (backbone.conv2, bound 4.3e-3) /
    1.21e-3 (layers.3 merge, bound 4.3e-3), every other probe below 8.3e-4; excluded share 0.069."""
    g = load_golden("train_steps")
    meta = g["meta"]
    c = make_coach(tmp_path, monkeypatch, "golden", fused,
                   [f"--nerf.sample_intvs={meta['n_samples']}", f"--nerf.rand_rays_train={meta['n_rays']}", "--nerf.sample_stratified=false",
                    f"--max_epoch={meta['max_epoch']}"], meta["steps_per_epoch"])
    named = dict(c.model.named_parameters())
    probes = meta["probes"]
    for i, name in enumerate(probes):  # same start as the reference
        a = int(g[f"probe{i}_start"])
        got = named[name].detach().reshape(-1)[a:a + g[f"probe{i}_p0"].size].cpu().numpy()
        assert np.array_equal(got, g[f"probe{i}_p0_f32"]), name
    rays = torch.from_numpy(g["ray_idx"]).to(c.opts.device)
    randperm = torch.randperm
    losses, lrs = [], []
    for step in range(3):
        lrs.append([gr["lr"] for gr in c.optim.param_groups])
        monkeypatch.setattr(torch, "randperm", lambda n, *a, **k: rays[step].clone())  # the model draws torch.randperm(H * W)[:n]
        var = scene_batch(c.opts.device, **meta["scene"])
        loss = c.train_iteration(var)
        monkeypatch.setattr(torch, "randperm", randperm)
        assert torch.equal(var.ray_idx, rays[step])
        c.sched.step()
        losses.append(float(loss.all.detach()))
    torch.cuda.synchronize()

    ok = True
    print("lr pairs:", lrs, "reference:", g["lrs"].tolist())
    lr_ok = lrs == g["lrs"].tolist()
    for step in range(3):
        spread = abs(g["loss32"][step] - g["loss64"][step])
        bound = max(10 * spread, 1e-6 * abs(g["loss64"][step]))
        err = abs(losses[step] - g["loss64"][step])
        print(f"loss step {step}: {losses[step]:.8f}  ref64 {g['loss64'][step]:.8f}  |diff| {err:.2e}  bound {bound:.2e}"
              f"  {'ok' if err <= bound else 'MISS'}")
        ok &= err <= bound
    kept = total = 0
    for i, name in enumerate(probes):
        a = int(g[f"probe{i}_start"])
        n = g[f"probe{i}_p0"].size
        s = g["lrs"][:, 0 if name.startswith("feat_enc.") else 1].sum()
        p3 = named[name].detach().reshape(-1)[a:a + n].double().cpu().numpy()
        q = (p3 - g[f"probe{i}_p0"]) / s
        q64 = (g[f"probe{i}_p3_f64"] - g[f"probe{i}_p0"]) / s
        keep = (np.abs(g[f"probe{i}_grad_f64"]) > meta["g_min"]).all(0)
        kept, total = kept + int(keep.sum()), total + n
        err = float(np.abs(q - q64)[keep].max())
        bound = 3 * 1e-3 + float(g[f"probe{i}_q_spread"])
        print(f"probe {name}[{a}:{a + n}]: max|q - q64| {err:.2e}  bound {bound:.2e} (ref spread {float(g[f'probe{i}_q_spread']):.2e})"
              f"  {'ok' if err <= bound else 'MISS'}")
        ok &= err <= bound
    excluded = 1 - kept / total
    print(f"excluded share {excluded:.3f} (cap {meta['max_excluded']})")
    assert lr_ok
    assert excluded <= meta["max_excluded"]
    assert ok


N_ITERS = 30  # chosen on the GPU: torch's path falls from 0.0666 (mean of the first five) to 0.0196 (last five), the fused path alike


def test_training_lowers_the_loss_on_both_paths(tmp_path, monkeypatch):
    """One synthetic 64x64 scene over and over, encoder and decoder at train.yaml's rates, no scheduler: the mean loss of the last
    five iterations is below that of the first five, on torch's AdamW + clip_grad_norm_ and on the fused path; and the first
    iteration's loss (same weights, rays and stratified offsets) agrees between the paths as well as fp32 allows:
    |l_fused - l64| <= 2 |l_torch - l64| + 2^-23 |l64| with l64 the float64 expression on the fused run's own prediction."""
    extra = ["--nerf.sample_intvs=32", "--nerf.rand_rays_train=256", "--optim.sched="]
    runs = {}
    for fused in (False, True):
        c = make_coach(tmp_path, monkeypatch, f"falls{int(fused)}", fused, extra, 1)
        assert c.sched is None and [g["lr"] for g in c.optim.param_groups] == [c.opts.optim.lr_enc, c.opts.optim.lr_dec]
        first = {}
        if fused:
            inner = c.compute_loss

            def spy(pred, src, mode=None):
                if not first:
                    gt = src.images[:, -1].reshape(1, 3, -1).permute(0, 2, 1)[:, pred.ray_idx]
                    first["l64"] = float(((pred.rgb.detach().double() - gt.double()) ** 2).mean())
                return inner(pred, src, mode=mode)

            c.compute_loss = spy
        torch.manual_seed(0)
        losses = []
        for _ in range(N_ITERS):
            losses.append(c.train_iteration(scene_batch(c.opts.device, height=64, width=64, n_src_views=3, seed=11)).all.detach())
        losses = [float(x) for x in losses]
        print(("fused" if fused else "torch"), "first five", np.mean(losses[:5]), "last five", np.mean(losses[-5:]))
        runs[fused] = (losses, first.get("l64"))
    for fused in (False, True):
        losses = runs[fused][0]
        assert np.isfinite(losses).all() and np.mean(losses[-5:]) < np.mean(losses[:5]), (fused, losses)
    l_t, l_f, l64 = runs[False][0][0], runs[True][0][0], runs[True][1]
    print(f"first loss: fused {l_f:.9f} torch {l_t:.9f} float64 {l64:.9f}")
    assert abs(l_f - l64) <= 2 * abs(l_t - l64) + 2.0 ** -23 * abs(l64)


def _run(args, cwd, limit=600):
    """a fresh child process under its own time limit"""
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable] + args, cwd=cwd, capture_output=True, text=True)
    print(r.stdout[-3000:], r.stderr[-3000:])
    return r


def test_train_py_end_to_end_then_resume_then_test_py(tmp_path):
    common = ["--data_test.llff=", "--data_test.blender=", "--data_test.dtu.img_wh=64,64", "--data_test.dtu.max_len=1",
              "--nerf.sample_intvs=16", "--nerf.rand_rays_test=4096", f"--output_root={tmp_path}"]
    train = [os.path.join(REPO, "train.py"), "--yaml=train", "--name=e2e", "--tb=false", "--data_train.img_wh=64,64", "--data_train.max_len=4",
             "--data_val.img_wh=64,64", "--data_val.max_len=1", "--nerf.rand_rays_train=96", "--nerf.rand_rays_val=4096",
             "--max_epoch=1", "--freq.ckpt_ep=1", "--freq.val_it=0.5", "--freq.scalar=1"] + common
    r = _run(train, tmp_path)
    assert r.returncode == 0
    out = os.path.join(tmp_path, "e2e")
    latest = os.path.join(out, "models", "latest.pth")
    ck = torch.load(latest, map_location="cpu", weights_only=False)
    assert set(ck) == {"model", "optim", "sched", "epoch", "iter"} and (ck["epoch"], ck["iter"]) == (1, 4)
    assert os.path.isfile(os.path.join(out, "models", "ep1_it4.pth"))
    rows = [json.loads(l) for l in open(os.path.join(out, "scalars.jsonl"))]
    assert sum(r_["split"] == "train" and r_["tag"] == "loss_render" for r_ in rows) == 4
    psnr = [r_["value"] for r_ in rows if r_["split"] == "val" and r_["tag"] == "PSNR"]
    assert len(psnr) >= 1 and all(np.isfinite(v) and 0 < v < 60 for v in psnr)
    assert "training done: 4 iterations" in r.stdout

    r = _run(train + ["--resume=true"], tmp_path)
    assert r.returncode == 0
    assert "resuming from epoch 1 (iteration 4)" in r.stdout and "training done: 4 iterations" in r.stdout
    assert len(open(os.path.join(out, "scalars.jsonl")).readlines()) == len(rows)  # nothing left to train

    r = _run([os.path.join(REPO, "test.py"), "--yaml=test", "--name=e2e_test", f"--load={latest}", "--data_test.tnt="] + common, tmp_path)
    assert r.returncode == 0
    assert "not found" not in r.stdout and "mean PSNR" in r.stdout
    assert os.path.isfile(os.path.join(tmp_path, "e2e_test", "test", "0results_dtu.txt"))


def test_training_convolutions_fall_back_per_convolution_and_drop_their_packs():
    """autograd.conv2d: a convolution the kernels do not build, or the stem asked for the gradient of the images, runs as torch's
    op (it used to raise inside backward); the split-fp16 packs live for one forward of their owner only, and a pack made from
    other weights is not used."""
    from matchnerf_amd import autograd as AG
    from matchnerf_amd.gmflow import CNNEncoder
    torch.manual_seed(0)
    odd = torch.nn.Conv2d(16, 32, 3, padding=1).cuda()
    assert not AG.conv2d_supported(odd)
    x = torch.randn(2, 16, 24, 24, device="cuda", requires_grad=True)
    y = AG.conv2d(odd, x)
    assert torch.equal(y, odd(x))
    y.sum().backward()
    assert x.grad is not None and odd.weight.grad is not None

    net = CNNEncoder().cuda().train()
    img = torch.rand(2, 3, 64, 64, device="cuda", requires_grad=True)
    out = net(img)
    convs = [m for m in net.modules() if isinstance(m, torch.nn.Conv2d)]
    assert all(getattr(c, "_mnerf_train_pack", None) is None for c in convs)  # dropped at the end of the owner's forward
    out.square().mean().backward()  # the stem's data gradient: torch's op, everything else on the HIP nodes
    assert img.grad is not None and torch.isfinite(img.grad).all() and float(img.grad.abs().max()) > 0
    assert all(c.weight.grad is not None and torch.isfinite(c.weight.grad).all() for c in convs)

    # a stale pack (made before the weight changed) is ignored: the result is that of the live weight
    c = net.layer1[0].conv1
    xin = torch.randn(2, 64, 16, 16, device="cuda")
    with torch.enable_grad():
        want = AG.conv2d(c, xin.clone().requires_grad_())
        c._mnerf_train_pack = (None, None, 0, None, (int(c.weight._version) - 1, int(c.weight.data_ptr())))
        got = AG.conv2d(c, xin.clone().requires_grad_())
    c._mnerf_train_pack = None
    assert torch.equal(got, want)


def test_resume_of_a_torch_written_checkpoint_still_clips_on_the_fused_path(tmp_path, monkeypatch):
    """latest.pth written with torch's AdamW (no `max_norm` in its param_groups), resumed with the fused optimizer: the encoder
    group carries optim.clip_enc again and the step leaves a clipped encoder gradient behind."""
    extra = ["--nerf.sample_intvs=32", "--nerf.rand_rays_train=256", "--optim.sched=", "--optim.clip_enc=0.01"]
    c = make_coach(tmp_path, monkeypatch, "clipresume", False, extra, 1)
    torch.manual_seed(0)
    c.train_iteration(scene_batch(c.opts.device, height=64, width=64, n_src_views=3, seed=11))
    c.save_checkpoint(ep=0, it=1)
    r = make_coach(tmp_path, monkeypatch, "clipresume", True, extra + ["--resume=true"], 1)
    r.restore_checkpoint()
    assert r.iter_start == 1 and r.optim.param_groups[0]["max_norm"] == 0.01
    assert all(float(r.optim.state[p]["step"]) == 1.0 for p in r.model.feat_enc.parameters())
    r.it = 1
    r.train_iteration(scene_batch(r.opts.device, height=64, width=64, n_src_views=3, seed=11))
    before = float(r.optim.last_sumsq[0].sqrt())
    after = float(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in r.model.feat_enc.parameters()])))
    print(f"encoder gradient norm before clipping {before:.4e}, after {after:.4e}")
    assert before > 0.01 and abs(after - 0.01) < 1e-5
