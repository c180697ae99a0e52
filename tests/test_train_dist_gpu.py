"""Data-parallel training on the GPU: the pack / unpack kernels of csrc/optim.hip against torch, the fused exchange against the
torch-path exchange, the averaged gradient of two ranks against a one-process yardstick, replicas that stay bit-identical, and
train.py end to end with two ranks.  The GPU box has one MI355X: the ranks are spawned processes that share it
(MNERF_FORCE_DEVICE=0) and talk through gloo, as in tests/test_dist_gpu.py; every wait has a time limit, a failed or late rank ends
the others and fails the test, nothing is retried, at most three ranks run per test."""
import functools
import hashlib
import json
import os
import queue
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import REPO

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 4096, 4097, 262144)
SEED = 0
SMALL = ["--nerf.sample_intvs=32", "--nerf.rand_rays_train=256", "--freq.ckpt_it=-1", "--freq.val_it=-1", "--freq.scalar=1"]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_ranks(target, world, *args, limit=600):
    """``target(rank, world, port, q, *args)`` in ``world`` spawned processes -> their (rank, payload) results, sorted.  A rank
    that reports an exception, dies or is late ends the others and fails the test."""
    assert world <= 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port, q) + tuple(args)) for r in range(world)]
    for p in procs:
        p.start()
    res, failure = [], None
    try:
        for _ in procs:
            try:
                rank, ok, payload = q.get(timeout=limit)
            except queue.Empty:
                failure = f"no result within {limit} s (got {[r[0] for r in res]})"
                break
            if not ok:
                failure = f"rank {rank}: {payload}"
                break
            res.append((rank, payload))
    finally:
        for p in procs:
            p.join(timeout=5 if failure else 60)
            if p.is_alive():
                p.kill()
                p.join(timeout=10)
    assert failure is None, failure
    return [r[1] for r in sorted(res, key=lambda r: r[0])]


def _guarded(fn):
    """worker body -> (rank, True, payload) or (rank, False, traceback) on the queue"""
    @functools.wraps(fn)  # spawn pickles the target by its module-level name
    def run(rank, world, port, q, *args):
        try:
            q.put((rank, True, fn(rank, world, port, *args)))
        except BaseException as e:  # noqa: BLE001
            import traceback
            q.put((rank, False, repr(e) + "\n" + traceback.format_exc()[-3000:]))
    return run


def _join_group(rank, world, port, backend="gloo", fused=True):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      MNERF_FORCE_DEVICE="0", MNERF_FUSED_OPTIM="1" if fused else "0")
    if backend == "gloo":
        os.environ["MNERF_DIST_BACKEND"] = "gloo"
        os.environ.pop("MNERF_DIST_INIT_ALWAYS", None)
    else:
        os.environ.pop("MNERF_DIST_BACKEND", None)
        os.environ["MNERF_DIST_INIT_ALWAYS"] = "1"
        os.environ["HSA_ENABLE_IPC_MODE_LEGACY"] = os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    from matchnerf_amd import dist as mdist
    return mdist.init_from_env()


def _leave_group():
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


# ------------------------------------------------------------------------------------------------ stub tensors


def make_params(device="cuda"):
    """parameters of SIZES elements whose gradients alternate between 16-byte aligned tensors and views that start one float into a
    larger buffer (4-byte aligned only); -> (params, the gradients' backing buffers)"""
    params, backing = [], []
    for i, n in enumerate(SIZES):
        p = torch.nn.Parameter(torch.zeros(n, device=device))
        base = torch.full((n + 9,), -7.0, device=device)
        p.grad = base[1:1 + n] if i % 2 else base[4:4 + n]
        assert p.grad.data_ptr() % 16 == (4 if i % 2 else 0) and p.grad.is_contiguous()
        params.append(p)
        backing.append(base)
    return params, backing


def fill_grads(params, seed):
    g = torch.Generator().manual_seed(seed)
    vals = [torch.randn(p.numel(), generator=g) for p in params]
    for p, v in zip(params, vals):
        p.grad.copy_(v)
    return vals


def host_bucket(vals, side, n_blocks, begin):
    from matchnerf_amd import hip
    b = torch.zeros(hip.grad_bucket_floats(n_blocks))
    for v, at in zip(vals, begin):
        b[at * hip.OPTIM_CHUNK:at * hip.OPTIM_CHUNK + v.numel()] = v
    b[n_blocks * hip.OPTIM_CHUNK:n_blocks * hip.OPTIM_CHUNK + side.numel()] = side
    return b


# ------------------------------------------------------------------------------------------------ 5. kernels against torch


def test_pack_and_unpack_kernels_are_bit_exact():
    """Copies and one fp32 multiply: pack against a bucket built on the host (padding and unused side slots zero, starting from a
    bucket full of NaN), unpack with scale = fp32(1/3) against bucket * scale; the floats around a 4-byte-aligned gradient are left
    alone; wrong arguments return the library's error codes."""
    from matchnerf_amd import hip
    from matchnerf_amd.optim import RowTable, mean_scale, row_blocks
    lib = hip.load()
    params, backing = make_params()
    vals = fill_grads(params, 1)
    side = torch.tensor([0.75, -3.5], device="cuda")
    begin, n_blocks = row_blocks(SIZES)
    rt = RowTable("test")
    rt.rebuild(tuple(map(id, params)), params)
    assert rt.n_blocks == n_blocks == 69
    rows = rt.send(params)
    bucket = torch.full((hip.grad_bucket_floats(n_blocks),), float("nan"), device="cuda")
    hip.grad_pack(rows, len(params), n_blocks, bucket, side)
    want = host_bucket(vals, side.cpu(), n_blocks, begin)
    got = bucket.cpu()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    hip.grad_pack(rows, len(params), n_blocks, bucket.fill_(float("nan")), None)  # no side values: the side chunk is all zero
    assert not bucket[n_blocks * hip.OPTIM_CHUNK:].any() and torch.equal(bucket[:n_blocks * hip.OPTIM_CHUNK].cpu(),
                                                                       want[:n_blocks * hip.OPTIM_CHUNK])

    summed = (want * 3.0 + 0.125).cuda()  # some other bucket, as a collective would leave it
    scale = mean_scale(3)
    assert scale == float(np.float32(1.0) / np.float32(3.0))
    side_out = torch.full((2,), float("nan"), device="cuda")
    hip.grad_unpack(rows, len(params), n_blocks, summed, scale, side_out)
    ref = (summed * torch.tensor(scale, dtype=torch.float32, device="cuda")).cpu()
    for p, base, at, i in zip(params, backing, begin, range(len(params))):
        n = p.numel()
        assert torch.equal(p.grad.cpu().view(torch.int32), ref[at * hip.OPTIM_CHUNK:at * hip.OPTIM_CHUNK + n].view(torch.int32)), n
        lead = 1 if i % 2 else 4
        assert bool((base[:lead] == -7.0).all()) and bool((base[lead + n:] == -7.0).all()), n  # nothing written around it
    assert torch.equal(side_out.cpu(), ref[n_blocks * hip.OPTIM_CHUNK:n_blocks * hip.OPTIM_CHUNK + 2])

    rp, bp = rows.data_ptr(), bucket.data_ptr()
    assert lib.mnerf_grad_pack(rp, 5, n_blocks, None, 0, None, None) == hip.MNERF_E_NULL
    assert lib.mnerf_grad_pack(rp, 5, 4, None, 0, bp, None) == hip.MNERF_E_RANGE          # n_blocks < n_rows
    assert lib.mnerf_grad_pack(rp + 8, 5, n_blocks, None, 0, bp, None) == hip.MNERF_E_ALIGN  # a misaligned table
    assert lib.mnerf_grad_pack(rp, 5, n_blocks, None, 0, bp + 4, None) == hip.MNERF_E_ALIGN
    assert lib.mnerf_grad_unpack(rp, 5, n_blocks, None, 0.5, None, 0, None) == hip.MNERF_E_NULL
    assert lib.mnerf_grad_unpack(rp, 5, 4, bp, 0.5, None, 0, None) == hip.MNERF_E_RANGE
    assert lib.mnerf_grad_unpack(rp + 8, 5, n_blocks, bp, 0.5, None, 0, None) == hip.MNERF_E_ALIGN
    assert lib.mnerf_grad_unpack(rp, 5, n_blocks, bp, 0.5, None, 2, None) == hip.MNERF_E_NULL
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 6. fused path = torch path


@_guarded
def _both_paths_worker(rank, world, port):
    _join_group(rank, world, port)
    from matchnerf_amd.optim import GradBucket, mean_scale, reduce_gradients_torch
    params, _ = make_params()
    every = [[torch.randn(n, generator=torch.Generator().manual_seed(100 * r + i)) for i, n in enumerate(SIZES)] for r in range(world)]
    sides = [torch.tensor([0.1 * (r + 1), 3.0 - r]) for r in range(world)]

    def load():
        for p, v in zip(params, every[rank]):
            p.grad.copy_(v)
        return sides[rank].cuda()

    bucket = GradBucket()
    out = {}
    for name, fn in (("fused", bucket.reduce), ("fused again", bucket.reduce), ("torch", reduce_gradients_torch)):
        side = fn(params, load())
        out[name] = ([p.grad.cpu().clone() for p in params], side.cpu())
    scale = torch.tensor(mean_scale(world))
    ok = True
    for i in range(len(params)):
        want = every[0][i].clone()
        for r in range(1, world):
            want += every[r][i]  # the ranks in rank order
        want *= scale
        for name in out:
            ok &= torch.equal(out[name][0][i].view(torch.int32), want.view(torch.int32))
    want_side = sides[0].clone()
    for r in range(1, world):
        want_side += sides[r]
    ok &= all(torch.equal(out[name][1], want_side * scale) for name in out)
    ok &= all(torch.equal(a, b) for a, b in zip(out["fused"][0], out["torch"][0]))
    _leave_group()
    return bool(ok)


@pytest.mark.parametrize("world", [2, 3])
def test_fused_exchange_equals_the_torch_exchange(world):
    """same seeded gradients per rank: after the fused exchange every .grad has the bits the torch-path exchange leaves, and both
    are (g0 + g1 [+ g2]) * fp32(1 / W)"""
    assert _run_ranks(_both_paths_worker, world) == [True] * world


# ------------------------------------------------------------------------------------------------ the real model in ranks


def _coach(tmp, name, rank, world, fused, extra, n_train, device):
    """tests/test_train_gpu.py's make_coach for a rank of a process group"""
    from matchnerf_amd import options, synthetic as syn
    from matchnerf_amd.coach import Coach
    os.chdir(tmp)
    os.environ["MNERF_FUSED_OPTIM"] = "1" if fused else "0"
    ids = ",".join(str(i) for i in range(max(world, 1)))
    cmd = options.parse_arguments(["--yaml=train", f"--name={name}", "--tb=false", f"--output_root={tmp}", f"--seed={SEED}",
                                   f"--gpu_ids={ids}"] + list(extra))
    opt = options.set(cmd, make_output_dir=rank == 0, verbose=False)
    if device is not None:
        opt.device = str(device)
    if torch.distributed.is_initialized():
        torch.distributed.barrier()
    c = Coach(opt)
    c.build_networks()
    c.model.load_state_dict(syn.to_torch(syn.seeded_state_dict(syn.state_dict_spec(n_src_views=3), 1), opt.device))

    class Loader:
        def __len__(self):
            return n_train
    c.train_loader = Loader()
    c.setup_optimizer()
    assert c.fused_optim == fused
    c.it, c.ep = 0, 0
    c.model.train()
    return c


def _scene(device, seed):
    from matchnerf_amd import synthetic as syn
    from matchnerf_amd.edict import EasyDict
    return EasyDict({k: torch.from_numpy(v).to(device) for k, v in syn.make_scene(height=64, width=64, n_src_views=3, seed=seed).items()})


def _gradient_before_the_step(c, var):
    """one train_iteration whose optimizer step is replaced by a snapshot of the gradients it would have consumed"""
    snap = []
    step = c.optim.step
    c.optim.step = lambda: snap.extend(p.grad.detach().clone() for g in c.optim.param_groups for p in g["params"])
    try:
        loss = c.train_iteration(var)
    finally:
        c.optim.step = step
    return snap, loss


@_guarded
def _gradient_worker(rank, world, port, tmp):
    from matchnerf_amd import dist as mdist
    _, _, dev = _join_group(rank, world, port)
    c = _coach(tmp, "grad", rank, world, True, SMALL, 4, dev)
    assert c.distributed and c.world == world
    mdist.reseed(SEED, rank)
    snap, _ = _gradient_before_the_step(c, _scene(dev, 11 + rank))
    torch.cuda.synchronize()
    grads = [g.cpu() for g in snap]
    digest = hashlib.sha256(b"".join(g.numpy().tobytes() for g in grads)).hexdigest()
    if rank == 0:
        torch.save(grads, os.path.join(tmp, "rank0_grads.pt"))
    _leave_group()
    return digest


def test_two_ranks_average_gradient_matches_a_one_process_yardstick(tmp_path, monkeypatch):
    """The real model at 64 x 64, W = 2, one scene per rank.  Yardstick: this process evaluates rank 0's and rank 1's iterations one
    after the other with the ranks' seeds (seed + r, set right before the iteration as the ranks do) and forms (gA + gB) * 0.5 in
    fp32 - three times; s = its own largest run-to-run difference per tensor.  The ranks' averaged gradient must lie within
    max(8 s, 2^-20 max|g|) of the first yardstick, per tensor.  If the backward is bit-reproducible only a commutative fp32 add
    separates the two; if its atomics reorder sums, s measures exactly that, and the factor 8 covers three samples under-estimating
    a spread.  Every tensor's s and error are printed before anything is asserted.

    Measured on MI355X (profiles/current/train_dist_tests_gpu.log): s is NOT zero - 152 of the 153 tensors differ between two
    evaluations in one process (the backward's atomics reorder sums), s from 2.9e-11 to 2.4e-07 (out_alpha_linear.2.weight, max|g| 2.5e+00).
    Worst pair: nerf_dec.ray_attention.layer_norm.bias, s 1.49e-08, error 2.98e-08 against a bound of 1.22e-07 (error / bound 0.245);
    every other tensor's error is below a quarter of its bound."""
    from matchnerf_amd import dist as mdist
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("MNERF_FUSED_OPTIM", "1")
    c = _coach(str(tmp_path), "yard", 0, 1, True, SMALL, 4, None)
    assert not c.distributed
    names = [n for n, p in c.model.named_parameters() if p.requires_grad]
    yard = []
    for _ in range(3):
        per_rank = []
        for r in range(2):
            mdist.reseed(SEED, r)
            snap, _ = _gradient_before_the_step(c, _scene(c.opts.device, 11 + r))
            per_rank.append(snap)
        yard.append([((a + b) * 0.5).cpu() for a, b in zip(*per_rank)])
    torch.cuda.synchronize()
    del c
    torch.cuda.empty_cache()

    digests = _run_ranks(_gradient_worker, 2, str(tmp_path))
    assert digests[0] == digests[1]  # both ranks hold the same averaged gradient
    got = torch.load(os.path.join(tmp_path, "rank0_grads.pt"))
    assert len(got) == len(yard[0]) == len(names) == 153
    worst, misses = None, []
    for i, name in enumerate(names):
        s = max(float((yard[a][i] - yard[b][i]).abs().max()) for a, b in ((0, 1), (0, 2), (1, 2)))
        gmax = float(yard[0][i].abs().max())
        bound = max(8 * s, 2.0 ** -20 * gmax)
        err = float((got[i] - yard[0][i]).abs().max())
        print(f"{name}: s {s:.3e}  max|g| {gmax:.3e}  bound {bound:.3e}  err {err:.3e}  {'ok' if err <= bound else 'MISS'}")
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
        if worst is None or ratio > worst[0]:
            worst = (ratio, name, s, err, bound)
        if err > bound:
            misses.append(name)
    print(f"worst pair: {worst[1]}  s {worst[2]:.3e}  err {worst[3]:.3e}  bound {worst[4]:.3e}  err/bound {worst[0]:.3f}")
    assert all(float(g.abs().max()) > 0 for g in got)
    assert not misses, misses


def _state_digest(c):
    h = hashlib.sha256()
    for g in c.optim.param_groups:
        for p in g["params"]:
            st = c.optim.state[p]
            for t in (p.detach(), st["exp_avg"], st["exp_avg_sq"]):
                h.update(t.cpu().numpy().tobytes())
    return h.hexdigest()


@_guarded
def _replica_worker(rank, world, port, tmp, fused):
    from matchnerf_amd import dist as mdist
    _, _, dev = _join_group(rank, world, port, fused=fused)
    c = _coach(tmp, f"rep{world}{int(fused)}", rank, world, fused, SMALL + ["--max_epoch=2"], 4, dev)
    assert c.sched_type == "OneCycleLR" and (c._bucket is not None) == fused
    start = [p.detach().clone() for p in c.model.parameters()]
    mdist.reseed(SEED, rank)
    losses, lrs = [], []
    for i in range(3):
        lrs.append([g["lr"] for g in c.optim.param_groups])
        losses.append(c.train_iteration(_scene(dev, 11 + 3 * i + rank)).all.detach())
        c.sched.step()
    torch.cuda.synchronize()
    moved = all(not torch.equal(p.detach(), s) for p, s in zip(c.model.parameters(), start))
    steps = {float(c.optim.state[p]["step"]) for g in c.optim.param_groups for p in g["params"]}
    out = dict(digest=_state_digest(c), moved=bool(moved), steps=sorted(steps), lrs=lrs,
               losses=[float(np.float32(float(x))) for x in losses])
    _leave_group()
    return out


@pytest.mark.parametrize("world,fused", [(2, True), (3, True), (2, False)], ids=["w2-fused", "w3-fused", "w2-torch"])
def test_replicas_stay_bit_identical(tmp_path, world, fused):
    """three Coach.train_iteration's with the scheduler stepping: every parameter, exp_avg and exp_avg_sq tensor has the same bits
    on every rank and differs from the start; the loss rank 0 logged is the fp32 sum of the ranks' own losses (in rank order)
    times fp32(1 / W), exactly."""
    res = _run_ranks(_replica_worker, world, str(tmp_path), fused)
    assert len({r["digest"] for r in res}) == 1, [r["digest"] for r in res]
    assert all(r["moved"] and r["steps"] == [3.0] and r["lrs"] == res[0]["lrs"] for r in res)
    assert len({tuple(r["losses"]) for r in res}) == world  # different scenes and rays per rank
    rows = [json.loads(l) for l in open(os.path.join(tmp_path, f"rep{world}{int(fused)}", "scalars.jsonl"))]
    logged = [r["value"] for r in rows if r["tag"] == "loss_render"]
    scale = np.float32(1.0) / np.float32(world)
    want = []
    for i in range(3):
        total = np.float32(res[0]["losses"][i])
        for r in range(1, world):
            total = total + np.float32(res[r]["losses"][i])
        want.append(float(total * scale))
    print("logged", logged, "ranks' own", [r["losses"] for r in res])
    assert len(logged) == 3  # rank 0 alone wrote
    assert logged == want


# ------------------------------------------------------------------------------------------------ 9. train.py end to end


def _train_py(args, cwd, limit=600):
    env = dict(os.environ, MNERF_FORCE_DEVICE="0", MNERF_DIST_BACKEND="gloo")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "MNERF_DIST_INIT_ALWAYS"):
        env.pop(k, None)
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.join(REPO, "train.py")] + args, cwd=cwd, env=env,
                       capture_output=True, text=True)
    print(r.stdout[-3000:], r.stderr[-3000:])
    return r


def test_train_py_with_two_ranks_then_resume_and_a_refused_world_size(tmp_path):
    """`python train.py --gpu_ids=0,1` launches its two ranks itself (both on this box's one GPU, gloo): 6 synthetic scenes are
    6 // 2 = 3 iterations, rank 0 alone writes latest.pth (world size 2 in it) and scalars.jsonl; three ranks refuse to resume that
    mid-epoch checkpoint; two ranks continue from it."""
    args = ["--yaml=train", "--name=ddp", "--gpu_ids=0,1", "--max_epoch=1", "--tb=false", "--data_train.img_wh=64,64",
            "--data_train.max_len=6", "--data_val.img_wh=64,64", "--data_val.max_len=1", "--nerf.rand_rays_train=96",
            "--nerf.rand_rays_val=4096", "--freq.ckpt_ep=-1", "--freq.ckpt_it=0.5", "--freq.val_it=0.5", "--freq.scalar=1",
            "--data_test.llff=", "--data_test.blender=", "--data_test.dtu.img_wh=64,64", "--data_test.dtu.max_len=1",
            "--nerf.sample_intvs=16", "--nerf.rand_rays_test=4096", f"--output_root={tmp_path}"]
    r = _train_py(args, tmp_path)
    assert r.returncode == 0
    out = os.path.join(tmp_path, "ddp")
    assert "data-parallel: 2 ranks" in r.stdout and r.stdout.count("training done: 3 iterations") == 1
    found = [os.path.join(d, f) for d, _, fs in os.walk(tmp_path) for f in fs if f in ("latest.pth", "scalars.jsonl")]
    assert sorted(found) == [os.path.join(out, "models", "latest.pth"), os.path.join(out, "scalars.jsonl")]
    ck = torch.load(os.path.join(out, "models", "latest.pth"), map_location="cpu", weights_only=False)
    assert set(ck) == {"model", "optim", "sched", "epoch", "iter", "world_size"}
    assert (ck["world_size"], ck["epoch"], ck["iter"]) == (2, 0, 2)  # ckpt_it = ceil(0.5 * 3): written in the middle of epoch 0
    rows = [json.loads(l) for l in open(os.path.join(out, "scalars.jsonl"))]
    assert sum(x["split"] == "train" and x["tag"] == "loss_render" for x in rows) == 3 == 6 // 2
    assert sum(x["split"] == "val" and x["tag"] == "PSNR" for x in rows) >= 1
    assert open(os.path.join(out, "run.bash")).read().count("train.py") == 1

    three = [a for a in args if not a.startswith("--gpu_ids")] + ["--gpu_ids=0,1,2", "--resume=true"]
    r = _train_py(three, tmp_path)
    assert r.returncode != 0
    assert "written in the middle of epoch 0" in r.stderr and "world size 2" in r.stderr and "world size 3" in r.stderr
    assert len(open(os.path.join(out, "scalars.jsonl")).readlines()) == len(rows)  # nothing trained

    r = _train_py([a for a in args if a != "--freq.ckpt_ep=-1"] + ["--freq.ckpt_ep=1", "--resume=true"], tmp_path)
    assert r.returncode == 0
    assert "resuming from epoch 0 (iteration 2)" in r.stdout and "training done: 3 iterations" in r.stdout
    rows2 = [json.loads(l) for l in open(os.path.join(out, "scalars.jsonl"))]
    assert sum(x["split"] == "train" and x["tag"] == "loss_render" for x in rows2) == 4  # the one iteration that was left
    ck = torch.load(os.path.join(out, "models", "latest.pth"), map_location="cpu", weights_only=False)
    assert (ck["world_size"], ck["epoch"], ck["iter"]) == (2, 1, 3)


# ------------------------------------------------------------------------------------------------ 10. the device collective


@_guarded
def _rccl_worker(rank, world, port):
    _, _, dev = _join_group(rank, world, port, backend="nccl")
    assert torch.distributed.get_backend() == "nccl" and dev.type == "cuda"
    from matchnerf_amd.optim import GradBucket
    params, _ = make_params()
    vals = fill_grads(params, 5)
    side = GradBucket().reduce(params, torch.tensor([1.25, -2.0], device="cuda"), always=True)
    ok = all(torch.equal(p.grad.cpu().view(torch.int32), v.view(torch.int32)) for p, v in zip(params, vals))
    ok &= torch.equal(side.cpu(), torch.tensor([1.25, -2.0]))
    _leave_group()
    return bool(ok)


def test_the_device_collective_runs_in_a_one_rank_rccl_group():
    """pack -> all_reduce on the DEVICE bucket -> unpack in a one-rank RCCL group (MNERF_DIST_INIT_ALWAYS=1): sum of one, scale
    1.0 - the gradients and side values come back with the bits they had"""
    assert _run_ranks(_rccl_worker, 1, limit=300) == [True]
