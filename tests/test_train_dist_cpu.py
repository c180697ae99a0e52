"""Host side of data-parallel training, without a GPU: the rank-aware order of the scenes, the layout of the gradient bucket, the
environments train.py gives its ranks, and the torch-path gradient exchange between two gloo ranks on CPU tensors."""
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import REPO
from matchnerf_amd import hip, options
from matchnerf_amd.coach import Coach, SyntheticScenes
from matchnerf_amd.edict import EasyDict

SIZES = (1, 3, 4096, 4097, 262144)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


# ------------------------------------------------------------------------------------------------ 1. loader partition


def _coach(tmp_path, monkeypatch, name, rank, world, extra=()):
    monkeypatch.chdir(tmp_path)
    data = list(extra) or ["--data_train.root_dir=", "--data_train.dataset_name=synthetic", "--data_train.max_len=7"]
    cmd = options.parse_arguments(["--yaml=train", f"--name={name}", "--cpu=true", "--tb=false", f"--output_root={tmp_path}",
                                   "--seed=5"] + data)
    c = Coach(options.set(cmd, verbose=False))
    c.rank, c.world, c.distributed = rank, world, True  # as in a process group of that size
    return c


@pytest.mark.parametrize("world", [2, 3])
def test_ranks_take_disjoint_equal_shares_of_one_permutation(tmp_path, monkeypatch, world):
    def shares(epoch, reseed_with=None):
        out = []
        for r in range(world):
            c = _coach(tmp_path, monkeypatch, f"part{world}", r, world)
            if reseed_with is not None:
                torch.manual_seed(reseed_with + r)  # training reseeds the global generator per rank; the order must not care
                torch.rand(r + 1)
            c.load_dataset(splits=["train"])
            assert isinstance(c.train_loader, SyntheticScenes) and len(c.train_loader) == 7 // world
            c.train_loader.set_epoch(epoch)
            idx = c.train_loader.indices()
            assert [b["scene"][0] for b in c.train_loader] == [f"synthetic{i}" for i in idx]  # what is iterated is what is listed
            out.append(idx)
        return out

    e0 = shares(0)
    flat = [i for s in e0 for i in s]
    assert all(len(s) == 7 // world for s in e0) and len(set(flat)) == len(flat) and set(flat) <= set(range(7))
    # drawn from ONE permutation: rank r holds elements r, r + W, ... of the permutation of (seed, epoch)
    perm = torch.randperm(7, generator=torch.Generator().manual_seed(5 + 0)).tolist()
    assert e0 == [perm[r:(7 // world) * world:world] for r in range(world)]
    e1 = shares(1)
    assert e1 != e0 and len({i for s in e1 for i in s}) == (7 // world) * world
    assert shares(0) == e0  # rebuilt with the same seed (resume): the same order
    assert shares(0, reseed_with=100) == e0 and shares(1, reseed_with=977) == e1  # whatever the global generator holds


def test_one_process_keeps_the_global_generator_order(tmp_path, monkeypatch):
    """no process group: the training order is torch.randperm from the global generator, as before"""
    c = _coach(tmp_path, monkeypatch, "single", 0, 1)
    c.distributed = False
    c.load_dataset(splits=["train"])
    assert len(c.train_loader) == 7
    torch.manual_seed(11)
    want = torch.randperm(7).tolist()
    torch.manual_seed(11)
    assert c.train_loader.indices() == want


def test_distributed_sampler_serves_the_on_disk_sets(tmp_path, monkeypatch):
    """an on-disk data set gets DistributedSampler(num_replicas=W, rank=r, seed=opts.seed, drop_last=True)"""
    from test_datasets import _make_dtu
    root = tmp_path / "dtu"
    meta, pairs = _make_dtu(root, tmp_path)
    seen = []
    for r in range(2):
        c = _coach(tmp_path, monkeypatch, "disk", r, 2, [f"--data_train.root_dir={root}", "--data_train.dataset_name=dtu",
                                                        "--data_train.max_len=-1", "--data_train.num_workers=0",
                                                        "--data_train.img_wh=64,32", f"--data_train.meta_dir={meta}",
                                                        f"--data_train.pairs_file={pairs}"])
        c.load_dataset(splits=["train"])
        s = c.train_loader.sampler
        assert isinstance(s, torch.utils.data.DistributedSampler) and (s.num_replicas, s.rank, s.seed, s.drop_last) == (2, r, 5, True)
        assert len(c.train_loader) == c._n_train // 2 == c._epoch_len(2)
        s.set_epoch(0)
        seen.append(list(s))
    assert not set(seen[0]) & set(seen[1]) and len(seen[0]) == len(seen[1])


# ------------------------------------------------------------------------------------------------ 2. bucket layout


def test_bucket_layout_and_numpy_round_trip():
    from matchnerf_amd.optim import mean_scale, row_blocks
    lib = hip.load()
    begin, n_blocks = row_blocks(SIZES)
    assert begin.tolist() == [0, 1, 2, 3, 5] and n_blocks == 5 + 64
    assert lib.mnerf_grad_bucket_floats(n_blocks) == hip.grad_bucket_floats(n_blocks) == (n_blocks + 1) * hip.OPTIM_CHUNK
    assert lib.mnerf_grad_bucket_floats(0) == -1 and lib.mnerf_grad_bucket_floats(1) == 2 * hip.OPTIM_CHUNK
    # the model's own table: 4 772 532 parameters in 153 tensors, 5.8 % padding inside the rows' chunks, then the side chunk
    from matchnerf_amd.models import models_dict
    opt = options.load_options("configs/train.yaml", verbose=False)
    opt.device = "cpu"
    numels = [p.numel() for p in models_dict[opt.model](opt).parameters()]
    blocks = row_blocks(numels)[1]
    floats = hip.grad_bucket_floats(blocks)
    print(f"{len(numels)} tensors, {sum(numels)} elements, {blocks} chunks, bucket {floats} floats")
    assert (len(numels), sum(numels)) == (153, 4772532) and blocks * hip.OPTIM_CHUNK - sum(numels) == 277836
    assert floats == (blocks + 1) * hip.OPTIM_CHUNK == 5054464

    # pack -> sum over W -> unpack in numpy
    def pack(grads, side):
        b = np.full(hip.grad_bucket_floats(n_blocks), np.nan, np.float32)  # every float must be written
        for g, at in zip(grads, begin):
            chunks = -(-g.size // hip.OPTIM_CHUNK)
            slot = b[at * hip.OPTIM_CHUNK:(at + chunks) * hip.OPTIM_CHUNK]
            slot[:g.size], slot[g.size:] = g, 0
        tail = b[n_blocks * hip.OPTIM_CHUNK:]
        tail[:side.size], tail[side.size:] = side, 0
        return b

    for world in (2, 3):
        rng = np.random.default_rng(world)
        grads = [[rng.standard_normal(n).astype(np.float32) for n in SIZES] for _ in range(world)]
        sides = [rng.standard_normal(2).astype(np.float32) for _ in range(world)]
        total = pack(grads[0], sides[0])
        for r in range(1, world):
            total = total + pack(grads[r], sides[r])
        scale = np.float32(mean_scale(world))
        assert scale == np.float32(1.0) / np.float32(world) and float(scale) == mean_scale(world)
        out = total * scale
        mask = np.ones(out.size, bool)
        for i, (n, at) in enumerate(zip(SIZES, begin)):
            want = grads[0][i]
            for r in range(1, world):
                want = want + grads[r][i]
            got = out[at * hip.OPTIM_CHUNK:at * hip.OPTIM_CHUNK + n]
            assert np.array_equal(got.view(np.int32), (want * scale).view(np.int32))
            mask[at * hip.OPTIM_CHUNK:at * hip.OPTIM_CHUNK + n] = False
        mask[n_blocks * hip.OPTIM_CHUNK:n_blocks * hip.OPTIM_CHUNK + 2] = False
        assert mask.sum() == out.size - sum(SIZES) - 2 and not out[mask].any()  # padding comes back as zero


def test_exchange_entry_points_check_their_arguments_on_the_host():
    lib = hip.load()
    assert lib.mnerf_grad_pack(None, 2, 5, None, 0, 32, None) == hip.MNERF_E_NULL
    assert lib.mnerf_grad_pack(16, 2, 5, None, 0, None, None) == hip.MNERF_E_NULL and b"bucket" in lib.mnerf_last_error()
    assert lib.mnerf_grad_pack(16, 6, 5, None, 0, 32, None) == hip.MNERF_E_RANGE
    assert lib.mnerf_grad_pack(20, 2, 5, None, 0, 32, None) == hip.MNERF_E_ALIGN
    assert lib.mnerf_grad_pack(16, 2, 5, None, 0, 36, None) == hip.MNERF_E_ALIGN
    assert lib.mnerf_grad_pack(16, 2, 5, None, 3, 32, None) == hip.MNERF_E_NULL
    assert lib.mnerf_grad_pack(16, 2, 5, 16, hip.OPTIM_CHUNK + 1, 32, None) == hip.MNERF_E_RANGE
    assert lib.mnerf_grad_unpack(None, 2, 5, 32, 0.5, None, 0, None) == hip.MNERF_E_NULL
    assert lib.mnerf_grad_unpack(16, 2, 5, None, 0.5, None, 0, None) == hip.MNERF_E_NULL
    assert lib.mnerf_grad_unpack(16, 2, 1, 32, 0.5, None, 0, None) == hip.MNERF_E_RANGE
    assert lib.mnerf_grad_unpack(24, 2, 5, 32, 0.5, None, 0, None) == hip.MNERF_E_ALIGN
    assert lib.mnerf_grad_unpack(16, 2, 5, 32, 0.5, None, 1, None) == hip.MNERF_E_NULL


# ------------------------------------------------------------------------------------------------ 3. launcher environments


def test_launcher_builds_the_ranks_environments():
    import train
    base = {"PATH": "/bin", "MNERF_FORCE_DEVICE": "0", "RANK": "9", "LOCAL_RANK": "9", "WORLD_SIZE": "12", "MASTER_PORT": "1",
            "MASTER_ADDR": "elsewhere", "GROUP_RANK": "4", "TORCHELASTIC_RUN_ID": "x"}
    envs = train.child_environments([2, 5, 7], base, 29731)
    assert len(envs) == 3
    for rank, (env, gpu) in enumerate(zip(envs, (2, 5, 7))):
        assert (env["RANK"], env["LOCAL_RANK"], env["WORLD_SIZE"]) == (str(rank), str(gpu), "3")
        assert env["MASTER_PORT"] == "29731" and env["MASTER_ADDR"] == "127.0.0.1"
        assert "GROUP_RANK" not in env and "TORCHELASTIC_RUN_ID" not in env
        assert env["PATH"] == "/bin" and env["MNERF_FORCE_DEVICE"] == "0"
    assert base["RANK"] == "9"  # the caller's environment is left alone
    assert train.requested_gpu_ids(["--yaml=train", "--gpu_ids=2,5,7"]) == [2, 5, 7]
    assert train.requested_gpu_ids(["--yaml=train", "--gpu_ids=3"]) == [3]
    assert train.requested_gpu_ids(["--yaml=train"]) == [0]


# ------------------------------------------------------------------------------------------------ 4. two gloo ranks on CPU tensors


def _stub_batch(rank):
    g = torch.Generator().manual_seed(40 + rank)
    return {"images": torch.rand(1, 4, 3, 4, 4, generator=g)}


def _exchange_worker(rank, world, port, tmp, q):
    try:
        os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                          MASTER_PORT=str(port), MNERF_DIST_BACKEND="gloo", MNERF_FUSED_OPTIM="0")
        os.environ.pop("MNERF_DIST_INIT_ALWAYS", None)
        import datetime

        import torch.distributed as td
        from matchnerf_amd import models
        from matchnerf_amd.optim import mean_scale, reduce_gradients_torch
        from test_train_cpu import StubLoader, StubModel
        td.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
        models.models_dict["stub"] = StubModel
        os.chdir(tmp)
        cmd = options.parse_arguments(["--yaml=train", "--name=ddp", "--cpu=true", "--max_epoch=3", "--tb=false", f"--output_root={tmp}",
                                       "--model=stub", "--nerf.rand_rays_train=4", "--freq.scalar=1", "--gpu_ids=0,1",
                                       "--freq.ckpt_it=-1", "--freq.val_it=-1"])
        opt = options.set(cmd, make_output_dir=rank == 0, verbose=False)
        td.barrier()
        c = Coach(opt)
        assert (c.rank, c.world, c.distributed) == (rank, world, True)
        c.build_networks()
        c.train_loader = StubLoader(6)
        c.setup_optimizer()  # gpu_ids of length 2 in a group of 2: accepted
        assert type(c.optim) is torch.optim.AdamW
        c.it, c.ep = 0, 0
        start = [p.detach().clone() for p in c.model.parameters()]

        # every rank works out BOTH ranks' gradients and losses (same weights), then exchanges its own
        own = {}
        for r in range(world):
            c.optim.zero_grad(set_to_none=True)
            var = EasyDict(_stub_batch(r))
            loss = c.compute_loss(c.model(var, mode="train"), var, mode="train").render
            loss.backward()
            own[r] = ([p.grad.clone() for p in c.model.parameters()], loss.detach().clone())
        scale = torch.tensor(mean_scale(world), dtype=torch.float32)
        for p, g in zip(c.model.parameters(), own[rank][0]):
            p.grad = g.clone()
        side = c.exchange_gradients(own[rank][1].reshape(1))
        ok_grads = all(torch.equal(p.grad, (a + b) * scale) for p, a, b in zip(c.model.parameters(), own[0][0], own[1][0]))
        ok_side = torch.equal(side, ((own[0][1] + own[1][1]) * scale).reshape(1))

        # a row list that differs on rank 1: BOTH ranks raise, nobody is left waiting
        params = list(c.model.parameters())
        raised = ""
        try:
            reduce_gradients_torch(params[:-1] if rank == 1 else params)
        except RuntimeError as e:
            raised = str(e)
        td.barrier()  # both ranks are still in step

        # one whole iteration: the logged loss is the mean, the replicas end equal
        mine = c.train_iteration(EasyDict(_stub_batch(rank)))
        moved = any(not torch.equal(p.detach(), s) for p, s in zip(c.model.parameters(), start))
        td.barrier()
        q.put((rank, bool(ok_grads), bool(ok_side), raised, float(mine.all.detach()), float(own[0][1]), float(own[1][1]),
               [p.detach().numpy().tobytes() for p in c.model.parameters()], bool(moved)))
        td.destroy_process_group()
    except Exception as e:  # noqa: BLE001
        import traceback
        q.put((rank, False, False, "EXC " + repr(e) + traceback.format_exc()[-1500:], 0.0, 0.0, 0.0, [], False))


def test_two_gloo_ranks_average_gradients_and_raise_together(tmp_path):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_exchange_worker, args=(r, 2, port, str(tmp_path), q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = sorted(q.get(timeout=240) for _ in procs)
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    assert not any(r[3].startswith("EXC") for r in res), [r[3] for r in res]
    assert [r[:3] for r in res] == [(0, True, True), (1, True, True)], res
    assert all("disagree" in r[3] for r in res), [r[3] for r in res]  # raised on BOTH ranks
    assert res[0][7] == res[1][7] and res[0][8] and res[1][8]  # replicas bit-identical after the step, and they moved
    # rank 0 alone wrote the scalars, and the loss in them is fp32 (l0 + l1) * 0.5 of the ranks' own losses
    assert (res[0][4], res[1][4]) == (res[0][5], res[0][6])
    rows = [json.loads(l) for l in open(os.path.join(tmp_path, "ddp", "scalars.jsonl"))]
    logged = [r["value"] for r in rows if r["tag"] == "loss_render"]
    want = float((np.float32(res[0][5]) + np.float32(res[0][6])) * np.float32(0.5))
    assert logged == [want] and len(rows) == 3


# ------------------------------------------------------------------------------------------------ resume rules, launcher status


def test_resume_at_another_world_size_only_from_an_epoch_boundary(tmp_path, monkeypatch):
    c = _coach(tmp_path, monkeypatch, "resume", 0, 3)
    c.load_dataset(splits=["train"])
    assert len(c.train_loader) == 2 and c._epoch_len(2) == 3 and c._epoch_len(1) == 7
    c._ckpt_extra = {"world_size": 2}
    c.epoch_start, c.iter_start = 1, 3  # the end of epoch 0 at world size 2: allowed, epoch 1 starts from its first batch
    c._check_resumed_world("latest.pth")
    assert c._skip_to == 1 * 2
    c.epoch_start, c.iter_start = 0, 2  # the middle of epoch 0
    with pytest.raises(RuntimeError, match="written in the middle of epoch 0 .* world size 2; this run has world size 3"):
        c._check_resumed_world("latest.pth")
    c._ckpt_extra = {}  # written by one process
    c.epoch_start, c.iter_start = 2, 14
    c._check_resumed_world("latest.pth")
    c.epoch_start, c.iter_start = 2, 15
    with pytest.raises(RuntimeError, match="world size 1"):
        c._check_resumed_world("latest.pth")
    same = _coach(tmp_path, monkeypatch, "resume", 1, 2)
    same.load_dataset(splits=["train"])
    same._ckpt_extra = {"world_size": 2}
    same.epoch_start, same.iter_start = 0, 2
    same._check_resumed_world("latest.pth")  # its own world size: any iteration
    assert not hasattr(same, "_skip_to")


def test_launcher_returns_non_zero_when_a_rank_fails(tmp_path):
    """`train.py --gpu_ids=0,1` starts its ranks as fresh processes and reports a failing one: with --cpu=true every rank stops at
    "training needs a GPU" (nothing here touches a GPU)"""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.update(MNERF_DIST_BACKEND="gloo", MNERF_FORCE_DEVICE="0")  # on a box that has one GPU both ranks name device 0
    r = subprocess.run([sys.executable, os.path.join(REPO, "train.py"), "--yaml=train", "--name=refused", "--gpu_ids=0,1", "--cpu=true",
                        "--tb=false", f"--output_root={tmp_path}"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "training needs a GPU" in r.stderr and "a rank failed" in r.stderr
    assert open(os.path.join(tmp_path, "refused", "run.bash")).read().count("train.py") == 1  # rank 0 alone made the directory


def test_epoch_boundary_resume_at_another_world_size_rebuilds_the_one_cycle_schedule(tmp_path, monkeypatch):
    """A checkpoint written by two ranks at the end of epoch 0 (2 steps per epoch there) resumed by ONE process with 5 steps per
    epoch: the saved OneCycleLR would end after 3 x 2 steps; the resumed run gets a schedule of 3 x 5 steps advanced to epoch 1,
    and trains epochs 1 and 2 to the end."""
    from test_train_cpu import stub_coach
    monkeypatch.setenv("MNERF_FUSED_OPTIM", "0")
    c = stub_coach(tmp_path, monkeypatch)
    c.train_loader.n = 2  # what each of two ranks saw of 5 scenes
    c._make_sched()
    assert c.sched.total_steps == 6
    c.it, c.ep, c.world = 0, 0, 2
    for b in c.train_loader:
        c.train_iteration(EasyDict(b))
        c.sched.step()
    c.save_checkpoint(ep=1, it=2)
    saved = torch.load(os.path.join(c.opts.output_path, "models", "latest.pth"), weights_only=False)
    assert (saved["world_size"], saved["epoch"], saved["iter"]) == (2, 1, 2) and saved["sched"]["total_steps"] == 6

    r = stub_coach(tmp_path, monkeypatch, ["--resume=true", "--freq.ckpt_ep=-1", "--freq.val_it=-1", "--freq.val_ep=-1",
                                           "--freq.ckpt_it=-1", "--freq.test_ep=-1"])
    assert r.world == 1 and len(r.train_loader) == 5
    r.restore_checkpoint()
    assert (r.epoch_start, r.iter_start, r._skip_to) == (1, 2, 5)
    ref_opt = torch.optim.AdamW([dict(params=[torch.nn.Parameter(torch.zeros(1))], lr=r.opts.optim.lr_enc),
                                 dict(params=[torch.nn.Parameter(torch.zeros(1))], lr=r.opts.optim.lr_dec)])
    ref = torch.optim.lr_scheduler.OneCycleLR(ref_opt, max_lr=[r.opts.optim.lr_enc, r.opts.optim.lr_dec], epochs=3, steps_per_epoch=5,
                                              pct_start=0.05, cycle_momentum=False, anneal_strategy="cos")
    for _ in range(5):
        ref_opt.step(), ref.step()
    assert r.sched.total_steps == 15 and [g["lr"] for g in r.optim.param_groups] == [g["lr"] for g in ref_opt.param_groups]
    r.train_model()  # epochs 1 and 2: ten more steps, no "Tried to step" from the schedule
    assert r.it == 2 + 10


# ------------------------------------------------------------------------------------------------ three gloo ranks: the order of the sum


def _sum_order_worker(rank, world, port, q):
    try:
        import datetime

        import torch.distributed as td
        from matchnerf_amd.optim import sum_over_ranks
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        td.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
        n, pad = 1_000_000, 277836
        vals = [torch.randn(n, generator=torch.Generator().manual_seed(r)) for r in range(world)]
        dense = sum_over_ranks(vals[rank].clone())
        padded = sum_over_ranks(torch.cat([torch.zeros(pad), vals[rank]]))
        want = (vals[0] + vals[1]) + vals[2]
        ours = torch.equal(dense, want) and torch.equal(padded[pad:], want) and not bool(padded[:pad].any())
        a, b = vals[rank].clone(), torch.cat([torch.zeros(pad), vals[rank]])
        td.all_reduce(a), td.all_reduce(b)  # what the transport's own all_reduce does with the same two layouts
        q.put((rank, bool(ours), int((a != b[pad:]).sum()), ""))
        td.destroy_process_group()
    except Exception as e:  # noqa: BLE001
        q.put((rank, False, -1, repr(e)))


def test_three_gloo_ranks_are_summed_in_rank_order_whatever_the_layout():
    """optim.sum_over_ranks over gloo at W = 3: (r0 + r1) + r2 for every element, the same bits for a dense buffer and for the same
    values behind 277 836 floats of padding (the bucket's), which is what lets the fused and the torch exchange be compared exactly.
    gloo's own all_reduce on the two layouts is run next to it and the number of elements on which ITS two results differ is
    printed (position-dependent order of the ring; measured: DESIGN.md section 4), not asserted."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_sum_order_worker, args=(r, 3, port, q)) for r in range(3)]
    for p in procs:
        p.start()
    try:
        res = sorted(q.get(timeout=240) for _ in procs)
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    print("gloo all_reduce, dense against padded layout: elements that differ of 1 000 000 per rank:", [r[2] for r in res])
    assert [r[:2] for r in res] == [(0, True), (1, True), (2, True)], res
