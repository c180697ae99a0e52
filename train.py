#!/usr/bin/env python
"""Training entry point on the MI355X hot path (counterpart of the reference's train.py:10-34).

    python train.py --yaml=train --name=run
    python train.py --yaml=train --name=run --resume=true          # continue from outputs/run/models/latest.pth
    python train.py --yaml=train --name=scene --load=ckpt.pth --optim.lr_enc=0   # per-scene fine-tuning of the decoder
    python train.py --yaml=train --name=run --gpu_ids=0,1,2,3      # data-parallel: one process per listed GPU

Options use the reference's ``--a.b.c=value`` grammar and YAML inheritance; the configured data sets are served by seeded
synthetic scenes when no dataset is on disk.

Several GPUs: in a process without ``WORLD_SIZE``, ``--gpu_ids`` longer than one starts one fresh child process per listed GPU
(RANK = position in the list, LOCAL_RANK = the GPU's ordinal, which is what ``dist.init_from_env`` selects the device by), waits for
them and returns non-zero if any fails; the launching process never touches a GPU.  Under ``torchrun`` the ranks it is given are
used as they are.  Every rank holds a full replica and trains on its own ``batch_size`` scenes; the gradients are averaged between
backward and clip + step, so the effective batch is W x ``batch_size`` (learning rates are not rescaled).  Rank r draws rays and
stratified offsets from ``seed + r``; the order of the scenes comes from (seed, epoch) alone.  Rank 0 writes the output directory.
``MNERF_FORCE_DEVICE=0 MNERF_DIST_BACKEND=gloo`` runs all ranks on one GPU (dry runs, tests)."""
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# what a launcher (torchrun, or a run of this file) sets for its ranks: never inherited by the children started here
RANK_VARIABLES = ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "GROUP_RANK", "ROLE_RANK", "ROLE_WORLD_SIZE",
                  "GROUP_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "TORCHELASTIC_RUN_ID", "TORCHELASTIC_RESTART_COUNT",
                  "TORCHELASTIC_MAX_RESTARTS")


def child_environments(gpu_ids, base_env, port):
    """The environments of the ranks of ``--gpu_ids``: one dict per listed GPU, ``base_env`` without any rank variable it may
    hold plus RANK (position in the list), LOCAL_RANK (the GPU's ordinal), WORLD_SIZE and ONE rendezvous address."""
    base = {k: v for k, v in base_env.items() if k not in RANK_VARIABLES}
    return [dict(base, RANK=str(rank), LOCAL_RANK=str(int(gpu)), WORLD_SIZE=str(len(gpu_ids)), LOCAL_WORLD_SIZE=str(len(gpu_ids)),
                 MASTER_ADDR="127.0.0.1", MASTER_PORT=str(int(port))) for rank, gpu in enumerate(gpu_ids)]


def requested_gpu_ids(argv):
    """``gpu_ids`` of the YAML + command line, read without processing the options (nothing here imports torch)"""
    from matchnerf_amd import options
    cmd = options.parse_arguments(argv)
    assert "yaml" in cmd, "--yaml=<config name> is required"
    ids = cmd.get("gpu_ids")
    if ids is None:
        ids = options.load_options("configs/{}.yaml".format(cmd["yaml"]), verbose=False).get("gpu_ids", [0])
    return [ids] if isinstance(ids, int) else list(ids)


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def child_command(argv, script=None):
    """what a rank is started with: this interpreter on ``script`` (default: this file) with the launcher's own arguments"""
    return [sys.executable, os.path.abspath(script or __file__)] + list(argv)


def launch(argv, gpu_ids, script=None):
    """One fresh child per GPU, running ``script`` (default: this file; test.py passes itself); -> 0 when all exit with 0.  When a
    child fails the others are ended (they would wait for it in their next collective) and its status is returned."""
    envs = child_environments(gpu_ids, os.environ, free_port())
    procs = [subprocess.Popen(child_command(argv, script), env=env) for env in envs]
    status = 0
    try:
        while any(p.poll() is None for p in procs):
            failed = [p.returncode for p in procs if p.poll() not in (None, 0)]
            if failed:
                status = failed[0]
                break
            time.sleep(0.2)
        status = status or next((p.returncode for p in procs if p.returncode not in (None, 0)), 0)
    finally:
        for p in procs:
            if p.poll() is None:
                p.terminate()
        for p in procs:
            try:
                p.wait(timeout=30)
            except subprocess.TimeoutExpired:
                p.kill()
                p.wait()
    if status:
        print(f"{os.path.basename(script or __file__)}: a rank failed (exit status {status}); ranks on GPUs {list(gpu_ids)}", file=sys.stderr)
    return status if 0 < status < 256 else (1 if status else 0)


def run(argv):
    import torch
    from matchnerf_amd import dist, options
    from matchnerf_amd.coach import Coach

    rank, world, device = 0, 1, None
    if "WORLD_SIZE" in os.environ or os.environ.get("MNERF_DIST_INIT_ALWAYS"):
        rank, world, device = dist.init_from_env()
    opt = options.set(opt_cmd=options.parse_arguments(argv), make_output_dir=rank == 0, verbose=rank == 0)
    if device is not None:
        opt.device = str(device) if not opt.cpu else "cpu"  # the rank's device is init_from_env's (MNERF_FORCE_DEVICE)
        if opt.seed is not None:
            dist.reseed(opt.seed, rank)
    if rank == 0:
        options.save_options_file(opt)
    dist.barrier()  # the output directory exists before any rank goes on
    if not str(opt.device).startswith("cuda"):
        raise SystemExit("train.py: training needs a GPU (the forward and backward kernels have no CPU path)")
    with torch.cuda.device(opt.device):
        coach = Coach(opt)
        coach.build_networks()
        coach.load_dataset(splits=["train", "val", "test"])
        coach.setup_visualizer()
        coach.setup_optimizer()
        coach.restore_checkpoint()
        coach.train_model()
    if torch.distributed.is_initialized():
        dist.barrier(always=True)
        torch.distributed.destroy_process_group()
    return coach


def main(argv):
    if "WORLD_SIZE" not in os.environ:
        gpu_ids = requested_gpu_ids(argv)
        if len(gpu_ids) > 1:
            return launch(argv, gpu_ids)
    run(argv)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
