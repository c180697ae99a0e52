#!/usr/bin/env python
"""Time the gradient exchange of data-parallel training on ONE GPU, in a forced one-rank RCCL group (MNERF_DIST_INIT_ALWAYS=1): the
per-rank parts of an exchange that a box without a second GPU can measure.  What the all-reduce costs over xGMI between 2-8 ranks is
NOT measured here.

    python tools/train_dist_time.py                         # (a) + (b), one JSON line per figure
    python tools/train_dist_time.py --parent-tree DIR       # (b) against another checkout (its own built library) in the same job

(a) pack, the collective (all_reduce of the device bucket in the one-rank group) and unpack on the real model's parameter set,
    each between two events of its own: median of --runs calls after --warmup.
(b) Coach.train_iteration at the bench's training shape (512x640, 1024 random rays, S = 64 and 128, 3 source views, fused optimizer)
    with the exchange, against the same iteration without a process group - run from --parent-tree when given (the commit before
    the exchange existed), from this tree otherwise.  Every measurement is a fresh child process; the two alternate, --rounds
    each, and the medians over all their iterations are compared."""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

TOOLS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TOOLS)
sys.path.insert(0, ROOT)


def emit(**kw):
    print(json.dumps(kw), flush=True)


def one_rank_group():
    from matchnerf_amd import dist
    os.environ.update(RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MNERF_DIST_INIT_ALWAYS="1")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if "MASTER_PORT" not in os.environ:  # a port nobody holds: the box may be shared
        import socket
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        os.environ["MASTER_PORT"] = str(s.getsockname()[1])
        s.close()
    os.environ.pop("MNERF_DIST_BACKEND", None)
    return dist.init_from_env()


def parts(args):
    import torch
    import torch.distributed as td
    from matchnerf_amd import hip, options
    from matchnerf_amd.models import models_dict
    from matchnerf_amd.optim import RowTable
    _, _, dev = one_rank_group()
    assert td.get_backend() == "nccl"
    opt = options.load_options("configs/train.yaml", verbose=False)
    opt.device = str(dev)
    model = models_dict[opt.model](opt).to(dev)
    params = list(model.feat_enc.parameters()) + list(model.nerf_dec.parameters())
    g = torch.Generator(device="cuda").manual_seed(0)
    for p in params:
        p.grad = torch.randn(p.shape, device="cuda", generator=g)
    rt = RowTable("train_dist_time")
    rt.rebuild(tuple(map(id, params)), params)
    rows, n_rows, n_blocks = rt.send(params), len(params), rt.n_blocks
    bucket = torch.empty(hip.grad_bucket_floats(n_blocks), device="cuda")
    side, side_out = torch.ones(2, device="cuda"), torch.empty(2, device="cuda")
    emit(figure="bucket", tensors=n_rows, elements=sum(p.numel() for p in params), chunks=n_blocks, bucket_floats=bucket.numel(),
         bucket_mb=round(bucket.numel() * 4 / 1e6, 2))
    steps = (("pack", lambda: hip.grad_pack(rows, n_rows, n_blocks, bucket, side)),
             ("all_reduce_one_rank", lambda: td.all_reduce(bucket)),
             ("unpack", lambda: hip.grad_unpack(rows, n_rows, n_blocks, bucket, 1.0, side_out)))
    ms = {name: [] for name, _ in steps}
    for i in range(args.warmup + args.runs):
        for name, fn in steps:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= args.warmup:
                ms[name].append(e0.elapsed_time(e1))
    moved = bucket.numel() * 4 * 2  # one read and one write of the bucket's size per kernel
    for name, _ in steps:
        med = statistics.median(ms[name])
        emit(figure="a_exchange_part", part=name, runs=args.runs, event_ms_median=round(med, 4), event_ms_min=round(min(ms[name]), 4),
             gb_per_s=round(moved / med / 1e6, 1) if name != "all_reduce_one_rank" else None)
    td.destroy_process_group()


def child(args):
    """iterations of Coach.train_iteration in this process: from --tree (no process group) or from this tree in a one-rank group"""
    import train_tail_time as tail  # its build_coach / iterations; it imports the package lazily
    if args.tree:
        sys.path.insert(0, os.path.abspath(args.tree))
    else:
        one_rank_group()
    import matchnerf_amd
    tmp = tempfile.mkdtemp(prefix="train_dist_")
    try:
        ms = tail.iterations(True, args.child, args.iters, 3, tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    emit(figure="child", this_tree=os.path.samefile(os.path.dirname(matchnerf_amd.__file__), os.path.join(ROOT, "matchnerf_amd")), ms=ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--parent-tree", help="a checkout of the commit to compare with, library built")
    ap.add_argument("--skip-parts", action="store_true")
    ap.add_argument("--parts-only", action="store_true", help="internal: (a) in this process, then exit")
    ap.add_argument("--child", type=int, metavar="S", help="internal: run the iterations at S samples per ray and exit")
    ap.add_argument("--tree", help="internal: with --child, import the package from this checkout and use no process group")
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.parts_only:
        return parts(args)
    if not args.skip_parts:
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--parts-only", "--runs", str(args.runs),
                            "--warmup", str(args.warmup)])
        if r.returncode != 0:
            emit(figure="a_exchange_part", error=f"exit {r.returncode}")
            return r.returncode  # nothing more on the GPU after a failed run
    base_tree = args.parent_tree or ROOT
    for s in (64, 128):
        ms, where = {"without": [], "with": []}, {}
        for _ in range(args.rounds):
            for which in ("without", "with"):
                cmd = ["timeout", "-k", "10", "400", sys.executable, os.path.abspath(__file__), "--child", str(s), "--iters", str(args.iters)]
                env = dict(os.environ)
                if which == "without":
                    cmd += ["--tree", base_tree]
                    for k in ("MNERF_DIST_INIT_ALWAYS", "WORLD_SIZE", "RANK", "LOCAL_RANK"):
                        env.pop(k, None)
                r = subprocess.run(cmd, env=env, capture_output=True, text=True)
                lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith('{"figure": "child"')]
                if r.returncode != 0 or not lines:
                    emit(figure="b_train_iteration", n_samples=s, exchange=which, error=f"exit {r.returncode}", stderr=r.stderr[-600:])
                    return 1  # nothing more on the GPU after a failed run
                ms[which] += lines[0]["ms"]
                where[which] = "this tree" if lines[0]["this_tree"] else "the other tree"
        for which in ("without", "with"):
            emit(figure="b_train_iteration", n_samples=s, exchange=which, tree=("parent" if args.parent_tree and which == "without" else "this"),
                 iterations=len(ms[which]), ms_median=round(statistics.median(ms[which]), 3), ms_min=round(min(ms[which]), 3),
                 ms_max=round(max(ms[which]), 3))
        emit(figure="b_difference", n_samples=s, with_minus_without_ms=round(statistics.median(ms["with"]) - statistics.median(ms["without"]), 3),
             packages=where)
    return 0


if __name__ == "__main__":
    sys.exit(main())
