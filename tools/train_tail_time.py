#!/usr/bin/env python
"""Time the tail of a training iteration (gradient clipping + AdamW step) and whole iterations, torch's path against the fused HIP
path (csrc/optim.hip, optim.FusedAdamW), and count kernel launches per iteration.

    python tools/train_tail_time.py                  # (a) + (b) + (c), one JSON line per figure
    python tools/train_tail_time.py --skip-trace     # without the rocprofv3 runs

(a) clip + step on the real model's parameter set with fixed gradients: torch.nn.utils.clip_grad_norm_ on the encoder + foreach
    torch.optim.AdamW against FusedAdamW.step().  Per call: device time between two events around it (median of --runs calls after
    --warmup) and host time per call.  Twice: gradient norm above max_norm (the gradients are scaled;
    they are restored from a copy before every call, outside the events) and below it.
(b) Coach.train_iteration at the bench's training shape (512x640, 1024 random rays, S = 64 and 128, 3 source views) with
    MNERF_FUSED_OPTIM=0 and 1: median wall time per iteration, synchronised per iteration.
(c) kernel dispatches per iteration: a child process per setting under `rocprofv3 --kernel-trace --stats` (no counters in the same
    run), counted over the last full periods between two forward decoder launches (one per iteration)."""
import argparse
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def emit(**kw):
    print(json.dumps(kw), flush=True)


def build_coach(fused, n_samples, out_root):
    import torch
    from matchnerf_amd import options, synthetic as syn
    from matchnerf_amd.coach import Coach
    os.environ["MNERF_FUSED_OPTIM"] = "1" if fused else "0"
    cmd = options.parse_arguments(["--yaml=train", f"--name=tail{int(fused)}_{n_samples}", "--tb=false", f"--output_root={out_root}",
                                   f"--nerf.sample_intvs={n_samples}", "--optim.sched=", "--freq.scalar=-1"])
    opt = options.set(cmd, verbose=False)
    c = Coach(opt)
    c.build_networks()
    c.model.load_state_dict(syn.to_torch(syn.seeded_state_dict(syn.state_dict_spec(n_src_views=3), 1), opt.device))

    class One:
        def __len__(self):
            return 1
    c.train_loader = One()
    c.setup_optimizer()
    for g in c.optim.param_groups:
        g["lr"] = 1e-7  # the timing scene stays put (as bench.py's train_step_workload)
    c.it, c.ep = 0, 0
    c.model.train()
    from matchnerf_amd.edict import EasyDict
    scene = syn.make_scene(512, 640, 3, seed=0)
    batch = lambda: EasyDict({k: torch.from_numpy(v).to(opt.device) for k, v in scene.items()})  # noqa: E731
    return c, batch


def tail(args):
    import torch
    from matchnerf_amd import options
    from matchnerf_amd.models import models_dict
    from matchnerf_amd.optim import FusedAdamW
    opt = options.load_options("configs/train.yaml", verbose=False)
    opt.device = "cuda:0"
    model = models_dict[opt.model](opt).to("cuda:0")
    enc, dec = list(model.feat_enc.parameters()), list(model.nerf_dec.parameters())
    params = enc + dec
    emit(figure="parameter_set", tensors=len(params), elements=sum(p.numel() for p in params),
         smallest=min(p.numel() for p in params), largest=max(p.numel() for p in params))
    g = torch.Generator(device="cuda").manual_seed(0)
    master = [torch.randn(p.shape, device="cuda", generator=g) for p in params]
    enc_norm = float(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(m) for m in master[:len(enc)]])))
    for case, target in (("clipped", 4.0), ("unclipped", 0.25)):
        grads = [m * (target / enc_norm) for m in master]
        for p in params:
            p.grad = torch.empty_like(p)
        tv = torch.optim.AdamW([dict(params=enc, lr=1e-7), dict(params=dec, lr=1e-7)], weight_decay=1e-4, foreach=True)
        fv = FusedAdamW([dict(params=enc, lr=1e-7, max_norm=1.0), dict(params=dec, lr=1e-7)], weight_decay=1e-4)

        def torch_tail():
            torch.nn.utils.clip_grad_norm_(enc, 1.0)
            tv.step()

        res = {}
        for name, fn in (("torch", torch_tail), ("fused", fv.step)):
            ms = []
            for i in range(args.warmup + args.runs):
                torch._foreach_copy_([p.grad for p in params], grads)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if i >= args.warmup:
                    ms.append(e0.elapsed_time(e1))
            torch.cuda.synchronize()
            host = 0.0
            for _ in range(args.runs):  # host time of the call alone; the gradients are restored before every call here too
                torch._foreach_copy_([p.grad for p in params], grads)
                t0 = time.perf_counter()
                fn()
                host += time.perf_counter() - t0
            torch.cuda.synchronize()
            res[name] = dict(event_ms_median=statistics.median(ms), event_ms_min=min(ms), host_ms_per_call=host / args.runs * 1e3)
        emit(figure="a_tail", case=case, runs=args.runs, **{f"{k}_{m}": round(v, 4) for k, r in res.items() for m, v in r.items()},
             speedup_event=round(res["torch"]["event_ms_median"] / res["fused"]["event_ms_median"], 2))


def iterations(fused, n_samples, n, warmup, out_root, sync=True):
    import torch
    c, batch = build_coach(fused, n_samples, out_root)
    torch.manual_seed(0)
    ms = []
    for i in range(warmup + n):
        var = batch()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c.train_iteration(var)
        if sync:
            torch.cuda.synchronize()
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    torch.cuda.synchronize()
    return ms


def dispatches_per_iteration(db, periods):
    import sqlite3
    cur = sqlite3.connect(db).cursor()
    tables = [r[0] for r in cur.execute("select name from sqlite_master where type in ('table', 'view')")]
    cols = [r[1] for r in cur.execute("pragma table_info(kernels)")] if "kernels" in tables else []
    names = [c for c in cols if "name" in c]
    if not names or "start" not in cols:
        raise RuntimeError(f"{db}: expected rocprofv3's rocpd view `kernels` with a name and a `start` column (as tools/rocpd_stats.py "
                           f"reads it); found tables {tables[:12]}, columns {cols}")
    name_col = "name" if "name" in cols else names[0]
    rows = cur.execute(f"select {name_col}, start from kernels").fetchall()
    dec = sorted(s for n, s in rows if ("decoder_kernel" in n or "decoder_pp_kernel" in n) and "backward" not in n)
    assert len(dec) > periods, (len(dec), periods)
    inside = [n for n, s in rows if dec[-periods - 1] <= s < dec[-1]]
    tail_names = ("adamw_step_kernel", "grad_sumsq", "l2_loss_kernel", "multi_tensor", "vectorized_elementwise", "reduce_kernel")
    return len(inside) / periods, sum(any(t in n for t in tail_names) for n in inside) / periods


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--skip-trace", action="store_true")
    ap.add_argument("--child", nargs=2, metavar=("FUSED", "S"), help="internal: run iterations for the kernel trace and exit")
    args = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="train_tail_")
    try:
        measure(args, tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def measure(args, tmp):
    if args.child:
        iterations(bool(int(args.child[0])), int(args.child[1]), 8, 3, tmp, sync=False)
        return
    tail(args)
    for s in (64, 128):
        res = {}
        for fused in (0, 1):
            ms = iterations(bool(fused), s, args.iters, 3, tmp)
            res[fused] = statistics.median(ms)
            emit(figure="b_train_iteration", n_samples=s, fused_optim=fused, iterations=args.iters, ms_median=round(res[fused], 3),
                 ms_min=round(min(ms), 3), ms_max=round(max(ms), 3))
        emit(figure="b_difference", n_samples=s, torch_minus_fused_ms=round(res[0] - res[1], 3))
    if args.skip_trace:
        return
    for fused in (0, 1):
        d = os.path.join(tmp, f"trace{fused}")
        cmd = ["timeout", "-k", "10", "400", "rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "t", "--", sys.executable,
               os.path.abspath(__file__), "--child", str(fused), "64"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        dbs = glob.glob(os.path.join(d, "**", "*_results.db"), recursive=True)
        if r.returncode != 0 or not dbs:
            emit(figure="c_launches", fused_optim=fused, error=f"rocprofv3 exit {r.returncode}", stderr=r.stderr[-400:])
            if r.returncode != 0:
                return  # nothing more on the GPU after a failed run
            continue
        try:
            total, tail_like = dispatches_per_iteration(dbs[0], 5)
        except Exception as e:  # noqa: BLE001
            emit(figure="c_launches", fused_optim=fused, error=f"{type(e).__name__}: {e}"[:500])
            continue
        emit(figure="c_launches", fused_optim=fused, n_samples=64, dispatches_per_iteration=total,
             of_which_elementwise_reduce_or_optimizer=tail_like)


if __name__ == "__main__":
    main()
