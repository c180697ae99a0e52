#!/usr/bin/env python
"""Time the evaluation of test frames: the bare forward pass against Coach.test_model with the host metrics
(MNERF_DEVICE_METRICS=0: metrics.psnr + EvalTools, one device-to-host copy per image) and with the device metrics
(csrc/metrics.hip through metrics.DeviceEval, one copy per loader).

    python tools/eval_time.py                 # one JSON line per figure, a summary line at the end

One process, one GPU: 8 synthetic 512x640 scenes (generated once, outside the timings), 3 source views, S = 64.  After one warm-up
pass of every setting the settings alternate --reps times; a figure is the median over the repetitions of
(wall time of one pass over the 8 scenes, synchronised at its end) / 8, in milliseconds per image:
  (a) forward(mode="test") alone (the batch is moved to the device as test_model moves it);
  (b) test_model, host metrics;      (c) test_model, device metrics;
  (b_mask), (c_mask): the same with a DTU-style ground-truth depth in every batch (holes = 0: the mask path).
(c) - (a) is what evaluation still costs per image; the last lines say where it goes: device time of the two metric launches on
one frame (events), of the mask op (depth == 0), and the host time of DeviceEval.finish() (the one copy of a loader).

    python tools/eval_time.py --lpips [--vgg16 vgg16-397923af.pth --lin vgg.pth]

The LPIPS case: test_model with the two weight files on disk, so that every image gets PSNR, SSIM and LPIPS - with LPIPS on the
device (MNERF_DEVICE_LPIPS=1: csrc/lpips.hip, a fifth column of the device rows) and on the host path (MNERF_DEVICE_LPIPS=0: one
round trip per frame and library convolutions behind EvalTools), crop and mask.  Without the two paths, seeded random weights with
the files' key names are written to the temporary directory (He-scaled convolutions, biases x 0.01, heads uniform in [0, 1)).
The device and the host LPIPS of every frame are printed side by side - with the real files this is where a user sees the
difference on them -, then the device time of one pass over a pair (events) and its kernels one by one (torch.profiler)."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_SCENES, HEIGHT, WIDTH, N_SAMPLES = 8, 512, 640, 64


def emit(**kw):
    print(json.dumps(kw), flush=True)


class Fixed:
    """a handed-in test loader over batches made beforehand"""

    def __init__(self, name, batches):
        self.name, self.batches = name, batches

    def get_name(self):
        return self.name

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter(self.batches)


def make_batches(n_src_views):
    import torch
    from matchnerf_amd import synthetic as syn
    plain, masked = [], []
    yy, xx = torch.meshgrid(torch.arange(HEIGHT), torch.arange(WIDTH), indexing="ij")
    for i in range(N_SCENES):
        sc = syn.make_scene(seed=100 + i, height=HEIGHT, width=WIDTH, n_src_views=n_src_views, near_far=(2.125, 4.525))
        batch = {k: torch.from_numpy(v) for k, v in sc.items()}
        batch["scene"] = [f"synthetic{i}"]
        plain.append(batch)
        # DTU's depth maps are 0 outside the object: an ellipse of valid depth, about 55 % of the frame
        inside = ((yy - HEIGHT / 2) / (0.42 * HEIGHT)) ** 2 + ((xx - WIDTH / 2 - 10 * i) / (0.42 * WIDTH)) ** 2 < 1.0
        masked.append(dict(batch, depth=torch.where(inside, 3.0, 0.0)[None]))
    return plain, masked


def build_coach(out_root):
    from matchnerf_amd import options
    from matchnerf_amd.coach import Coach
    cmd = options.parse_arguments(["--yaml=test", "--name=eval_time", f"--output_root={out_root}", f"--nerf.sample_intvs={N_SAMPLES}",
                                   "--data_test.llff=", "--data_test.blender=", "--data_test.tnt=",
                                   f"--data_test.dtu.img_wh={WIDTH},{HEIGHT}", f"--data_test.dtu.max_len={N_SCENES}"])
    opt = options.set(cmd, verbose=False)
    c = Coach(opt)
    c.build_networks()
    c.restore_checkpoint()
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--lpips", action="store_true", help="the LPIPS case: test_model with the two weight files on disk")
    ap.add_argument("--vgg16", default=None, help="torchvision's vgg16-397923af.pth (default: seeded random weights)")
    ap.add_argument("--lin", default=None, help="lpips v0.1's vgg.pth (default: seeded random weights)")
    args = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="eval_time_")
    cwd = os.getcwd()
    try:
        os.chdir(tmp)
        if args.lpips:
            measure_lpips(args, tmp)
        else:
            measure(args, tmp)
    finally:
        os.chdir(cwd)
        shutil.rmtree(tmp, ignore_errors=True)


def measure(args, tmp):
    import contextlib
    import io

    import torch
    from matchnerf_amd import hip, metrics
    from matchnerf_amd.edict import EasyDict
    if not torch.cuda.is_available():
        raise SystemExit("eval_time.py needs a GPU")
    c = build_coach(tmp)
    plain, masked = make_batches(c.n_src_views)
    loaders = {"crop": Fixed("dtu", plain), "mask": Fixed("dtu", masked)}
    emit(figure="setup", device=torch.cuda.get_device_name(0), scenes=N_SCENES, height=HEIGHT, width=WIDTH, n_src_views=c.n_src_views,
         n_samples=N_SAMPLES, reps=args.reps, masked_share=round(float((masked[0]["depth"] == 0).float().mean()), 3))

    def forward_only(kind):
        c.model.eval()
        with torch.no_grad():
            for batch in loaders[kind]:
                var = EasyDict({k: (v.to(c.opts.device) if torch.is_tensor(v) else v) for k, v in batch.items()})
                var.pop("depth", None)
                c.model(var, mode="test")

    def test_model(kind, device_metrics):
        os.environ["MNERF_DEVICE_METRICS"] = "1" if device_metrics else "0"
        c.load_dataset(loaders=[loaders[kind]])
        with contextlib.redirect_stdout(io.StringIO()):
            return c.test_model()

    settings = [("a_forward", lambda: forward_only("crop")), ("b_host", lambda: test_model("crop", False)),
                ("c_device", lambda: test_model("crop", True)), ("b_mask_host", lambda: test_model("mask", False)),
                ("c_mask_device", lambda: test_model("mask", True))]
    reports = {}
    for name, fn in settings:  # the warm-up pass
        reports[name] = fn()
    torch.cuda.synchronize()
    for host, dev in (("b_host", "c_device"), ("b_mask_host", "c_mask_device")):
        diff = max(abs(reports[host]["dtu"][k] - reports[dev]["dtu"][k]) for k in reports[host]["dtu"])
        emit(figure="agreement", pair=[host, dev], max_psnr_difference_db=diff)
    ms = {name: [] for name, _ in settings}
    for _ in range(args.reps):
        for name, fn in settings:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / N_SCENES)
    med = {k: statistics.median(v) for k, v in ms.items()}
    for name, _ in settings:
        emit(figure=name, ms_per_image_median=round(med[name], 3), ms_per_image_all=[round(x, 3) for x in ms[name]])

    # where (c) - (a) goes: the two launches on one frame, the mask op, the one copy of a loader
    dev = c.opts.device
    pred = torch.rand(1, HEIGHT * WIDTH, 3, device=dev)
    images = torch.rand(1, c.n_src_views + 1, 3, HEIGHT, WIDTH, device=dev)
    depth = masked[0]["depth"].to(dev)
    parts = {}
    for what, fn in (("kernel_crop", lambda: hip.image_metrics(pred, images[:, -1])),
                     ("kernel_mask", lambda: hip.image_metrics(pred, images[:, -1], depth == 0)),
                     ("mask_op", lambda: depth == 0)):
        times = []
        for i in range(25):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= 5:
                times.append(e0.elapsed_time(e1))
        parts[what] = statistics.median(times)
    ev = metrics.DeviceEval()
    for i in range(N_SCENES):
        ev.add(i, pred, images[:, -1])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev.finish()
    parts["finish_one_copy_per_loader_host"] = (time.perf_counter() - t0) * 1e3
    emit(figure="breakdown_ms", **{k: round(v, 4) for k, v in parts.items()},
         note="kernel_*: device time of the two launches + the binding's two allocations on one 512x640 frame (events; kernel_mask "
              "includes the mask op); finish: host time of the one copy of 8 rows, once per loader")
    emit(figure="summary", a_forward=round(med["a_forward"], 3), b_host=round(med["b_host"], 3), c_device=round(med["c_device"], 3),
         b_mask_host=round(med["b_mask_host"], 3), c_mask_device=round(med["c_mask_device"], 3),
         c_minus_a=round(med["c_device"] - med["a_forward"], 3), c_mask_minus_a=round(med["c_mask_device"] - med["a_forward"], 3),
         b_minus_a=round(med["b_host"] - med["a_forward"], 3), b_mask_minus_a=round(med["b_mask_host"] - med["a_forward"], 3),
         c_below_b=bool(med["c_device"] < med["b_host"]), c_mask_below_b_mask=bool(med["c_mask_device"] < med["b_mask_host"]))


def random_lpips_files(tmp):
    import torch
    from matchnerf_amd import metrics
    g = torch.Generator().manual_seed(0)
    vgg = {}
    for i, (ci, co) in metrics.LPIPS_VGG_CONVS.items():
        vgg[f"features.{i}.weight"] = torch.randn(co, ci, 3, 3, generator=g) * (2.0 / (9 * ci)) ** 0.5
        vgg[f"features.{i}.bias"] = torch.randn(co, generator=g) * 0.01
    lin = {f"lin{l}.model.1.weight": torch.rand(1, c, 1, 1, generator=g) for l, c in enumerate(metrics.LPIPS_CHANNELS)}
    paths = os.path.join(tmp, "vgg16_random.pth"), os.path.join(tmp, "lpips_lin_random.pth")
    torch.save(vgg, paths[0])
    torch.save(lin, paths[1])
    return paths


def measure_lpips(args, tmp):
    import contextlib
    import io

    import numpy as np
    import torch
    from matchnerf_amd import hip, metrics
    if not torch.cuda.is_available():
        raise SystemExit("eval_time.py needs a GPU")
    if bool(args.vgg16) != bool(args.lin):
        raise SystemExit("--vgg16 and --lin go together")
    vgg16, lin = (args.vgg16, args.lin) if args.vgg16 else random_lpips_files(tmp)
    os.environ["MNERF_LPIPS_VGG16"], os.environ["MNERF_LPIPS_LIN"] = os.path.abspath(vgg16), os.path.abspath(lin)
    os.environ["MNERF_DEVICE_METRICS"] = "1"
    c = build_coach(tmp)
    plain, masked = make_batches(c.n_src_views)
    loaders = {"crop": Fixed("dtu", plain), "mask": Fixed("dtu", masked)}
    emit(figure="setup", device=torch.cuda.get_device_name(0), scenes=N_SCENES, height=HEIGHT, width=WIDTH, n_src_views=c.n_src_views,
         n_samples=N_SAMPLES, reps=args.reps, weights="files" if args.vgg16 else "seeded random")
    rows = {}
    real = c._evaluate

    def keep(*a, **kw):
        rows["last"] = real(*a, **kw)
        return rows["last"]

    c._evaluate = keep

    def test_model(kind, device_lpips):
        os.environ["MNERF_DEVICE_LPIPS"] = "1" if device_lpips else "0"
        c.load_dataset(loaders=[loaders[kind]])
        with contextlib.redirect_stdout(io.StringIO()):
            c.test_model()
        return rows["last"]

    settings = [("lpips_host", lambda: test_model("crop", False)), ("lpips_device", lambda: test_model("crop", True)),
                ("lpips_mask_host", lambda: test_model("mask", False)), ("lpips_mask_device", lambda: test_model("mask", True))]
    first = {name: fn() for name, fn in settings}  # the warm-up pass (the device path packs its weight streams here, once)
    torch.cuda.synchronize()
    for host, dev in (("lpips_host", "lpips_device"), ("lpips_mask_host", "lpips_mask_device")):
        for rh, rd in zip(first[host], first[dev]):
            emit(figure="lpips_values", pair=[host, dev], image=[int(rh[0]), int(rh[1])], host=float(rh[4]), device=float(rd[4]),
                 difference=float(abs(rh[4] - rd[4])))
        emit(figure="agreement", pair=[host, dev], max_lpips_difference=float(np.abs(first[host][:, 4] - first[dev][:, 4]).max()),
             psnr_ssim_identical=bool(np.array_equal(first[host][:, :4], first[dev][:, :4])))
    ms = {name: [] for name, _ in settings}
    for _ in range(args.reps):
        for name, fn in settings:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / N_SCENES)
    med = {k: statistics.median(v) for k, v in ms.items()}
    for name, _ in settings:
        emit(figure=name, ms_per_image_median=round(med[name], 3), ms_per_image_all=[round(x, 3) for x in ms[name]],
             spread=round(max(ms[name]) - min(ms[name]), 3))

    # one pass over one pair of 512x640 frames: device time (events), then kernel by kernel
    dev = c.opts.device
    lp = metrics.DeviceLPIPS(dev)
    pred = torch.rand(1, HEIGHT * WIDTH, 3, device=dev)
    images = torch.rand(1, c.n_src_views + 1, 3, HEIGHT, WIDTH, device=dev)
    depth = masked[0]["depth"].to(dev)
    parts = {}
    for what, fn in (("lpips_crop", lambda: lp(pred, images[:, -1], None)), ("lpips_mask", lambda: lp(pred, images[:, -1], depth == 0))):
        times = []
        for i in range(15):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= 5:
                times.append(e0.elapsed_time(e1))
        parts[what] = statistics.median(times)
    emit(figure="lpips_pass_ms", **{k: round(v, 4) for k, v in parts.items()},
         note="device time of hip.lpips_vgg on one 512x640 pair (events): input stage, 13 convolutions, 4 pools, 5 heads, the sum")
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            lp(pred, images[:, -1], None)
            torch.cuda.synchronize()
        for ev in prof.events():
            us = float(ev.device_time if hasattr(ev, "device_time") else ev.cuda_time)
            if us > 0:
                emit(figure="lpips_kernel", name=ev.name[:90], us=round(us, 1))
    except Exception as e:  # noqa: BLE001  (the profiler is a convenience of this tool; the event figures above stand)
        emit(figure="lpips_kernel", error=repr(e)[:200])
    emit(figure="summary", lpips_host=round(med["lpips_host"], 3), lpips_device=round(med["lpips_device"], 3),
         lpips_mask_host=round(med["lpips_mask_host"], 3), lpips_mask_device=round(med["lpips_mask_device"], 3),
         device_below_host=bool(med["lpips_device"] < med["lpips_host"]),
         mask_device_below_host=bool(med["lpips_mask_device"] < med["lpips_mask_host"]))


if __name__ == "__main__":
    main()
