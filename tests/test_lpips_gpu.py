"""csrc/lpips.hip on the GPU: the wide convolution, the max-pool and the head alone, hip.lpips_vgg end to end, the gain logic on a
layer-rescaled network, independence of the batch and reproducibility, Coach.test_model with MNERF_DEVICE_LPIPS on and off, and the
sharded run.

Weights are seeded random tensors with torchvision's and lpips's key names (the recipe of tests/test_datasets.py: He-scaled
convolutions, biases x 0.01, heads uniform in [0, 1)).  The yardstick is metrics.LPIPSVGG in float64 on the CPU, fed float64 copies
of the same fp32 images after EvalTools.set_inputs - never the code under test.

Gates (set by the interface and the definitions, not by what the kernels give):
  convolution   3e-6 x the largest output: the gate tests/test_conv.py holds mnerf_conv2d to
  max-pool      bit-equal to F.max_pool2d
  head          1e-10: "the same definition in another summation order"
  end to end    |d - d64| <= 1e-5 max(1, d64): the gate of tests/test_datasets.py for this quantity, a fifth of half a unit of the
                last digit 0results_*.txt prints; pred == gt and an all-masked frame give exactly 0.0

Measured on MI355X: wide convolutions 0.67e-6 .. 1.38e-6 of the largest output (512 -> 512 at 5 x 5 the largest); head 1.1e-16 at 64 and
at 512 channels; end to end |d - d64| at most 7.2e-8 (64 x 80 crop, independent noise, d = 0.736), 1e-10 .. 4.5e-8 on the other
contents, the same figures on the layer-rescaled network (5.1e-8 at 40 x 52: the gains follow the scales exactly); pred == gt and
the all-masked frame exactly 0.0; the LPIPS of Coach.test_model's two paths (fp32 library
convolutions on the host path) differs by at most 4e-8 (1.09772189 / 1.09772193)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import REPO
from matchnerf_amd import gmflow as G
from matchnerf_amd import hip, metrics

pytestmark = pytest.mark.gpu

_CACHE = {}


def state_dict():
    """(vgg file contents, lin file contents) of the seeded random network"""
    if "sd" not in _CACHE:
        g = torch.Generator().manual_seed(0)
        vgg = {}
        for i, (ci, co) in metrics.LPIPS_VGG_CONVS.items():
            vgg[f"features.{i}.weight"] = torch.randn(co, ci, 3, 3, generator=g) * (2.0 / (9 * ci)) ** 0.5
            vgg[f"features.{i}.bias"] = torch.randn(co, generator=g) * 0.01
        lin = {f"lin{l}.model.1.weight": torch.rand(1, c, 1, 1, generator=g) for l, c in enumerate(metrics.LPIPS_CHANNELS)}
        _CACHE["sd"] = (vgg, lin)
    return _CACHE["sd"]


def rescaled_state_dict():
    """layer k's weight x s_k and bias x s_1 ... s_k, s alternating between 2^5 and 2^-4: every feature map is a power of two times the
    original one (ReLU is positively homogeneous), every stage is unit-normalised, so d changes only through the 1e-10 term"""
    if "sd_scaled" not in _CACHE:
        vgg, lin = state_dict()
        out, total = {}, 1.0
        for k, i in enumerate(sorted(metrics.LPIPS_VGG_CONVS)):
            s = 2.0 ** 5 if k % 2 == 0 else 2.0 ** -4
            total *= s
            out[f"features.{i}.weight"] = vgg[f"features.{i}.weight"] * s
            out[f"features.{i}.bias"] = vgg[f"features.{i}.bias"] * total
        _CACHE["sd_scaled"] = (out, lin)
    return _CACHE["sd_scaled"]


def net64(sd):
    net = metrics._lpips_module()()
    net.load_state_dict({**sd[0], **sd[1]}, strict=True)
    return net.double().eval()


def yardstick(sd, pred, gt, mask):
    """pred / gt [n,h,w,3] fp32 numpy, mask [n,h,w] bool or None -> float64 [n]"""
    key = ("net", id(sd[0]))
    if key not in _CACHE:
        _CACHE[key] = net64(sd)
    net, out = _CACHE[key], []
    to_t = lambda a: torch.from_numpy(np.ascontiguousarray(a))[None].permute(0, 3, 1, 2) * 2 - 1.0
    for i in range(pred.shape[0]):
        tools = metrics.EvalTools()
        tools.set_inputs(pred[i].astype(np.float64), gt[i].astype(np.float64), None if mask is None else mask[i])
        with torch.no_grad():
            out.append(float(net(to_t(tools.proc_pred), to_t(tools.proc_gt)).item()))
    return np.asarray(out, np.float64)


def device_lpips(sd):
    key = ("dev", id(sd[0]))
    if key not in _CACHE:
        _CACHE[key] = metrics.DeviceLPIPS("cuda", state_dict={**sd[0], **sd[1]})
    return _CACHE[key]


def on_device(sd, pred, gt, mask):
    n, h, w, _ = pred.shape
    p = torch.from_numpy(pred).cuda().reshape(n, h * w, 3)
    g = torch.from_numpy(gt).cuda().permute(0, 3, 1, 2).contiguous()
    m = None if mask is None else torch.from_numpy(mask).cuda()
    return device_lpips(sd)(p, g, m).cpu().numpy()


def make_images(h, w, seed):
    """-> pred, gt [5,h,w,3] fp32: independent noise; two smooth pairs; gt + 0.02 noise; pred == gt"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    smooth = lambda a, b, p: 0.5 + 0.4 * np.sin(a * yy[..., None] + b * xx[..., None] + p + np.arange(3))
    gt = [rng.random((h, w, 3)), smooth(0.21, 0.13, 0.0), smooth(0.05, 0.31, 1.0), rng.random((h, w, 3)), rng.random((h, w, 3))]
    pred = [rng.random((h, w, 3)), smooth(0.19, 0.15, 0.3), smooth(0.07, 0.29, 0.8), gt[3] + 0.02 * rng.standard_normal((h, w, 3)), gt[4]]
    return np.stack(pred).astype(np.float32), np.stack(gt).astype(np.float32)


def make_mask(kind, n, h, w, seed):
    if kind == "none":
        return None
    m = np.random.default_rng(seed + 7).random((n, h, w)) < 0.3
    m[0] = True  # a mask that drops every pixel
    return m


CASES = [(40, 52, "none"), (37, 50, "random30"), (64, 80, "none"), (64, 80, "random30")]


def case(h, w, kind):
    key = ("case", h, w, kind)
    if key not in _CACHE:
        pred, gt = make_images(h, w, seed=h * 100 + w)
        mask = make_mask(kind, pred.shape[0], h, w, seed=h * 100 + w)
        _CACHE[key] = (pred, gt, mask, yardstick(state_dict(), pred, gt, mask))
    return _CACHE[key]


def check(got, want, what, zero):
    for i, (a, b) in enumerate(zip(got, want)):
        print(f"{what} image {i}: device {a!r}  float64 {b!r}  |diff| {abs(a - b):.3e}  gate {1e-5 * max(1.0, b):.1e}")
    for i, (a, b) in enumerate(zip(got, want)):
        assert abs(a - b) <= 1e-5 * max(1.0, b), (what, i, a, b)
        if i in zero:
            assert a == 0.0 and b == 0.0, (what, i, a, b)


# ------------------------------------------------------------------------------------------------ the building blocks


def _conv(x, wt, bias, relu=True):
    ws, ew = G.pack_conv_blocks(wt)
    scal = hip.absmax_regions(2, "cuda")
    hip.absmax(x.cuda(), scal[0])
    co, ci = wt.shape[:2]
    got = hip.conv2d(x.cuda(), torch.from_numpy(ws).cuda(), bias.cuda(), ci, co, 3, 1, ew, scal[0], leaky=0.0 if relu else 1.0,
                     out_absmax=scal[1])
    return got, scal, (ws, ew)


@pytest.mark.parametrize("ci,co,h,w", [(128, 256, 9, 12), (256, 512, 4, 6), (256, 512, 5, 5), (512, 512, 4, 6), (512, 512, 5, 5)])
def test_wide_convolution_with_bias_and_relu_matches_float64(ci, co, h, w):
    gen = torch.Generator().manual_seed(ci + co + h)
    x = torch.randn(2, ci, h, w, generator=gen) * (0.5 + 4 * torch.rand(1, ci, 1, 1, generator=gen))
    x[0, 0, 0, 0] = 37.0  # one spike: sets the tensor's operand scale
    wt = torch.randn(co, ci, 3, 3, generator=gen) * (2.0 / (9 * ci)) ** 0.5
    bias = torch.randn(co, generator=gen)
    got, scal, _ = _conv(x, wt, bias)
    want = F.relu(F.conv2d(x.double(), wt.double(), bias.double(), padding=1))
    assert got.shape == want.shape
    err = float((got.cpu().double() - want).abs().max())
    print(f"\nwide conv {ci}->{co} at {h}x{w}: |err| {err:.2e}, max|want| {float(want.abs().max()):.2e}, ratio {err / float(want.abs().max()):.2e}")
    assert err < 3e-6 * float(want.abs().max())
    assert float(hip.absmax_value(scal[1])) == float(got.abs().max())


def test_the_64_channel_layer_is_todays_instance():
    """64 -> 64 at 18 x 25 through the block-wise stream and through pack_conv: one block, the same instance, the same bits"""
    gen = torch.Generator().manual_seed(64)
    x = torch.randn(2, 64, 18, 25, generator=gen)
    wt = torch.randn(64, 64, 3, 3, generator=gen) * (2.0 / (9 * 64)) ** 0.5
    bias = torch.randn(64, generator=gen)
    got, scal, (ws, ew) = _conv(x, wt, bias)
    ws0, ew0 = G.pack_conv(wt)
    assert ew0 == ew and np.array_equal(ws0.view(np.uint32), ws.view(np.uint32))
    old = hip.conv2d(x.cuda(), torch.from_numpy(ws0).cuda(), bias.cuda(), 64, 64, 3, 1, ew0, scal[0], leaky=0.0)
    assert torch.equal(got.view(torch.int32), old.view(torch.int32))
    want = F.relu(F.conv2d(x.double(), wt.double(), bias.double(), padding=1))
    assert float((got.cpu().double() - want).abs().max()) < 3e-6 * float(want.abs().max())


@pytest.mark.parametrize("h,w", [(37, 50), (18, 25), (9, 12)])
def test_maxpool_is_bit_equal_to_torch(h, w):
    x = torch.randn(2, 5, h, w, generator=torch.Generator().manual_seed(h))
    got = hip.maxpool2x2(x.cuda()).cpu()
    want = F.max_pool2d(x, 2, 2)
    assert got.shape == want.shape == (2, 5, h // 2, w // 2)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("c", [64, 512])
def test_head_alone_matches_float64(c):
    gen = torch.Generator().manual_seed(c)
    a, b = torch.randn(c, 5, 7, generator=gen).relu(), torch.randn(c, 5, 7, generator=gen).relu()
    a[:, 2, 3] = 0.0  # a pixel whose features are all zero in one image: the 1e-10 term
    wv = torch.rand(c, generator=gen)
    got = float(hip.lpips_head(a.cuda(), b.cuda(), wv.cuda()).item())
    ad, bd = a.double(), b.double()
    na = ad / (ad.pow(2).sum(0, keepdim=True).sqrt() + 1e-10)
    nb = bd / (bd.pow(2).sum(0, keepdim=True).sqrt() + 1e-10)
    want = float((((na - nb) ** 2) * wv.double().view(c, 1, 1)).sum(0).mean())
    print(f"\nhead {c}: device {got!r} float64 {want!r} |diff| {abs(got - want):.2e}")
    assert abs(got - want) <= 1e-10
    assert float(hip.lpips_head(a.cuda(), a.cuda(), wv.cuda()).item()) == 0.0


# ------------------------------------------------------------------------------------------------ end to end


@pytest.mark.parametrize("h,w,kind", CASES)
def test_lpips_matches_the_float64_network(h, w, kind):
    pred, gt, mask, want = case(h, w, kind)
    got = on_device(state_dict(), pred, gt, mask)
    check(got, want, f"{h}x{w} {kind}", zero={4} | ({0} if mask is not None else set()))


def test_gain_logic_on_a_layer_rescaled_network():
    pred, gt, mask, base = case(40, 52, "none")
    sd = rescaled_state_dict()
    want = yardstick(sd, pred, gt, mask)
    assert np.abs(want - base).max() <= 1e-7  # the float64 value moves only through the 1e-10 term
    check(on_device(sd, pred, gt, mask), want, "rescaled 40x52", zero={4})
    pred, gt, mask, _ = case(37, 50, "random30")
    check(on_device(sd, pred, gt, mask), yardstick(sd, pred, gt, mask), "rescaled 37x50 masked", zero={0, 4})


def test_bits_do_not_depend_on_the_batch_or_the_run():
    bits = lambda a: a.view(np.int64)
    for h, w, kind in ((40, 52, "none"), (37, 50, "random30")):
        pred, gt, mask, _ = case(h, w, kind)
        m3 = None if mask is None else mask[:3]
        first = on_device(state_dict(), pred[:3], gt[:3], m3)
        alone = on_device(state_dict(), pred[1:2], gt[1:2], None if mask is None else mask[1:2])
        again = on_device(state_dict(), pred[:3], gt[:3], m3)
        print(h, w, kind, first, alone, again)
        assert np.array_equal(bits(alone[0:1]), bits(first[1:2]))
        assert np.array_equal(bits(again), bits(first))


def test_the_binding_refuses_cpu_tensors_and_small_frames():
    dl = device_lpips(state_dict())
    with pytest.raises(hip.MnerfError):
        hip.lpips_vgg(torch.rand(1, 400, 3), torch.rand(1, 3, 20, 20), None, dl.weights)
    with pytest.raises(hip.MnerfError):  # 17 rows without a mask: the crop keeps 15
        dl(torch.rand(1, 17 * 40, 3, device="cuda"), torch.rand(1, 3, 17, 40, device="cuda"), None)
    with pytest.raises(hip.MnerfError):
        dl(torch.rand(1, 15 * 40, 3, device="cuda"), torch.rand(1, 3, 15, 40, device="cuda"), torch.zeros(1, 15, 40, dtype=torch.bool, device="cuda"))


# ------------------------------------------------------------------------------------------------ Coach.test_model

LINE = re.compile(r"^dtu_\d{3}_\d: PSNR -?\d+\.\d{4} SSIM -?\d+\.\d{4} LPIPS -?\d+\.\d{4}$")
MEAN = re.compile(r"^mean PSNR -?\d+\.\d{4} SSIM -?\d+\.\d{4} LPIPS -?\d+\.\d{4}$")


def weight_files(tmp_path):
    vgg, lin = state_dict()
    torch.save(vgg, tmp_path / "vgg16.pth")
    torch.save(lin, tmp_path / "lin.pth")
    return str(tmp_path / "vgg16.pth"), str(tmp_path / "lin.pth")


class WithDepth:
    """a test loader whose batches carry a ground-truth depth with holes (DTU): test_model masks with depth == 0"""

    def __init__(self, loader):
        self.loader = loader

    def get_name(self):
        return self.loader.get_name()

    def __iter__(self):
        for i, batch in enumerate(self.loader):
            b, _, _, h, w = batch["images"].shape
            depth = torch.ones(b, h, w)
            depth[:, : h // 3, i::3] = 0.0
            yield dict(batch, depth=depth)


def test_coach_test_model_with_the_switch_on_and_off(tmp_path, monkeypatch):
    from matchnerf_amd import options
    from matchnerf_amd.coach import Coach
    monkeypatch.chdir(tmp_path)
    vgg_path, lin_path = weight_files(tmp_path)
    monkeypatch.setenv("MNERF_LPIPS_VGG16", vgg_path)
    monkeypatch.setenv("MNERF_LPIPS_LIN", lin_path)
    monkeypatch.delenv("MNERF_DEVICE_METRICS", raising=False)
    cmd = options.parse_arguments(["--yaml=test", "--name=switch", "--nerf.sample_intvs=32", "--data_test.llff=", "--data_test.blender=",
                                   "--data_test.tnt=", "--data_test.dtu.img_wh=48,32", "--data_test.dtu.max_len=2"])
    opt = options.set(cmd, verbose=False)
    c = Coach(opt)
    c.build_networks()
    c.restore_checkpoint()
    c.load_dataset()
    c.load_dataset(loaders=[WithDepth(c.test_loaders[0])])
    rows, lines = {}, {}
    real_evaluate, real_tools = c._evaluate, metrics.EvalTools

    def keep_rows(*a, **kw):
        r = real_evaluate(*a, **kw)
        rows["now"] = r
        return r

    def no_tools(*a, **kw):
        raise AssertionError("metrics.EvalTools was constructed on the device path")

    monkeypatch.setattr(c, "_evaluate", keep_rows)
    for switch in ("1", "0"):
        monkeypatch.setenv("MNERF_DEVICE_LPIPS", switch)
        monkeypatch.setattr(metrics, "EvalTools", no_tools if switch == "1" else real_tools)
        c.test_model()
        rows[switch] = rows.pop("now")
        lines[switch] = open(os.path.join(opt.output_path, "test", "0results_dtu.txt")).read().splitlines()
        print(switch, rows[switch], lines[switch])
    for ls in lines.values():
        assert len(ls) == 3 and all(LINE.match(l) for l in ls[:2]) and MEAN.match(ls[2]), ls
    for a, b in zip(lines["1"], lines["0"]):
        assert a.split(" LPIPS")[0] == b.split(" LPIPS")[0]  # PSNR and SSIM text: identical
    assert rows["1"].shape == rows["0"].shape == (2, 5)
    assert np.array_equal(rows["1"][:, :4], rows["0"][:, :4])
    assert np.isfinite(rows["1"][:, 4]).all() and (rows["0"][:, 4] > 0).all()
    assert np.abs(rows["1"][:, 4] - rows["0"][:, 4]).max() <= 1e-5


def test_two_ranks_write_the_one_process_file_with_the_lpips_column(tmp_path):
    """`python test.py --gpu_ids=0,1` (both ranks on the one GPU, gloo) against the one-process run: rank 0's results file, LPIPS
    column included, byte for byte"""
    vgg_path, lin_path = weight_files(tmp_path)
    env = dict(os.environ, MNERF_FORCE_DEVICE="0", MNERF_DIST_BACKEND="gloo", MNERF_LPIPS_VGG16=vgg_path, MNERF_LPIPS_LIN=lin_path)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "MNERF_DIST_INIT_ALWAYS", "MNERF_DEVICE_METRICS", "MNERF_DEVICE_LPIPS"):
        env.pop(k, None)
    args = ["--yaml=test", "--nerf.sample_intvs=16", "--data_test.llff=", "--data_test.blender=", "--data_test.tnt=",
            "--data_test.dtu.img_wh=48,32", "--data_test.dtu.max_len=3", f"--output_root={tmp_path}"]
    files = {}
    for name, extra in (("one", []), ("two", ["--gpu_ids=0,1"])):
        r = subprocess.run(["timeout", "-k", "10", "420", sys.executable, os.path.join(REPO, "test.py")] + args + [f"--name={name}"] + extra,
                           cwd=tmp_path, env=env, capture_output=True, text=True)
        print(r.stdout[-3000:], r.stderr[-3000:])
        assert r.returncode == 0, name
        files[name] = open(tmp_path / name / "test" / "0results_dtu.txt", "rb").read()
    assert files["one"].count(b"\n") == 4 and files["one"].count(b" LPIPS ") == 4 and files["one"].startswith(b"dtu_000_0: PSNR ")
    assert files["two"] == files["one"]
