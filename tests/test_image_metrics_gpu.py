"""csrc/metrics.hip on the GPU: PSNR / SSIM rows of hip.image_metrics against the host's float64 evaluation (metrics.psnr and
metrics.EvalTools fed float64 copies of the same fp32 arrays), the hand-derived SSIM vectors, bit reproducibility, the refusals of
the binding, and Coach.test_model with MNERF_DEVICE_METRICS on and off.

Gates (set by the definition, not by what the kernel gives): kept pixels exact; MSE 1e-12 relative (fp64 sums of at most 15 360
exact fp64 squares in another order: ~1e-14); PSNR 1e-8 dB (4.34 x the MSE's relative error); SSIM 1e-10, the project's gate for
"the same definition in another summation order" (tests/test_datasets.py); 5e-6 against the closed forms, its gate for float32
inputs.

Measured on MI355X: SSIM differs from the host's by at most 4.0e-14 (the flat, bright image at 23 x 37, crop) and by at most 2e-15 on
every other content; MSE by at most 4 units in the last place, PSNR by at most 4e-15 dB; the closed forms are met to 1.2e-8
(constant images: the fp32 rounding of 0.2 and 0.6), 1e-16 and 3e-16; Coach.test_model's two paths differ by 3.6e-15 dB."""
import json
import os
import re
import warnings

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from matchnerf_amd import hip, metrics

pytestmark = pytest.mark.gpu

SHAPES = [(7, 7), (10, 10), (16, 24), (23, 37), (45, 70), (64, 80)]  # one window; crop 8x8; < a tile; odd; across tile edges both ways
CONTENTS = ("noise", "smooth_a", "smooth_b", "near_gt", "flat_bright")
_HOST = {}


def make_images(h, w, seed):
    """-> pred [5,h,w,3], gt [5,h,w,3] float32: the five contents of CONTENTS"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    smooth = lambda a, b, p: 0.5 + 0.4 * np.sin(a * yy[..., None] + b * xx[..., None] + p + np.arange(3))
    gt = [rng.random((h, w, 3)), smooth(0.21, 0.13, 0.0), smooth(0.05, 0.31, 1.0), rng.random((h, w, 3))]
    pred = [rng.random((h, w, 3)), smooth(0.19, 0.15, 0.3), smooth(0.07, 0.29, 0.8), gt[3] + 1e-3 * rng.standard_normal((h, w, 3))]
    base_g, base_p = rng.uniform(0.5, 1.0), rng.uniform(0.5, 1.0)
    gt.append(base_g + 1e-4 * rng.standard_normal((h, w, 3)))  # flat and bright: fp32 window moments lose the variance here
    pred.append(base_p + 1e-4 * rng.standard_normal((h, w, 3)))
    return np.stack(pred).astype(np.float32), np.stack(gt).astype(np.float32)


def make_mask(kind, n, h, w, seed):
    if kind == "none":
        return None
    if kind == "all_false":
        return np.zeros((n, h, w), bool)
    m = np.random.default_rng(seed + 7).random((n, h, w)) < 0.3
    if kind == "one_all_true":
        m[1] = True
    return m


def host_rows(pred, gt, mask):
    """the yardstick: float64 copies of the fp32 arrays through metrics.psnr and EvalTools -> [n, 4] (PSNR, SSIM, MSE, kept)"""
    rows = []
    for i in range(pred.shape[0]):
        p, g = pred[i].astype(np.float64), gt[i].astype(np.float64)
        m = None if mask is None else mask[i]
        tools = metrics.EvalTools()
        tools.set_inputs(p, g, m)
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")  # the mean of no pixel
            ps = metrics.psnr(p, g, m)
            ss = tools.get_metrics(["SSIM"])["SSIM"]
            if m is not None:
                kept = int((~m).sum())
                mse = float(np.mean((p[~m] - g[~m]) ** 2))
            else:
                hc, wc = h_w_crop(p.shape)
                kept = (p.shape[0] - 2 * hc) * (p.shape[1] - 2 * wc)
                mse = float(np.mean((p[hc:-hc, wc:-wc] - g[hc:-hc, wc:-wc]) ** 2))
        rows.append([ps, ss, mse, kept])
    return np.asarray(rows, np.float64)


def h_w_crop(shape):
    return shape[0] // 10, shape[1] // 10


def case(h, w, kind):
    """inputs and the host's rows of one (shape, mask kind), computed once"""
    key = (h, w, kind)
    if key not in _HOST:
        pred, gt = make_images(h, w, seed=h * 100 + w)
        mask = make_mask(kind, pred.shape[0], h, w, seed=h * 100 + w)
        _HOST[key] = (pred, gt, mask, host_rows(pred, gt, mask))
    return _HOST[key]


def device_rows(pred, gt, mask, **kw):
    """pred / gt [n,h,w,3] numpy -> the kernel's rows as numpy [n, 4]"""
    n, h, w, _ = pred.shape
    p = torch.from_numpy(pred).cuda().reshape(n, h * w, 3)
    g = torch.from_numpy(gt).cuda().permute(0, 3, 1, 2).contiguous()
    m = None if mask is None else torch.from_numpy(mask).cuda()
    return hip.image_metrics(p, g, m, **kw).cpu().numpy()


def compare(got, want, what):
    for i, (a, b) in enumerate(zip(got, want)):
        print(f"{what} image {i}: PSNR {a[0]!r} / {b[0]!r}  SSIM {a[1]!r} / {b[1]!r} (diff {abs(a[1] - b[1]):.2e})  "
              f"MSE {a[2]!r} / {b[2]!r}  kept {a[3]} / {b[3]}")
    for i, (a, b) in enumerate(zip(got, want)):
        assert a[3] == b[3], (what, i)
        if b[3] == 0:  # no kept pixel: the host gives NaN, and SSIM 1 of two images of zeros
            assert np.isnan(a[0]) and np.isnan(b[0]) and np.isnan(a[2]) and np.isnan(b[2]), (what, i)
            assert a[1] == 1.0 == b[1], (what, i)
            continue
        assert abs(a[2] - b[2]) <= 1e-12 * abs(b[2]), (what, i)
        assert abs(a[0] - b[0]) <= 1e-8, (what, i)
        assert abs(a[1] - b[1]) <= 1e-10, (what, i)


@pytest.mark.parametrize("h,w", SHAPES)
def test_rows_match_the_float64_host_evaluation(h, w):
    kinds = ["all_false", "random30", "one_all_true"] + (["none"] if min(h, w) >= 10 else [])
    for kind in kinds:
        pred, gt, mask, want = case(h, w, kind)
        compare(device_rows(pred, gt, mask), want, f"{h}x{w} {kind}")
        if mask is not None:  # the mask as uint8 gives the same bits
            n = pred.shape[0]
            got = hip.image_metrics(torch.from_numpy(pred).cuda().reshape(n, h * w, 3), torch.from_numpy(gt).cuda().permute(0, 3, 1, 2).contiguous(),
                                    torch.from_numpy(mask.astype(np.uint8) * 3).cuda()).cpu().numpy()
            assert np.array_equal(got.view(np.int64), device_rows(pred, gt, mask).view(np.int64))


@pytest.mark.parametrize("kind", ["none", "random30"])
def test_gt_as_the_target_view_of_a_batch(kind):
    """gt = images[:, -1] of a [3,4,3,H,W] tensor: contiguous images, a batch stride of four images, no copy"""
    h, w = 23, 37
    pred, gt, mask, want = case(h, w, kind)
    pred, gt, want = pred[:3], gt[:3], want[:3]
    images = torch.full((3, 4, 3, h, w), 9.0, device="cuda")
    images[:, -1] = torch.from_numpy(gt).cuda().permute(0, 3, 1, 2)
    view = images[:, -1]
    assert not view.is_contiguous() and view.stride(0) == 4 * 3 * h * w
    m = None if mask is None else torch.from_numpy(mask[:3]).cuda()
    got = hip.image_metrics(torch.from_numpy(pred).cuda().reshape(3, h * w, 3), view, m).cpu().numpy()
    compare(got, want, f"view {kind}")


def test_hand_derived_vectors():
    g = json.load(open(os.path.join(GOLDEN, "ssim_hand_derived.json")))
    assert len(g["cases"]) == 3
    for c in g["cases"]:
        h, w, ch = c["shape"]
        s = np.where(np.arange(w) % 2 == 0, 1.0, -1.0)[None, :, None]
        if c["kind"] == "constant":
            x, y = np.full((h, w, ch), c["a"]), np.full((h, w, ch), c["b"])
        elif c["kind"] == "stripes":
            x, y = np.broadcast_to(c["m"] + c["amp"] * s, (h, w, ch)), np.broadcast_to(c["m"] - c["amp"] * s, (h, w, ch))
        else:
            x, y = np.broadcast_to(c["m"] + c["amp"] * s, (h, w, ch)), np.broadcast_to(c["m"] + 0.5 * c["amp"] * s, (h, w, ch))
        got = device_rows(np.array(x, np.float32)[None], np.array(y, np.float32)[None], np.zeros((1, h, w), bool))
        print(c["name"], repr(got[0, 1]), c["ssim"], abs(got[0, 1] - c["ssim"]))
        assert abs(got[0, 1] - c["ssim"]) <= 5e-6, c["name"]
        assert got[0, 3] == h * w


def test_bits_do_not_depend_on_the_run_the_batch_or_the_stream():
    h, w = 45, 70
    pred, gt, mask, _ = case(h, w, "random30")
    bits = lambda a: a.view(np.int64)
    for m in (mask, None):
        first = device_rows(pred[:3], gt[:3], None if m is None else m[:3])
        assert np.array_equal(bits(first), bits(device_rows(pred[:3], gt[:3], None if m is None else m[:3])))
        for i in range(3):  # an image alone = the same image inside a batch of 3
            alone = device_rows(pred[i:i + 1], gt[i:i + 1], None if m is None else m[i:i + 1])
            assert np.array_equal(bits(alone[0]), bits(first[i])), i
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            other = device_rows(pred[:3], gt[:3], None if m is None else m[:3], stream=side)
        assert np.array_equal(bits(other), bits(first))


def test_the_binding_refuses_before_any_launch(monkeypatch):
    lib = hip.load()
    calls = []
    monkeypatch.setattr(lib, "mnerf_image_metrics", lambda *a: calls.append(a) or 0)
    h, w = 12, 16
    pred = torch.rand(2, h * w, 3, device="cuda")
    gt = torch.rand(2, 3, h, w, device="cuda")
    mask = torch.zeros(2, h, w, dtype=torch.bool, device="cuda")
    bad = [
        (pred.cpu(), gt.cpu(), None),                                    # CPU tensors
        (pred, gt.cpu(), None),
        (pred.double(), gt.double(), None),                              # a wrong dtype
        (pred.half(), gt, None),
        (torch.rand(2, 9 * w, 3, device="cuda"), torch.rand(2, 3, 9, w, device="cuda"), None),      # H = 9 without a mask
        (torch.rand(2, 6 * w, 3, device="cuda"), torch.rand(2, 3, 6, w, device="cuda"), torch.zeros(2, 6, w, dtype=torch.bool, device="cuda")),
        (pred[:, :-1], gt, None),                                        # pred / gt shapes disagree
        (pred, gt[:1], None),
        (torch.rand(2, 3, h * w, device="cuda").permute(0, 2, 1), gt, None),  # a pred that is not contiguous
        (pred, gt.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2), None),  # images of gt that are not contiguous
        (pred, gt, mask.float()),                                        # a mask of another type
        (pred, gt, mask[:, :-1]),
    ]
    for p, g, m in bad:
        with pytest.raises(hip.MnerfError):
            hip.image_metrics(p, g, m)
    assert calls == []
    hip.image_metrics(pred, gt, mask)  # and the arguments these were derived from pass
    assert len(calls) == 1


# ------------------------------------------------------------------------------------------------ Coach.test_model

LINE = re.compile(r"^dtu_\d{3}_\d: PSNR -?\d+\.\d{4} SSIM -?\d+\.\d{4}$")
MEAN = re.compile(r"^mean PSNR -?\d+\.\d{4} SSIM -?\d+\.\d{4}$")


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


@pytest.mark.parametrize("masked", [False, True], ids=["crop", "depth-mask"])
def test_coach_test_model_with_the_switch_on_and_off(tmp_path, monkeypatch, masked):
    from matchnerf_amd import options
    from matchnerf_amd.coach import Coach
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("MNERF_LPIPS_VGG16", raising=False)
    cmd = options.parse_arguments(["--yaml=test", "--name=switch", "--nerf.sample_intvs=32", "--data_test.llff=", "--data_test.blender=",
                                   "--data_test.tnt=", "--data_test.dtu.img_wh=48,32", "--data_test.dtu.max_len=2"])
    opt = options.set(cmd, verbose=False)
    c = Coach(opt)
    c.build_networks()
    c.restore_checkpoint()
    c.load_dataset()
    if masked:
        c.load_dataset(loaders=[WithDepth(c.test_loaders[0])])
    out = {}
    for switch in ("1", "0"):
        monkeypatch.setenv("MNERF_DEVICE_METRICS", switch)
        assert metrics.device_metrics_enabled() == (switch == "1")
        rep = c.test_model()
        lines = open(os.path.join(opt.output_path, "test", "0results_dtu.txt")).read().splitlines()
        out[switch] = (rep, lines)
        print(switch, rep, lines)
    (dev, dev_lines), (host, host_lines) = out["1"], out["0"]
    assert list(dev) == list(host) == ["dtu"]
    assert list(dev["dtu"]) == list(host["dtu"]) == ["dtu_000_0", "dtu_001_0"]
    for k in dev["dtu"]:
        assert isinstance(dev["dtu"][k], float) and np.isfinite(dev["dtu"][k])
        assert abs(dev["dtu"][k] - host["dtu"][k]) <= 1e-6, k
    for lines in (dev_lines, host_lines):
        assert len(lines) == 3 and all(LINE.match(l) for l in lines[:2]) and MEAN.match(lines[2]), lines
    for a, b in zip(dev_lines, host_lines):
        assert a.split(" PSNR")[0] == b.split(" PSNR")[0]
        # four printed decimals: the difference is a whole number of 1e-4 steps, at most one
        assert round(abs(float(a.rsplit(" ", 1)[1]) - float(b.rsplit(" ", 1)[1])) * 1e4) <= 1, (a, b)
