"""Backward of the backbone / up-sampler convolutions (csrc/conv_backward.hip) against torch's own conv gradients in float64 on the
CPU: every (channels, filter, stride) combination the GMFlow CNN has, odd sizes, borders, bit-reproducibility of the weight gradient."""
import pytest
import torch

import launch_plan_tables as T
from launch_plan_tables import CB_CASES as CASES

pytestmark = pytest.mark.gpu


def _ref(x, w, dy, stride):
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y = torch.nn.functional.conv2d(x64, w64, None, stride, w.shape[2] // 2)
    assert y.shape == dy.shape, (y.shape, dy.shape)
    y.backward(dy.double())
    return x64.grad, w64.grad


@pytest.mark.parametrize("case", CASES)
def test_conv_backward_matches_torch_float64(case):
    from matchnerf_amd import hip
    n, ci, co, h, w, k, s = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(n, ci, h, w, generator=g)
    wt = torch.randn(co, ci, k, k, generator=g) / (ci * k * k) ** 0.5
    ho, wo = (h + 2 * (k // 2) - k) // s + 1, (w + 2 * (k // 2) - k) // s + 1
    # gradients over many binades, as a real loss produces them
    dy = torch.randn(n, co, ho, wo, generator=g) * 2.0 ** torch.randint(-20, -4, (n, co, 1, 1), generator=g).float()
    dx_ref, dw_ref = _ref(x, wt, dy, s)
    dx = hip.conv2d_backward_data(dy.cuda(), wt.cuda(), h, w, s).cpu().double()
    dw = hip.conv2d_backward_weight(x.cuda(), dy.cuda(), k, s).cpu().double()
    assert (dx - dx_ref).abs().max() <= 2e-6 * dx_ref.abs().max(), case
    assert (dw - dw_ref).abs().max() <= 2e-6 * dw_ref.abs().max(), case
    again = hip.conv2d_backward_weight(x.cuda(), dy.cuda(), k, s).cpu().double()
    assert torch.equal(again, dw)


def test_conv_backward_at_the_backbone_shape():
    """layer1's convolution at the DTU shape (3 x 64 x 256 x 320): the weight gradient's chunked reduction over 768 rows"""
    from matchnerf_amd import hip
    assert T.CB_BACKBONE_SHAPE == (3, 64, 64, 256, 320, 3, 1)  # the row of launch_plan_tables that stands for this test
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 64, 256, 320, generator=g).cuda()
    wt = (torch.randn(64, 64, 3, 3, generator=g) / 24.0).cuda()
    dy = (torch.randn(3, 64, 256, 320, generator=g) * 1e-4).cuda()
    dx = hip.conv2d_backward_data(dy, wt, 256, 320, 1)
    dw = hip.conv2d_backward_weight(x, dy, 3, 1)
    ref_dx = torch.nn.grad.conv2d_input(x.shape, wt.double(), dy.double(), 1, 1)
    ref_dw = torch.nn.grad.conv2d_weight(x.double(), wt.shape, dy.double(), 1, 1)
    assert (dx.double() - ref_dx).abs().max() <= 2e-6 * ref_dx.abs().max()
    assert (dw.double() - ref_dw).abs().max() <= 5e-6 * ref_dw.abs().max()


def _gradient_operands(case, seed):
    n, ci, co, h, w, k, s = case
    g = torch.Generator().manual_seed(sum(case) + seed)
    x = torch.randn(n, ci, h, w, generator=g)
    wt = torch.randn(co, ci, k, k, generator=g) / (ci * k * k) ** 0.5
    ho, wo = (h + 2 * (k // 2) - k) // s + 1, (w + 2 * (k // 2) - k) // s + 1
    # gradients over many binades, as a real loss produces them
    dy = torch.randn(n, co, ho, wo, generator=g) * 2.0 ** torch.randint(-20, -4, (n, co, 1, 1), generator=g).float()
    return x, wt, dy


@pytest.mark.parametrize("case", T.flat(T.CB_DATA_NEW))
def test_data_gradient_instances_match_torch_float64(case):
    """conv_gemm_kernel<1,2 | 2,1 | 2,2 | 3,1 | 4,1, FWD = false>: every instance of the data gradient above <1,1>, with the
    filters and strides full frames send to it, at the smallest odd shapes that select it (tests/test_launch_plans.py holds each
    case to its instance).  The gate of test_conv_backward_matches_torch_float64.  Measured on MI355X, |err| / max|ref|:
      (2, 96, 96, 171, 65, 3, 1): 1.19e-06
      (1, 128, 128, 513, 33, 3, 1): 1.64e-06
      (1, 128, 128, 513, 33, 1, 1): 4.74e-07
      (1, 64, 96, 513, 129, 3, 2): 1.24e-06
      (1, 64, 96, 513, 129, 1, 2): 4.21e-07
      (1, 96, 128, 513, 65, 3, 2): 8.50e-07
      (1, 96, 128, 513, 65, 1, 2): 4.25e-07
      (2, 96, 96, 513, 33, 3, 1): 1.63e-06
      (2, 128, 128, 513, 33, 3, 1): 1.42e-06"""
    from matchnerf_amd import hip
    n, ci, co, h, w, k, s = case
    x, wt, dy = _gradient_operands(case, 3)
    ref = torch.nn.grad.conv2d_input(x.shape, wt.double(), dy.double(), s, k // 2)
    dx = hip.conv2d_backward_data(dy.cuda(), wt.cuda(), h, w, s).cpu().double()
    err = float((dx - ref).abs().max() / ref.abs().max())
    print(f"\ndata gradient {case}: {err:.2e}")
    assert dx.shape == ref.shape and err <= 2e-6, case


@pytest.mark.parametrize("case", T.flat(T.CB_FWD_NEW))
def test_forward_f32_instances_match_torch_float64(case):
    """conv_gemm_kernel<..., FWD = true, TAIL>: every instance of the fp32 forward above <1,1>, the TAIL form (a source channel
    count that is no multiple of 8: the 3-channel stem) included.  The gate of test_conv_forward_f32_matches_torch_float64.
    Measured on MI355X, |err| / max|ref|:
      (3, 64, 96, 227, 129, 3, 2): 1.03e-06
      (2, 96, 96, 171, 65, 3, 1): 1.22e-06
      (3, 64, 96, 227, 129, 1, 2): 2.68e-07
      (1, 128, 128, 513, 33, 3, 1): 1.31e-06
      (1, 128, 128, 513, 33, 1, 1): 3.62e-07
      (2, 96, 128, 511, 65, 3, 2): 1.31e-06
      (2, 96, 128, 511, 65, 1, 2): 2.82e-07
      (2, 64, 64, 513, 65, 3, 1): 1.20e-06
      (3, 64, 96, 455, 129, 3, 2): 1.07e-06
      (3, 64, 96, 455, 129, 1, 2): 2.89e-07
      (2, 96, 96, 513, 33, 3, 1): 1.09e-06
      (2, 128, 128, 513, 33, 3, 1): 1.32e-06
      (2, 3, 64, 511, 129, 7, 2): 5.28e-07
      (3, 3, 64, 455, 129, 7, 2): 5.34e-07
      (3, 3, 64, 455, 257, 7, 2): 4.87e-07
      (2, 3, 96, 513, 33, 3, 1): 2.42e-07
      (2, 3, 128, 513, 33, 3, 1): 1.91e-07"""
    from matchnerf_amd import hip
    n, ci, co, h, w, k, s = case
    g = torch.Generator().manual_seed(sum(case) + 4)
    x = torch.randn(n, ci, h, w, generator=g)
    wt = torch.randn(co, ci, k, k, generator=g) / (ci * k * k) ** 0.5
    bias = torch.randn(co, generator=g) if k == 1 else None
    ref = torch.nn.functional.conv2d(x.double(), wt.double(), None if bias is None else bias.double(), s, k // 2)
    y = hip.conv2d_forward_f32(x.cuda(), wt.cuda(), None if bias is None else bias.cuda(), s).cpu().double()
    err = float((y - ref).abs().max() / ref.abs().max())
    print(f"\nforward f32 {case}: {err:.2e}")
    assert y.shape == ref.shape and err <= 2e-6, case


@pytest.mark.parametrize("case", T.CB_WGRAD_CASES)
def test_weight_gradient_chunks_of_several_rows_match_torch_float64(case):
    """conv_wgrad_kernel<K, S> and conv_wgrad16_kernel<K, S> with several dY rows per chunk, a short last chunk and chunks that
    run over an image boundary (cb_chunks: rpc > 1, rows % rpc != 0, ho % rpc != 0) - what the stride-2 layers of a 512 x 640
    training step launch.  The gates of the two older tests (2e-6 exact f32, 1e-5 split fp16), bit-reproducible.  Measured on
    MI355X, |err| / max|ref| (f32, f16x3):
      (2, 128, 128, 61, 37, 3, 1): 1.86e-07, 1.53e-07
      (2, 96, 128, 153, 75, 3, 2): 2.62e-07, 2.09e-07
      (3, 128, 128, 87, 37, 1, 1): 2.30e-07, 1.96e-07
      (3, 96, 128, 229, 75, 1, 2): 2.27e-07, 2.15e-07"""
    from matchnerf_amd import hip
    n, ci, co, h, w, k, s = case
    x, _, dy = _gradient_operands(case, 5)
    x, dy = x.cuda(), dy.cuda()
    ref = torch.nn.grad.conv2d_weight(x.cpu().double(), (co, ci, k, k), dy.cpu().double(), s, k // 2)
    dw = hip.conv2d_backward_weight(x, dy, k, s).cpu().double()
    regs = hip.absmax_regions(2, x.device)
    hip.absmax(x, regs[0]), hip.absmax(dy, regs[1])
    dw16 = hip.conv2d_backward_weight(x, dy, k, s, regs[0], regs[1]).cpu().double()
    e32, e16 = (float((d - ref).abs().max() / ref.abs().max()) for d in (dw, dw16))
    print(f"\nweight gradient {case}: f32 {e32:.2e}, f16x3 {e16:.2e}")
    assert e32 <= 2e-6 and e16 <= 1e-5, (case, e32, e16)
    assert torch.equal(hip.conv2d_backward_weight(x, dy, k, s).cpu().double(), dw)
    assert torch.equal(hip.conv2d_backward_weight(x, dy, k, s, regs[0], regs[1]).cpu().double(), dw16)


def _instance_norm_backward_against_float64(shape, relu, unaligned=False):
    from matchnerf_amd import hip
    g = torch.Generator().manual_seed(sum(shape) + int(relu))
    x = torch.randn(*shape, generator=g) * 3.0 + 0.5
    dy = torch.randn(*shape, generator=g) * 1e-3
    x64 = x.double().requires_grad_(True)
    y = torch.nn.functional.instance_norm(x64)
    if relu:
        y = torch.relu(y)
    y.backward(dy.double())
    xg, dyg = x.cuda(), dy.cuda()
    if unaligned:  # the same values at buffers that start 4 bytes past a 16-byte boundary
        xg, dyg = (torch.cat([t.new_zeros(1), t.reshape(-1)])[1:].view(shape) for t in (xg, dyg))
        assert xg.data_ptr() % 16 == 4 and xg.is_contiguous()
    dx = hip.instance_norm_backward(xg, dyg, relu).cpu().double()
    err = float((dx - x64.grad).abs().max() / x64.grad.abs().max())
    print(f"\ninstance norm backward {shape} relu={relu} unaligned={unaligned}: {err:.2e}")
    assert err <= 1e-5, (shape, relu)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape", T.IN_BWD_OLD)
def test_instance_norm_backward_matches_autograd_float64(shape, relu):
    _instance_norm_backward_against_float64(shape, relu)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("entry", T.IN_BWD_NEW, ids=str)
def test_instance_norm_backward_mid_size_planes_match_autograd_float64(entry, relu):
    """instance_norm_backward_cached_kernel<256, 20>: planes of 8 193 to 20 480 elements (the 128 x 160 planes of the 96-channel
    stage of a 512 x 640 training step) at both ends of the range, and the same size where it must take the streaming kernel: a
    plane that is no multiple of 4 and one in unaligned buffers.  The gate of the test above.  Measured on MI355X:
      (1, 2, 128, 160) relu=False unaligned=False: 1.12e-07
      (1, 2, 128, 160) relu=True unaligned=False: 1.06e-07
      (1, 3, 2, 4098) relu=False unaligned=False: 1.39e-07
      (1, 3, 2, 4098) relu=True unaligned=False: 9.63e-08
      (1, 2, 127, 161) relu=False unaligned=False: 1.00e-07
      (1, 2, 127, 161) relu=True unaligned=False: 1.28e-07
      (1, 2, 128, 160) relu=False unaligned=True: 1.13e-07
      (1, 2, 128, 160) relu=True unaligned=True: 1.06e-07"""
    if entry[0] == "unaligned":
        _instance_norm_backward_against_float64(entry[1], relu, unaligned=True)
    else:
        _instance_norm_backward_against_float64(entry, relu)


@pytest.mark.parametrize("case", CASES + T.CB_STEM_FWD_CASES)
def test_conv_forward_f32_matches_torch_float64(case):
    from matchnerf_amd import hip
    n, ci, co, h, w, k, s = case
    g = torch.Generator().manual_seed(sum(case) + 1)
    x = torch.randn(n, ci, h, w, generator=g)
    wt = torch.randn(co, ci, k, k, generator=g) / (ci * k * k) ** 0.5
    bias = torch.randn(co, generator=g) if k == 1 else None
    ref = torch.nn.functional.conv2d(x.double(), wt.double(), None if bias is None else bias.double(), s, k // 2)
    y = hip.conv2d_forward_f32(x.cuda(), wt.cuda(), None if bias is None else bias.cuda(), s).cpu().double()
    assert y.shape == ref.shape and (y - ref).abs().max() <= 2e-6 * ref.abs().max(), case


@pytest.mark.parametrize("shape", [(2, 30, 44), (1, 17, 23), (3, 64, 80)])
def test_stem_weight_gradient_matches_torch_float64(shape):
    from matchnerf_amd import hip
    n, h, w = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(n, 3, h, w, generator=g)
    dy = torch.randn(n, 64, (h - 1) // 2 + 1, (w - 1) // 2 + 1, generator=g) * 1e-3
    ref = torch.nn.grad.conv2d_weight(x.double(), (64, 3, 7, 7), dy.double(), 2, 3)
    dw = hip.conv_stem_backward_weight(x.cuda(), dy.cuda()).cpu().double()
    assert (dw - ref).abs().max() <= 3e-6 * ref.abs().max(), shape


@pytest.mark.parametrize("case", CASES)
def test_weight_gradient_on_the_16_bit_pipe_matches_torch_float64(case):
    """split-fp16 operands (one gain per tensor from the absmax regions), three products per MAC: 22-bit operands"""
    from matchnerf_amd import hip
    n, ci, co, h, w, k, s = case
    g = torch.Generator().manual_seed(sum(case) + 2)
    x = (torch.randn(n, ci, h, w, generator=g) * 3.0).cuda()
    ho, wo = (h + 2 * (k // 2) - k) // s + 1, (w + 2 * (k // 2) - k) // s + 1
    dy = (torch.randn(n, co, ho, wo, generator=g) * 1e-4).cuda()
    regs = hip.absmax_regions(2, x.device)
    hip.absmax(x, regs[0]), hip.absmax(dy, regs[1])
    ref = torch.nn.grad.conv2d_weight(x.cpu().double(), (co, ci, k, k), dy.cpu().double(), s, k // 2)
    dw = hip.conv2d_backward_weight(x, dy, k, s, regs[0], regs[1]).cpu().double()
    assert (dw - ref).abs().max() <= 1e-5 * ref.abs().max(), case
    assert torch.equal(hip.conv2d_backward_weight(x, dy, k, s, regs[0], regs[1]).cpu().double(), dw)


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 2, 1, 4), (1, 1, 64, 80), (1, 2, 6, 1)])
def test_bilinear_upsampling_and_its_adjoint_match_torch(shape):
    from matchnerf_amd import hip
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(*shape, generator=g)
    add = torch.randn(shape[0], shape[1], 2 * shape[2], 2 * shape[3], generator=g)
    x64 = x.double().requires_grad_(True)
    ref = F.interpolate(x64, scale_factor=2, mode="bilinear", align_corners=False) + add.double()
    out = hip.upsample_bilinear2x(x.cuda(), add.cuda()).cpu().double()
    assert (out - ref.detach()).abs().max() < 1e-6
    gout = torch.randn(ref.shape, generator=g)
    ref.backward(gout.double())
    din = hip.upsample_bilinear2x_backward(gout.cuda()).cpu().double()
    assert (din - x64.grad).abs().max() < 1e-6
