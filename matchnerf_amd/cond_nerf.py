"""CondNeRF — the conditional radiance-field decoder of MatchNeRF, MI355X-native.

Host-side mirror of /root/reference/models/rfdecoder/cond_nerf.py:8-50 (+ nerf.py,
ray_transformer.py): the module owns the same parameters under the same ``state_dict`` keys
(binding for checkpoint drop-in), but it does not evaluate them with
torch ops.  ``pack_wstream_h`` / ``pack_wstream16`` / ``pack_wstream`` re-lay the weights out as the MFMA
A-fragment stream consumed by the fused HIP kernel (csrc/decoder.hip) and the evaluation itself happens in
``libmnerf_hip.so`` (``mnerf_decoder_chunk`` / ``mnerf_decoder_samples`` / ``mnerf_render_chunk``).

The stream layouts and their packers live in wstream.py (also DESIGN.md §5); their names stay importable from here.
"""
import torch
import torch.nn as nn

from .wstream import (  # noqa: F401  (re-exported: the decoder's packers, schedules and layout constants)
    BIAS, F16_TARGET_EXP, FRAG_FLOATS, H_SEG_STEPS, SEG_CAP_FLOATS, SMALL_FIXED, TAIL_FLOATS, TAIL_LAYOUT, WSTREAM_FORMATS, ZERO,
    _bias_fragment, _enc_cols, _enc_cols16, _fragments, _fragments16, _fragments_h, _reg_cols16, _reg_order, bf16_round, bf16_to_f32,
    decoder_schedule, decoder_schedule16, decoder_schedule_h, decoder_stages, decoder_stages16, decoder_stages_h,
    f16_weight_exponent, pack_for_math, pack_key, pack_small, pack_wstream, pack_wstream16, pack_wstream_h, raytrans_table,
    split_bf16x3, split_f16x2)


def decoder_math():
    """Matrix arithmetic of the fused decoder, chosen with MNERF_DECODER_MATH:
    'f16x3' (default) fp32 operands as two range-managed fp16 terms, three products per MAC on the fp16 MFMA;
    'bf16x6' fp32 operands as three bf16 terms, six products per MAC (strict: error of an fp32 FMA chain);
    'f32' the exact-f32 MFMA;
    'f16' (opt-in FAST mode, reduced precision: outside the 1e-4 parity gate) the f16x3 stream read as plain fp16 weights, one
    product per MAC on fp16 activations with per-sample gains, fp32 accumulation (ping-pong decoder only)."""
    import os
    m = os.environ.get("MNERF_DECODER_MATH", "f16x3")
    if m not in WSTREAM_FORMATS:
        raise ValueError(f"MNERF_DECODER_MATH={m!r}: expected one of {sorted(WSTREAM_FORMATS)}")
    return m


# ----------------------------------------------------------------------------- module


class _RayAttentionParams(nn.Module):
    """Parameter holder with the keys of MultiHeadAttention(4, 16, 4, 4)
    (ray_transformer.py:32-47); evaluated inside csrc/decoder.hip."""

    def __init__(self):
        super().__init__()
        self.w_qs = nn.Linear(16, 16, bias=False)
        self.w_ks = nn.Linear(16, 16, bias=False)
        self.w_vs = nn.Linear(16, 16, bias=False)
        self.fc = nn.Linear(16, 16, bias=False)
        self.layer_norm = nn.LayerNorm(16, eps=1e-6)


class CondNeRF(nn.Module):
    """Same constructor contract and parameter names as the reference's CondNeRF
    (cond_nerf.py:11-50).  ``forward`` keeps the reference signature and runs the fused HIP decoder on
    caller-supplied sample coordinates (``mnerf_decoder_samples``); ``MatchNeRF.render`` uses the ray-chunk form
    that also rebuilds the rays and composites in-kernel.  ``composite`` keeps the reference signature
    (nerf.py:101) and runs the K5 HIP kernel."""

    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        dec, nerf = opt.decoder, opt.nerf
        W, D = dec.net_width, dec.net_depth
        skip = list(dec.skip)
        if not nerf.view_dep:
            raise NotImplementedError("nerf.view_dep=false is unusable in the reference as well "
                                      "(cond_nerf.py:47-50 references views_linears unconditionally)")
        if W != 128 or D != 6 or skip != [4]:
            raise NotImplementedError(
                f"fused decoder kernel is built for net_width=128, net_depth=6, skip=[4] "
                f"(configs/base.yaml:30-32); got {W}, {D}, {skip}")
        L_3D = dec.posenc.L_3D if dec.posenc else 0
        L_view = dec.posenc.L_view if dec.posenc else 0
        if L_view != 0:
            raise NotImplementedError("decoder.posenc.L_view > 0 is not built (base.yaml:35 uses 0)")
        if dec.raytrans_act not in ("ReLU", "ELU"):
            raise NotImplementedError(f"decoder.raytrans_act={dec.raytrans_act}")
        self.L_3D = L_3D
        d3 = 3 + 6 * L_3D
        self.cond_dim = int(sum(opt.encoder.cos_n_group)) + opt.n_src_views * 4
        self.pts_linears = nn.ModuleList(
            [nn.Linear(d3, W)] + [nn.Linear(W + d3, W) if i in skip else nn.Linear(W, W) for i in range(D - 1)])
        self.pts_bias = nn.Linear(self.cond_dim, W)
        act = getattr(nn, dec.raytrans_act)
        self.views_linears = nn.ModuleList([nn.Linear(3 + W, W // 2)])
        self.alpha_linear = nn.Sequential(nn.Linear(W, 16), act())
        self.ray_attention = _RayAttentionParams()
        self.out_alpha_linear = nn.Sequential(nn.Linear(16, 16), act(), nn.Linear(16, 1), nn.ReLU())
        self.feature_linear = nn.Linear(W, W)
        self.rgb_linear = nn.Linear(W // 2, 3)
        for m in [*self.pts_linears, *self.views_linears, self.feature_linear, self.alpha_linear[0], self.rgb_linear]:
            nn.init.kaiming_normal_(m.weight.data)   # cond_nerf.py:102-106
            nn.init.zeros_(m.bias.data)
        self._packed = None  # (key, wstream, small)

    # -- packing cache -----------------------------------------------------------------
    def _pack_key(self, n_samples):
        return pack_key(list(self.parameters()), n_samples, bool(self.opt.decoder.raytrans_posenc),
                        bool(self.opt.nerf.legacy_coord), self.math_for(n_samples, self._training_now()))

    def _training_now(self):
        return torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())

    def math_for(self, n_samples, training=False):
        """the matrix path the kernel runs for S samples per ray (MNERF_DECODER_MATH).  f16x3 / bf16x6 / f32 exist for every
        S <= 256.  The one-product fast mode "f16" exists in the ping-pong decoder at S <= 128 only and has no backward of its
        own (mnerf_decoder_backward re-evaluates the forward in fp32: gradients of another function), so a request for it falls
        back to the parity path f16x3 - with one warning - for longer rays and under autograd, instead of failing with
        MNERF_E_UNSUPPORTED deep inside a launch."""
        math = decoder_math()
        if math == "f16" and (n_samples > 128 or training):
            if not getattr(self, "_warned_f16", False):
                import warnings
                warnings.warn(f"MNERF_DECODER_MATH=f16 (one-product fast mode) does not exist for "
                              f"{'training' if training else f'sample_intvs={n_samples} > 128'}: using f16x3")
                self._warned_f16 = True
            return "f16x3"
        return math

    def packed(self, n_samples, device):
        """(wstream, small, cond_stride, wstream_format) for the HIP kernel; re-packed when any
        parameter changed (load_state_dict / optimizer step), S or MNERF_DECODER_MATH changed."""
        key = self._pack_key(n_samples)
        if self._packed is None or self._packed[0] != key or self._packed[1].device != torch.device(device):
            math = self.math_for(n_samples, self._training_now())
            if math in ("f16x3", "f16") and self.pts_bias.weight.is_cuda and self.pts_bias.weight.device == torch.device(device):
                # parameters on the GPU (every training iteration re-packs after the optimizer step): the stream is assembled
                # THERE, without a device->host copy (packing.DecoderPacker, bit-identical to pack_wstream_h)
                self._packed = (key,) + self._packed_on_device(n_samples, torch.device(device)) + (WSTREAM_FORMATS[math],)
                return self._packed[1], self._packed[2], self._packed[3], self._packed[4]
            sd = {"nerf_dec." + k: v for k, v in self.state_dict().items()}
            ws, cond_dim, cond_stride = pack_for_math(math)(sd, self.opt.n_src_views, list(self.opt.encoder.cos_n_group),
                                                            self.L_3D, bool(self.opt.nerf.legacy_coord))
            assert cond_dim == self.cond_dim
            limit = 64 if math == "f32" else 96  # MNERF_COND_STRIDE_MAX_F32 / MNERF_COND_STRIDE_MAX
            if cond_stride > limit:
                raise NotImplementedError(
                    f"cond_dim={cond_dim} (n_src_views={self.opt.n_src_views}) needs {cond_stride} floats per sample; "
                    f"the {math} decoder stream supports {limit}")
            small = pack_small(sd, n_samples, bool(self.opt.decoder.raytrans_posenc))
            self._packed = (key, torch.from_numpy(ws).to(device), torch.from_numpy(small).to(device), cond_stride,
                            WSTREAM_FORMATS[math])
        return self._packed[1], self._packed[2], self._packed[3], self._packed[4]

    def _packed_on_device(self, n_samples, device):
        from . import packing
        legacy = bool(self.opt.nerf.legacy_coord)
        pkey = (self.opt.n_src_views, tuple(self.opt.encoder.cos_n_group), self.L_3D, legacy, str(device))
        if getattr(self, "_packer", None) is None or self._packer[0] != pkey:
            self._packer = (pkey, packing.DecoderPacker(self, self.opt.n_src_views, list(self.opt.encoder.cos_n_group), self.L_3D,
                                                        legacy, device), {})
        _, pk, tables = self._packer
        assert pk.cond_dim == self.cond_dim
        if pk.cond_stride > 96:  # MNERF_COND_STRIDE_MAX
            raise NotImplementedError(f"cond_dim={pk.cond_dim} (n_src_views={self.opt.n_src_views}) needs {pk.cond_stride} floats "
                                      f"per sample; the f16x3 decoder stream supports 96")
        ln = self.ray_attention.layer_norm
        parts = [ln.weight.detach().float().reshape(-1), ln.bias.detach().float().reshape(-1)]
        if bool(self.opt.decoder.raytrans_posenc):
            if n_samples not in tables:
                tables[n_samples] = torch.from_numpy(raytrans_table(n_samples).reshape(-1)).to(device)
            parts.append(tables[n_samples])
        return pk.pack(), torch.cat(parts), pk.cond_stride

    def decoder_struct(self, n_samples, device, setbg_opaque=False):
        """C-ABI ``mnerf_decoder`` for S samples per ray (the packed tensors stay cached on the module)."""
        from . import hip
        ws, small, cond_stride, wfmt = self.packed(n_samples, device)
        d = hip.Decoder()
        d.wstream, d.wstream_floats, d.small_ = ws.data_ptr(), ws.numel(), small.data_ptr()
        d.n_views, d.cond_dim, d.cond_stride = self.opt.n_src_views, self.cond_dim, cond_stride
        d.wstream_format = wfmt
        d.L_3D = self.L_3D
        dec, nerf = self.opt.decoder, self.opt.nerf
        d.raytrans_posenc, d.raytrans_elu = int(bool(dec.raytrans_posenc)), int(dec.raytrans_act == "ELU")
        d.density_maskfill, d.wo_render_interval = int(bool(dec.density_maskfill)), int(bool(nerf.wo_render_interval))
        d.setbg_opaque = int(bool(setbg_opaque))
        return d

    def forward(self, opt, points_3D, ray_unit=None, cond_info=None, mode=None):
        """cond_nerf.py:52-100 with the reference's signature: points_3D [B,R,S,3] (coordinates w.r.t. source view
        0), ray_unit [B,R,S,3] (or [B,R,3]), cond_info = dict(feat_info, color_info, mask_info) [B,R,S,*]
        -> rgb [B,R,S,3], density [B,R,S].  One launch of the fused HIP decoder per batch element
        (mnerf_decoder_samples): no eager op chain, no autograd (training goes through MatchNeRF.render)."""
        from . import hip
        if ray_unit is None or cond_info is None:
            raise ValueError("CondNeRF.forward needs ray_unit and cond_info (nerf.view_dep is always true here)")
        if not points_3D.is_cuda:
            raise RuntimeError("CondNeRF.forward: the HIP decoder needs CUDA tensors (no CPU fallback)")
        b, r, s, _ = points_3D.shape
        dev = points_3D.device
        dec = self.decoder_struct(s, dev)
        if ray_unit.dim() == 3:
            ray_unit = ray_unit[:, :, None, :].expand(b, r, s, 3)
        cond = torch.zeros(b, r * s, dec.cond_stride, device=dev)
        c = torch.cat([cond_info["feat_info"], cond_info["color_info"], cond_info["mask_info"]], -1)
        if c.shape[-1] != self.cond_dim:
            raise ValueError(f"cond_info has {c.shape[-1]} channels, the decoder was built for {self.cond_dim}")
        cond[..., :self.cond_dim] = c.reshape(b, r * s, self.cond_dim).float()
        cond[..., self.cond_dim] = 1.0
        rgb, sigma = [], []
        with torch.no_grad():
            for i in range(b):
                o = hip.decoder_samples(dec, points_3D[i].float().contiguous(), ray_unit[i].float().contiguous(), cond[i],
                                        legacy_coord=bool(opt.nerf.legacy_coord))
                rgb.append(o[0])
                sigma.append(o[1])
        return torch.stack(rgb, 0), torch.stack(sigma, 0)

    def composite(self, opt, ray, rgb_samples, density_samples, depth_samples, setbg_opaque):
        """nerf.py:101-124 with the reference signature; tensors [B,R,S,*] on the GPU -> rgb [B,R,3], depth [B,R,1],
        opacity [B,R,1], prob [B,R,S,1]."""
        from . import hip
        b, r, s = density_samples.shape
        ray_len = None if opt.nerf.wo_render_interval else ray.norm(dim=-1).reshape(b * r).contiguous()
        rgb, depth, opacity, prob = hip.composite(
            rgb_samples.reshape(b * r, s, 3).contiguous(), density_samples.reshape(b * r, s).contiguous(),
            depth_samples.reshape(b * r, s).contiguous(), ray_len,
            wo_render_interval=bool(opt.nerf.wo_render_interval), setbg_opaque=bool(setbg_opaque), want_prob=True)
        return rgb.reshape(b, r, 3), depth.reshape(b, r, 1), opacity.reshape(b, r, 1), prob.reshape(b, r, s, 1)
