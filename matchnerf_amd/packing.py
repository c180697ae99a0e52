"""Device-side packing of weights into the split-fp16 MFMA operand streams — the training path's twin of the numpy packers
(wstream.pack_units, wstream.pack_wstream_h).  Both evaluate the same descriptions from wstream.py (the recipes' units, the
decoder's stage table), so they are bit-identical by construction; tests/test_wstream_bytes_cpu.py pins the bytes.

Two forms: per stream (`pack_qkv`, `pack_encoder_block`: a handful of device ops per unit) and, what training uses, everything
in one go (`TransformerPacker`, `ConvPacker`: ONE concatenation of all weights, ONE gather through an index built once, the
fp16 split — about ten launches and one device->host copy per optimizer step for all 24 streams of the 12 layers).

Why: the training forward of every transformer layer runs the inference kernels, which read host-packed weight streams cached
on the parameters' `_version`.  After each `optimizer.step()` all 12 layers re-packed on the HOST: `.detach().cpu().numpy()` on
every weight (a blocking device sync each), numpy fragment building for the [1024,256] / [128,1024] FFN weights, a pageable
host->device copy — dozens of syncs per training step that the torch-Linear path did not have (advisor, round 4).  Here a
stream is ONE gather of the weight (index tensor built once per layer shape and kept on the device), a power-of-two scale and
the fp16 hi | lo split, all as device ops on the caller's stream; the only host round trip is the per-tensor scale exponent the
kernels take as an integer argument, and `FeatureTransformer.refresh_packs` fetches the exponents of ALL stale layers with
one device->host copy per step."""
import numpy as np
import torch

from . import wstream as W
from .wstream import exponent_of_absmax, split_f16x2_torch

_INDEX_CACHE = {}        # (unit, tensor shape, device) -> the unit's index tensor
_DECODER_PLAN = {}       # (decoder shape, device) -> the index tensors of DecoderPacker
_TRANSFORMER_INDEX = {}  # (layer kinds, device) -> (int32 index [units, 512], per-layer unit spans)
_CONV_INDEX = {}         # (conv shapes, device) -> (int32 index [units, 512], spans)


def weight_exponents(tensors):
    """Scale exponents of several weight tensors with ONE device->host copy."""
    if not tensors:
        return []
    amax = torch.stack([t.detach().abs().max() for t in tensors]).tolist()
    return [exponent_of_absmax(float(m)) for m in amax]


def _unit_halves(u, w, ew):
    """fp16 [T, nmb, 2, 64, 8] on w's device: unit `u` of the 2-D weight `w` scaled by 2^ew (a host integer)"""
    w = w.detach().to(torch.float32)
    key = (u.cols.shape, u.cols.tobytes(), u.nmb, None if u.rows is None else u.rows.tobytes(), tuple(w.shape), str(w.device))
    if key not in _INDEX_CACHE:
        _INDEX_CACHE[key] = torch.from_numpy(W.unit_index(u, w.shape, pad=w.numel())).to(w.device)
    # exact (a power of two as a host scalar; torch.ldexp goes through pow() on the device)
    flat = torch.cat([(w * float(2.0 ** int(ew))).reshape(-1), w.new_zeros(1)])
    return torch.stack(split_f16x2_torch(flat[_INDEX_CACHE[key]]), 2)


def fragments_h(weight, cols, nmb, ew):
    """Same bits as wstream._fragments_h, on weight's device."""
    return _unit_halves(W.Unit(0, np.asarray(cols), nmb), weight, ew)


def _pack_units(units, tensors, ews):
    """wstream.pack_units on the tensors' device; `ews`: the exponents if the caller already fetched them"""
    if ews is None:
        ews = weight_exponents(tensors)
    halfs = [_unit_halves(u, tensors[u.tensor], ews[u.tensor]).reshape(-1) for u in units]
    return torch.cat(halfs).view(torch.float32), tuple(int(e) for e in ews)


def pack_qkv(wq, wk, wv, ews=None):
    """wstream.pack_qkv on the weights' device -> (wstream float32 words, (ew_q, ew_k, ew_v))."""
    return _pack_units(W.qkv_units([w.shape for w in (wq, wk, wv)]), (wq, wk, wv), ews)


def pack_encoder_block(merge_w, mlp0_w=None, mlp2_w=None, ews=None):
    """wstream.pack_encoder_block on the weights' device -> (wstream float32 words, (ew_merge, ew_w1, ew_w2))."""
    ws = (merge_w,) if mlp0_w is None else (merge_w, mlp0_w, mlp2_w)
    stream, ews = _pack_units(W.encoder_block_units([w.shape for w in ws]), ws, ews)
    return stream, (ews + (0, 0))[:3]


class _GatherPacker:
    """Several recipes' streams from one gather: the index (int32 [units, 512]) maps every fragment element to its position in
    the concatenation of the scaled weight tensors (one trailing zero serves the padding); it depends on the shapes only and is
    built once per device."""

    def _build_index(self, streams):
        """streams: (recipes, tensors) - the recipes (unit lists) that read these tensors, the tensors in concatenation order
        -> (index, (first, last) unit per recipe)"""
        chunks, spans, off, pos = [], [], 0, 0
        for recipes, tensors in streams:
            bases = [off + sum(t.numel() for t in tensors[:i]) for i in range(len(tensors))]
            for units in recipes:
                chunks.append(W.stream_index(units, [t.shape for t in tensors], bases))
                spans.append((pos, pos + chunks[-1].shape[0]))
                pos = spans[-1][1]
            off += sum(t.numel() for t in tensors)
        idx = np.concatenate(chunks, 0)
        idx = np.where(idx < 0, off, idx)  # the zero slot behind the last weight
        assert idx.max() <= off < 2 ** 31
        return torch.from_numpy(idx.astype(np.int32)).to(self.device), spans

    def _gather(self, ts):
        """-> (float32 words [units * 512] of one fresh buffer, the tensors' exponents).  One device->host copy (the exponents)."""
        ews = [exponent_of_absmax(float(m)) for m in torch.stack(torch._foreach_norm(ts, float("inf"))).tolist()]
        scaled = torch._foreach_mul(ts, [float(2.0 ** e) for e in ews])
        flat = torch.cat([t.reshape(-1) for t in scaled] + [ts[0].new_zeros(1)])
        hi, lo = split_f16x2_torch(flat[self.index.long()])           # [units, 512]
        return torch.stack([hi, lo], 1).reshape(-1).view(torch.float32), ews  # [units][hi | lo][512] halves = 512 words per unit


class TransformerPacker(_GatherPacker):
    """All operand streams of a gmflow.FeatureTransformer (12 layers: q|k|v streams + post-attention streams); the index has
    ~3.1 M entries for the shipped 6-block transformer."""

    def __init__(self, ft, device):
        self.device = torch.device(device)
        self.layers = [l for blk in ft.layers for l in (blk.self_attn, blk.cross_attn_ffn)]
        # the index depends on the layers' SHAPES only: shared by every transformer of that shape on the device (nn.DataParallel
        # makes a new replica object per forward; rebuilding 3 M index entries each time would cost half a second)
        sig = (tuple(bool(l.no_ffn) for l in self.layers), str(self.device))
        if sig not in _TRANSFORMER_INDEX:
            streams = []
            for l in self.layers:
                streams += [([W.qkv_units([w.shape for w in l._qkv_params()])], l._qkv_params()),
                            ([W.encoder_block_units([w.shape for w in l._block_weights()])], l._block_weights())]
            _TRANSFORMER_INDEX[sig] = self._build_index(streams)
        self.index, self.spans = _TRANSFORMER_INDEX[sig]

    def matches(self, ft):
        layers = [l for blk in ft.layers for l in (blk.self_attn, blk.cross_attn_ffn)]
        return len(layers) == len(self.layers) and all(a is b for a, b in zip(layers, self.layers))

    def pack(self):
        """-> per layer ((qkv stream, (ew_q, ew_k, ew_v)), (block stream, (ew_merge, ew_w1, ew_w2))); streams are float32-word
        views of one fresh buffer.  One device->host copy (the exponents)."""
        # the parameter OBJECTS are collected again on every pack: a layer whose Parameter was replaced since construction
        # (layer.q_proj.weight = nn.Parameter(...), parametrize, weight tying) must not be packed from the old tensor
        per_stream = [ps for l in self.layers for ps in (l._qkv_params(), l._block_weights())]
        words, ews = self._gather([t.detach() for ps in per_stream for t in ps])
        out, k = [], 0
        for ps, (first, last) in zip(per_stream, self.spans):
            out.append((words[first * 512:last * 512], (tuple(ews[k:k + len(ps)]) + (0, 0))[:3]))
            k += len(ps)
        return list(zip(out[0::2], out[1::2]))


class ConvPacker(_GatherPacker):
    """The split-fp16 weight streams of a list of nn.Conv2d (wstream.conv_units) for the TRAINING path: per convolution the
    forward stream and, for stride-1 convolutions whose data gradient is itself a convolution the forward kernel builds
    (c_in 64 / 96 / 128), the stream of the flipped, transposed filter (wstream.conv_backward_units)."""

    def __init__(self, convs, device):
        self.device = torch.device(device)
        self.convs = list(convs)
        sig = (tuple((c.out_channels, c.in_channels, c.kernel_size[0], c.stride[0]) for c in self.convs), str(self.device))
        if sig not in _CONV_INDEX:
            _CONV_INDEX[sig] = self._build_index(self._streams())
        self.index, self.spans = _CONV_INDEX[sig]

    @staticmethod
    def has_backward_stream(conv):
        return conv.stride[0] == 1 and conv.kernel_size[0] in (1, 3) and conv.in_channels in (64, 96, 128) and conv.out_channels % 32 == 0

    def _streams(self):
        return [([W.conv_units(c.weight.shape)] + ([W.conv_backward_units(c.weight.shape)] if self.has_backward_stream(c) else []),
                 [c.weight]) for c in self.convs]

    def pack(self):
        """-> per convolution (forward stream, backward stream or None, ew): float32-word views of one fresh buffer"""
        words, ews = self._gather([c.weight.detach() for c in self.convs])
        spans, out = iter(self.spans), []
        for c, e in zip(self.convs, ews):
            f, b = next(spans), next(spans) if self.has_backward_stream(c) else None
            out.append((words[f[0] * 512:f[1] * 512], None if b is None else words[b[0] * 512:b[1] * 512], e))
        return out


class DecoderPacker:
    """The conditional-NeRF decoder's split-fp16 weight stream (wstream.pack_wstream_h) assembled on the device, with NO
    device->host copy at all: this stream carries its scale exponents in the stage headers (float [128] = 2^-ew, [129] = ew), so
    they are computed where the weights are (frexp of the tensor's absmax).  Built once per decoder shape: index maps from the
    stage table and schedule the numpy packer reads (every fp32 word of the stream that is not a fragment half is a plain copy
    of one parameter element: the bias headers and the resident tail segment)."""

    def __init__(self, dec, n_views, cos_n_group, L_3D, legacy, device, prefix="nerf_dec."):
        self.device = torch.device(device)
        sd = {prefix + k: v for k, v in dec.state_dict().items()}
        self.names = [k for k in sd if not k.endswith("num_batches_tracked")]
        self._dec_ref, self._prefix = dec, prefix
        self.params = [dict(dec.named_parameters())[k[len(prefix):]] for k in self.names]
        # the plan depends on the decoder's shape only: shared by every decoder of that shape on the device (DataParallel replicas)
        key = (int(n_views), tuple(int(g) for g in cos_n_group), int(L_3D), bool(legacy), str(self.device),
               tuple((k, tuple(p.shape)) for k, p in zip(self.names, self.params)))
        if key not in _DECODER_PLAN:
            _DECODER_PLAN[key] = self._build_plan(n_views, cos_n_group, L_3D, legacy, prefix)
        (self.zero_pos, self.cond_dim, self.cond_stride, self.total, self.frag_src, self.frag_dst, self.frag_tensor, self.word_src,
         self.word_dst, self.hdr_dst, self.hdr_tensor) = _DECODER_PLAN[key]

    def _build_plan(self, n_views, cos_n_group, L_3D, legacy, prefix):
        numels = [p.numel() for p in self.params]
        base = dict(zip(self.names, np.cumsum([0] + numels[:-1]).tolist()))
        shape = {k: tuple(p.shape) for k, p in zip(self.names, self.params)}
        tensor_id = {k: i for i, k in enumerate(self.names)}
        zero_pos = sum(numels)  # flat = cat(params) + [0]
        cond_dim, cond_stride = W.cond_dims(n_views, cos_n_group)
        table = W.decoder_stage_table(cond_dim, L_3D, legacy)
        segs, total = W.decoder_schedule_h(cond_dim, L_3D)
        frag_src, frag_dst, frag_tensor = [], [], []
        word_src, word_dst, hdr_dst, hdr_tensor = [], [], [], []
        frag_cache = {}
        for name, first, steps, m, off_w, fl, hdr in segs:
            if name == "tail":
                continue
            st = table[name]
            wname = prefix + st.weight
            n_out, n_in_total = shape[wname]
            if name not in frag_cache:
                frag_cache[name] = W.fragment_index(st.cols, m, n_out, n_in_total - st.c0 if st.ncols is None else st.ncols,
                                                    flat_of=lambda r, c: r * n_in_total + st.c0 + c, base=base[wname],
                                                    pad=zero_pos).reshape(-1, 512)
            if hdr:
                b = W._bias_index(shape[prefix + st.bias][0], m)[:128]  # (only l5h has no bias, and it has no header)
                word_src.append(np.where(b < 0, zero_pos, base[prefix + st.bias] + b))
                word_dst.append(off_w + np.arange(128))
                hdr_dst.append(off_w + 128)
                hdr_tensor.append(tensor_id[wname])
                off_w += W.FRAG_FLOATS
            units = frag_cache[name][first * m:(first + steps) * m]
            frag_src.append(units)
            frag_dst.append(off_w + 512 * np.arange(units.shape[0])[:, None] + np.arange(512)[None, :])
            frag_tensor.append(np.full(units.shape[0], tensor_id[wname]))
        # the resident tail segment: plain fp32 copies, taken from the numpy packer run on position-valued stand-ins for the
        # parameters (position + 1; 0 = padding)
        assert zero_pos + 1 < 2 ** 24, "position-valued stand-ins must be exact in float32"
        pos_sd = {k: (base[k] + 1 + np.arange(n, dtype=np.float32)).reshape(shape[k]) for k, n in zip(self.names, numels)}
        tail = W.pack_tail(W._reader(pos_sd, prefix, L_3D)).astype(np.int64)
        word_src.append(np.where(tail == 0, zero_pos, tail - 1))
        word_dst.append(segs[-1][4] + np.arange(tail.size))
        assert segs[-1][0] == "tail"
        dev = self.device
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.int64)).to(dev)
        return (zero_pos, cond_dim, cond_stride, total, t(np.concatenate(frag_src, 0)), t(np.concatenate(frag_dst, 0)),
                t(np.concatenate(frag_tensor)), t(np.concatenate(word_src)), t(np.concatenate(word_dst)),
                torch.tensor(hdr_dst, dtype=torch.int64, device=dev), torch.tensor(hdr_tensor, dtype=torch.int64, device=dev))

    def pack(self):
        """-> wstream (float32 words [total]) on the parameters' device; same bits as wstream.pack_wstream_h."""
        # (the Parameter objects are looked up again on every pack: see TransformerPacker.pack)
        named = dict(self._dec_ref.named_parameters())
        self.params = [named[k[len(self._prefix):]] for k in self.names]
        ts = [p.detach().to(torch.float32) for p in self.params]
        amax = torch.stack(torch._foreach_norm(ts, float("inf")))
        # wstream.exponent_of_absmax on the device: the exponents go into the stream and never to the host
        _, e = torch.frexp(amax)
        ew = torch.where((amax == 0) | ~torch.isfinite(amax), torch.zeros_like(e), W.F16_TARGET_EXP - e).to(torch.int32)
        scale = ((ew + 127) << 23).view(torch.float32)          # 2^ew, exact
        inv = ((127 - ew) << 23).view(torch.float32)            # 2^-ew
        flat = torch.cat([t.reshape(-1) for t in ts] + [amax.new_zeros(1)])
        hi, lo = split_f16x2_torch(flat[self.frag_src] * scale[self.frag_tensor][:, None])
        out = flat.new_zeros(self.total)
        out[self.frag_dst.reshape(-1)] = torch.stack([hi, lo], 1).reshape(-1).view(torch.float32)
        out[self.word_dst] = flat[self.word_src]
        out[self.hdr_dst] = inv[self.hdr_tensor]
        out[self.hdr_dst + 1] = ew[self.hdr_tensor].to(torch.float32)
        return out
