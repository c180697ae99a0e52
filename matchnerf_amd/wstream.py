"""Weight streams: how every matrix kernel of the library reads its weights, written once.

One rule.  A kernel evaluates a Linear ``y = W x`` transposed on the MFMA and reads ``W`` as a stream of A-operand
fragments: element ``(step t, 32-row block m, lane, j)`` holds ``W[32 m + lane % 32, cols[t, lane // 32, j]]``, zero outside
``W`` or where ``cols < 0`` (``fragment_index``).  ``cols [T, 2, J]`` is the column map: which input feature the lower / upper
half-wave feeds at K-step ``t`` (J = 8 for the 16-wide K-steps of the split formats, J = 1 for the exact-f32 MFMA).
Everything else in this file says which tensor, which rows and which column map make up a stream:

* the decoder's stages (``decoder_stage_table``) and their cut into segments (``decoder_schedule*``) for the three decoder
  formats ``pack_wstream`` (f32), ``pack_wstream16`` (split-bf16), ``pack_wstream_h`` (split-fp16, default);
* the recipes — lists of ``Unit`` — of the q|k|v, encoder-block and convolution streams.  The numpy packers here
  (``pack_units``), the per-stream device packers and the one-gather packers of packing.py evaluate the same lists.

Decoder stream layouts (also DESIGN.md §5)
------------------------------------------
f32 format: ``v_mfma_f32_32x32x2_f32``; for K-step ``t`` and output block ``m`` the wave needs one float per lane,
``A[t][lane][m] = W[m*32 + lane % 32][col(t, lane // 32)]``:

* hidden activations arrive in accumulator-register order: step ``t = 16*mb + r`` pairs
  features ``32*mb + (r & 3) + 8*(r >> 2)`` (lower half) and that ``+ 4`` (upper half);
* positional encoding: step ``t = 3*l + c`` pairs ``sin(2^l x_c)`` and ``cos(2^l x_c)``;
  the two trailing steps carry ``(x | y)`` and ``(z | 1)``;
* conditioning vector: step ``t`` pairs ``cond[t]`` and ``cond[stride/2 + t]``;
* a bias is one more column multiplied by the constant 1 operand.

Stages in consumption order (steps x output blocks):
FiLM(stride/2 x4) L0(3L+2 x4) L1..L4(65 x4) L5-enc(3L+2 x4) L5-h(64 x4) feature(65 x4)
views(66 x2) rgb(33 x1) alpha(65 x1) and a "tail" = [qkv(8 x2) | fc(8 x1) | out_alpha.0(9 x1) |
out_alpha.2(9 x1)] — the ray-transformer projections and the density head, which stay resident
in LDS across the attention phase.  Each stage is cut into segments of at most 33 KiB, each
segment padded to a multiple of 256 floats (1 KiB DMA pieces); the tail is one segment.

Format 1 ("bf16x6"): the same transposed MFMA chain on v_mfma_f32_32x32x16_bf16.  Every fp32
weight is split into three bf16 terms w = hi + mid + lo (24 significand bits, exact), the kernel
splits the activations the same way on the fly, and a product is accumulated in fp32 from the six
terms hi.hi, hi.mid, mid.hi, hi.lo, lo.hi, mid.mid (dropped terms < 2^-24 relative): fp32-grade
results (measured: max error BELOW an fp32 FMA chain's) at 16/6 of the f32 matrix rate.
A K-step covers 16 inputs: lane (n, half) supplies k = 8*half + j, j < 8.  With activations in
accumulator-register order, step t of a 16-register block takes registers 8*(t&1)+j, i.e. feature
32*blk + (reg&3) + 8*(reg>>2) + 4*half — again no transposes between layers.
Stream unit = 1 KiB fragment (64 lanes x 8 bf16).  Per (step, block): [hi | mid | lo] fragments.
The first segment of a stage starts with a 1 KiB fp32 BIAS fragment, bias[(half*4 + m)*16 + r],
which the kernel loads as the initial accumulator value (so biases stay exact fp32).

Format 2 ("f16x3", default): the same chain on v_mfma_f32_32x32x16_f16 with TWO fp16 terms per operand and THREE products
per MAC (hi.hi + hi.lo + lo.hi; the dropped lo.lo is < 2^-22 of the product) - half the matrix work and ~half the
operand-split VALU work of bf16x6.  fp16 has 11 significand bits but only a 5-bit exponent, so both operands are
range-managed with exact power-of-two scales:
  * weights: one scale 2^ew per weight TENSOR chosen on the host so that max|W| lands in [2^13, 2^14);
    hi = f16(W 2^ew), lo = f16(W 2^ew - hi) (round-to-nearest; residual exact in fp32).  2^-ew travels in the stage header;
  * activations: one scale per SAMPLE and stage chosen in the kernel from the running maximum of the sample's 128 features
    (in-lane max + one cross-half shuffle) so that the largest operand lands in [2^14, 2^15).
The accumulator then holds 2^ew * g * (W x) and the layer epilogue multiplies the exact inverse back in.
Error per product <= ~2^-22 relative (fp32 chain: 2^-24 per rounding); elements more than 2^17 below the sample's largest
feature lose their lo term to fp16 underflow, an absolute error below 2^-25 of that maximum.
Stream unit = (K16-step, block): [hi | lo] fragments of 1 KiB (64 lanes x 8 fp16), same (lane, j) -> k map as format 1.  A
stage's first segment starts with a 1 KiB fp32 header: floats [0,128) = bias in accumulator order (UNscaled; the kernel
multiplies it by the operand gain), float [128] = 2^-ew, float [129] = ew.  The q|k|v, encoder-block and convolution
streams are sequences of the same unit; their kernels take ew as an integer argument.
"""
from collections import namedtuple

import numpy as np
import torch

from . import hip

SEG_CAP_FLOATS = 33 * 256
FRAG_FLOATS = 256
SMALL_FIXED = hip.SMALL_FIXED  # floats of the `small` block before the ray-posenc table: LayerNorm weight | bias
# sub-stages of the tail segment: name -> (float offset in segment, K-steps, output blocks)
TAIL_LAYOUT = {"qkv": (0, 8, 2), "fco": (1024, 8, 1), "oa0": (1536, 9, 1), "oa2": (2112, 9, 1)}
TAIL_FLOATS = 2688
TAIL_SEG_FLOATS = ((TAIL_FLOATS + 255) // 256) * 256
F16_TARGET_EXP = 14  # weights: max |W 2^ew| in [2^13, 2^14); activations: max in [2^14, 2^15)
H_SEG_STEPS = 4      # K16-steps per segment of a 4-block stage: 4 x 4 x 2 KiB + 1 KiB header = 33 KiB
WSTREAM_FORMATS = {"f32": hip.WSTREAM_F32, "bf16x6": hip.WSTREAM_BF16X3, "f16x3": hip.WSTREAM_F16X2, "f16": hip.WSTREAM_F16X1}
EB_SEG_FLOATS = 32 * 256  # one weight segment of the encoder block kernel: 4 K16-steps x 4 blocks x [hi | lo] x 1 KiB
EB_CHUNK = 128            # hidden units of the FFN produced and consumed at a time


# ----------------------------------------------------------------------------- small helpers


def as_f32(v):
    """tensor or array -> float32 numpy array on the host"""
    return np.asarray(v.detach().cpu().numpy() if torch.is_tensor(v) else v, np.float32)


def pack_key(params, *extra):
    """Cache key of anything packed from `params`: changes with an in-place update (optimizer step, load_state_dict), with a
    re-allocation and with `extra` (the device, ...)."""
    return (tuple(int(p._version) for p in params), tuple(int(p.data_ptr()) for p in params)) + extra


def exponent_of_absmax(m):
    """ew such that m * 2^ew is in [2^(F16_TARGET_EXP-1), 2^F16_TARGET_EXP); 0 for zero / non-finite.  (The decoder's device
    packer, packing.DecoderPacker.pack, restates this rule with torch.frexp: its exponents must not leave the device.)"""
    if m == 0.0 or not np.isfinite(m):
        return 0
    return int(F16_TARGET_EXP - np.frexp(np.float32(m))[1])


def f16_weight_exponent(w):
    """exponent_of_absmax of max|w|  (0 for an empty or all-zero tensor)"""
    return exponent_of_absmax(float(np.max(np.abs(w))) if w.size else 0.0)


def split_f16x2(x):
    """fp32 -> (hi, lo) fp16 with hi + lo ~= x to 22 bits (round to nearest; the residual is exact in fp32)."""
    x = np.ascontiguousarray(x, np.float32)
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def split_f16x2_torch(x):
    """split_f16x2 as torch ops on x's device"""
    hi = x.to(torch.float16)
    return hi, (x - hi.to(torch.float32)).to(torch.float16)


def bf16_round(x):
    """float32 array -> bf16 bit patterns (uint16), round to nearest even."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_to_f32(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


def split_bf16x3(w):
    """fp32 -> (hi, mid, lo) bf16 bit patterns with hi + mid + lo == w (to 24 bits)."""
    w = np.ascontiguousarray(w, np.float32)
    hi = bf16_round(w)
    r1 = w - bf16_to_f32(hi)
    mid = bf16_round(r1)
    r2 = r1 - bf16_to_f32(mid)
    return hi, mid, bf16_round(r2)


def _with_zero(a):
    """`a` flattened with one trailing zero: position a.size serves every padding element of a gather"""
    return np.append(np.ascontiguousarray(a, np.float32).reshape(-1), np.float32(0))


# ----------------------------------------------------------------------------- the fragment index


def fragment_index(cols, nmb, n_rows, n_cols, rows=None, flat_of=None, base=0, pad=-1):
    """int64 [T, nmb, 64, J]: where fragment element (t, m, lane, j) = W[rows[32 m + lane % 32], cols[t, lane // 32, j]] lies,
    as ``base + row * n_cols + col`` in a row-major [*, n_cols] matrix or as ``base + flat_of(row, col)`` (a view of other
    storage, e.g. a convolution filter; a negative result marks padding).  `pad` where the stream row is >= n_rows or the
    column is negative or >= n_cols.  `rows` maps stream rows to matrix rows (a permutation, a chunk of rows)."""
    cols = np.asarray(cols)
    t_n, _, j_n = cols.shape
    # lane = 32 half + n: the half picks the column, n the row - computed per (half, n), never per lane and step
    col = cols[:, None, :, None, :]                                                   # [T, 1, 2, 1, J]
    row = (32 * np.arange(nmb)[:, None] + np.arange(32))[None, :, None, :, None]       # [1, nmb, 1, 32, 1]
    ok_r, ok_c = row < n_rows, (col >= 0) & (col < n_cols)
    row, col = np.where(ok_r, row, 0), np.where(ok_c, col, 0)
    if rows is not None:
        row = np.asarray(rows)[row]
    if flat_of is None and ok_r.all() and ok_c.all():
        return (base + row * n_cols + col).reshape(t_n, nmb, 64, j_n)
    flat = row * n_cols + col if flat_of is None else flat_of(row, col)
    return np.where(ok_r & ok_c & (flat >= 0), base + flat, pad).reshape(t_n, nmb, 64, j_n)


# ----------------------------------------------------------------------------- column maps

BIAS, ZERO = -1, -2  # f32 format: the bias column of [W | bias]; no column (both are padding in the split formats)
NATURAL = np.arange(128).reshape(8, 2, 8)  # K16-step t, half h, j -> feature 16 t + 8 h + j


def _reg_order(n_blocks):
    """input feature fed by (lower, upper) half-wave at step t when the operand is a previous
    layer's accumulator (C/D layout of v_mfma_f32_32x32x2_f32)."""
    lo, hi = [], []
    for mb in range(n_blocks):
        for r in range(16):
            f = 32 * mb + (r & 3) + 8 * (r >> 2)
            lo.append(f)
            hi.append(f + 4)
    return lo, hi


def _enc_cols(L, legacy, base=0):
    """columns of the positional-encoding part of a weight matrix per step.
    legacy layout  [x(3) | sin(l-major,c) (3L) | cos (3L)]      (cond_nerf.py:108-116)
    regular layout [x(3) | per c: sin(l=0..L-1), cos(l=0..L-1)] (nerf.py:126-133)"""
    lo, hi = [], []
    for t in range(3 * L):
        l, c = divmod(t, 3)
        if legacy:
            lo.append(base + 3 + t)
            hi.append(base + 3 + 3 * L + t)
        else:
            lo.append(base + 3 + c * 2 * L + l)
            hi.append(base + 3 + c * 2 * L + L + l)
    lo += [base + 0, base + 2]
    hi += [base + 1, BIAS]
    return lo, hi


def _cols2(lo, hi):
    """(lower, upper) column lists of the f32 format -> column map [T, 2, 1]"""
    return np.stack([np.asarray(lo, np.int64), np.asarray(hi, np.int64)], 1)[:, :, None]


def _reg_cols16(n_blocks):
    """[T=2*n_blocks, 2, 8] input feature per (step, half, j) for accumulator-order operands."""
    t, h, j = np.meshgrid(np.arange(2 * n_blocks), np.arange(2), np.arange(8), indexing="ij")
    reg = 8 * (t & 1) + j
    return 32 * (t >> 1) + (reg & 3) + 8 * (reg >> 2) + 4 * h


def _enc_cols16(L, legacy):
    """positional-encoding slots a = 8t + j: (sin | cos) of argument a, then (x | y), (z | -)."""
    lo, hi = _enc_cols(L, legacy)
    te = (len(lo) + 7) // 8
    cols = np.full((te, 2, 8), ZERO, np.int64)
    for a in range(len(lo)):
        cols[a // 8, 0, a % 8] = lo[a]
        cols[a // 8, 1, a % 8] = ZERO if hi[a] == BIAS else hi[a]
    return cols


def _bias_index(n, nmb):
    """int64 [FRAG_FLOATS]: the bias element at each float of a stage header, accumulator order bias[(half*4 + m)*16 + r]
    (-1: none)"""
    h, m, r = np.meshgrid(np.arange(2), np.arange(nmb), np.arange(16), indexing="ij")
    f = 32 * m + (r & 3) + 8 * (r >> 2) + 4 * h
    idx = np.full(FRAG_FLOATS, -1, np.int64)
    idx[((h * 4 + m) * 16 + r).reshape(-1)] = np.where(f < n, f, -1).reshape(-1)
    return idx


def _bias_fragment(bias, nmb):
    if bias is None:
        return np.zeros(FRAG_FLOATS, np.float32)
    idx = _bias_index(bias.shape[0], nmb)
    return _with_zero(bias)[np.where(idx < 0, bias.shape[0], idx)]


def _k_row_order():
    """Row permutation of Wk for ``mnerf_qkv_projection`` / ``mnerf_qkv_window_images``: accumulator row 32 m + n of the
    transposed chain is register r = (n & 3) + 4 (n >> 3) of lane half (n >> 2) & 1; it is given output channel
    16 t + 8 half + j with 8 t + j = 16 m + r, so that a lane's registers 8t..8t+7 are the eight channels it supplies to
    K16-step t of the attention's S^T = K Q^T."""
    rows = np.zeros(128, np.int64)
    for m in range(4):
        for n in range(32):
            r, half = (n & 3) + 4 * (n >> 3), (n >> 2) & 1
            q = 16 * m + r
            rows[32 * m + n] = 16 * (q >> 3) + 8 * half + (q & 7)
    assert sorted(rows.tolist()) == list(range(128))
    return rows


K_ROW_ORDER = _k_row_order()


# ----------------------------------------------------------------------------- decoder: stages and schedules

Stage = namedtuple("Stage", "weight c0 ncols bias cols group")


def cond_stride_of(cond_dim):
    """floats per sample of the conditioning vector: its features and the constant 1, up to a multiple of 8"""
    return ((cond_dim + 1 + 7) // 8) * 8


def cond_dims(n_views, cos_n_group):
    """(cond_dim, cond_stride)"""
    cond_dim = int(sum(cos_n_group)) + 4 * n_views
    return cond_dim, cond_stride_of(cond_dim)


def decoder_stage_table(cond_dim, L_3D, legacy, kstep=16):
    """stage name -> Stage: weight key; first column and number of columns of its slice (None: all); bias key or None; column
    map [T, 2, J] (kstep 16: J = 8, the split formats, whose bias travels in the stage header; kstep 2: J = 1, the f32 format,
    whose bias is the column BIAS); scale group - stages of one group share one exponent ew (l5e and l5h: one tensor, one
    accumulator)."""
    d_enc = 3 + 6 * L_3D
    if kstep == 16:
        tf = (cond_dim + 15) // 16
        film = np.arange(16 * tf).reshape(tf, 2, 8)
        film = np.where(film < cond_dim, film, ZERO)
        enc, hid, rgb = _enc_cols16(L_3D, legacy), _reg_cols16(4), _reg_cols16(2)
        hid_b = hid  # a stage with a bias reads the same columns: the bias is not one of them
        dirs = np.full((1, 2, 8), ZERO, np.int64)
        dirs[0, 0, :3] = [128, 129, 130]
        views = np.concatenate([hid, dirs], 0)
    else:
        fs = cond_stride_of(cond_dim) // 2
        mark = [c if c < cond_dim else (BIAS if c == cond_dim else ZERO) for c in range(2 * fs)]
        film = _cols2(mark[:fs], mark[fs:])
        (h_lo, h_hi), (v_lo, v_hi) = _reg_order(4), _reg_order(2)
        enc, hid, hid_b = _cols2(*_enc_cols(L_3D, legacy)), _cols2(h_lo, h_hi), _cols2(h_lo + [BIAS], h_hi + [ZERO])
        views, rgb = _cols2(h_lo + [128, 130], h_hi + [129, BIAS]), _cols2(v_lo + [BIAS], v_hi + [ZERO])

    def lin(module, cols, c0=0, ncols=None, bias=True):
        return Stage(module + ".weight", c0, ncols, module + ".bias" if bias else None, cols, module)

    table = {"film": lin("pts_bias", film), "l0": lin("pts_linears.0", enc),
             "l5e": lin("pts_linears.5", enc, 0, d_enc), "l5h": lin("pts_linears.5", hid, d_enc, 128, bias=False),
             "alpha": lin("alpha_linear.0", hid_b), "feature": lin("feature_linear", hid_b),
             "views": lin("views_linears.0", views), "rgb": lin("rgb_linear", rgb)}
    table.update({f"l{i}": lin(f"pts_linears.{i}", hid_b) for i in range(1, 5)})
    return table


def decoder_stages(cond_stride, L_3D):
    fs, es = cond_stride // 2, 3 * L_3D + 2
    names = ["film", "l0", "l1", "l2", "l3", "l4", "l5e", "l5h", "feature", "views", "rgb", "alpha"]
    steps = [fs, es, 65, 65, 65, 65, es, 64, 65, 66, 33, 65]
    nmb = [4, 4, 4, 4, 4, 4, 4, 4, 4, 2, 1, 1]
    return list(zip(names, steps, nmb))


def decoder_schedule(cond_stride, L_3D):
    """Mirror of build_schedule() in csrc/decoder_common.hpp -> (segments, total_floats);
    segment = (stage, first_step, n_steps, nmb, float_offset, padded_floats)."""
    segs, off = [], 0
    for name, t, m in decoder_stages(cond_stride, L_3D):
        cap = SEG_CAP_FLOATS // (64 * m)
        nseg = (t + cap - 1) // cap
        base = t // nseg
        first = 0
        for k in range(nseg):
            steps = t - base * (nseg - 1) if k == nseg - 1 else base
            fl = ((steps * 64 * m + 255) // 256) * 256
            assert fl <= SEG_CAP_FLOATS
            segs.append((name, first, steps, m, off, fl))
            off += fl
            first += steps
    segs.append(("tail", 0, 0, 0, off, TAIL_SEG_FLOATS))
    return segs, off + TAIL_SEG_FLOATS


def _split_stages(cond_dim, L_3D, per):
    """(name, nmb, [K16-steps per segment], has_header) in consumption order: 4-block stages in segments of `per` steps"""
    def chunks(t):
        return [per] * (t // per) + ([t % per] if t % per else [])

    tf, te = (cond_dim + 15) // 16, (3 * L_3D + 2 + 7) // 8
    st = [("film", 4, chunks(tf), True), ("l0", 4, chunks(te), True)]
    st += [(f"l{i}", 4, chunks(8), True) for i in range(1, 5)]
    # alpha right after the trunk: it and feature are the only consumers of the last hidden activations, which
    # are then dead during views / rgb (its 16 outputs wait in 8 registers for the ray transformer)
    st += [("l5e", 4, chunks(te), True), ("l5h", 4, chunks(8), False), ("alpha", 1, [8], True),
           ("feature", 4, chunks(8), True), ("views", 2, [4, 5], True), ("rgb", 1, [4], True)]
    return st


def decoder_stages16(cond_dim, L_3D):
    return _split_stages(cond_dim, L_3D, 2)


def decoder_stages_h(cond_dim, L_3D):
    return _split_stages(cond_dim, L_3D, H_SEG_STEPS)


def _split_schedule(stages, parts):
    """-> (segments, total_floats) of a split format with `parts` fragments per unit;
    segment = (stage, first_step, n_steps, nmb, float_offset, floats, has_header)."""
    segs, off = [], 0
    for name, m, seg_steps, has_hdr in stages:
        first = 0
        for k, steps in enumerate(seg_steps):
            hdr = has_hdr and k == 0
            fl = (steps * m * parts + (1 if hdr else 0)) * FRAG_FLOATS
            assert fl <= SEG_CAP_FLOATS, (name, fl)
            segs.append((name, first, steps, m, off, fl, hdr))
            off += fl
            first += steps
    segs.append(("tail", 0, 0, 0, off, TAIL_SEG_FLOATS, False))
    return segs, off + TAIL_SEG_FLOATS


def decoder_schedule16(cond_dim, L_3D):
    return _split_schedule(decoder_stages16(cond_dim, L_3D), 3)


def decoder_schedule_h(cond_dim, L_3D):
    return _split_schedule(decoder_stages_h(cond_dim, L_3D), 2)


# ----------------------------------------------------------------------------- decoder: the numpy packers


def _reader(sd, prefix, L_3D):
    def g(name):
        return as_f32(sd[prefix + name])

    assert g("pts_linears.5.weight").shape[1] == 3 + 6 * L_3D + 128, "decoder.skip must be [4] with net_width 128"
    return g


def _stage_slice(w, st):
    return w[:, st.c0:] if st.ncols is None else w[:, st.c0:st.c0 + st.ncols]


def _fragments(weight, bias, cols, nmb):
    """A[t, lane, m] of the f32 format for one stage (float32 [T, 64, nmb]); cols [T, 2, 1]"""
    n_out, n_in = weight.shape
    ext = np.concatenate([weight, np.zeros((n_out, 1), np.float32) if bias is None else bias[:, None]], 1)  # [W | bias]
    idx = fragment_index(np.where(cols == BIAS, n_in, cols), nmb, n_out, n_in + 1, pad=ext.size)
    return _with_zero(ext)[idx][..., 0].transpose(0, 2, 1)


def pack_tail(g):
    """float32 [TAIL_SEG_FLOATS], exact-f32 fragments in every format: ray-transformer projections [w_qs; w_ks; w_vs]
    (48 rows), fc, out_alpha_linear.{0,2}"""
    a_lo, a_hi = (x[:8] for x in _reg_order(1))  # 16 inputs held in registers 0..7 of one block
    a, a_b = _cols2(a_lo, a_hi), _cols2(a_lo + [BIAS], a_hi + [ZERO])
    wqkv = np.concatenate([g(f"ray_attention.w_{x}s.weight") for x in "qkv"], 0)
    tail = {"qkv": _fragments(wqkv, None, a, 2),
            "fco": _fragments(g("ray_attention.fc.weight"), None, _cols2(range(8), range(8, 16)), 1),
            "oa0": _fragments(g("out_alpha_linear.0.weight"), g("out_alpha_linear.0.bias"), a_b, 1),
            "oa2": _fragments(g("out_alpha_linear.2.weight"), g("out_alpha_linear.2.bias"), a_b, 1)}
    out = np.zeros(TAIL_SEG_FLOATS, np.float32)
    for sub, (off, t, nm) in TAIL_LAYOUT.items():
        assert tail[sub].shape == (t, 64, nm), (sub, tail[sub].shape)
        out[off:off + tail[sub].size] = tail[sub].reshape(-1)
    return out


def pack_wstream(sd, n_views, cos_n_group, L_3D=10, legacy=True, prefix="nerf_dec."):
    """state_dict (numpy or torch, reference keys) -> (wstream float32 [total], cond_dim, cond_stride)."""
    g = _reader(sd, prefix, L_3D)
    cond_dim, cond_stride = cond_dims(n_views, cos_n_group)
    table = decoder_stage_table(cond_dim, L_3D, legacy, kstep=2)
    segs, total = decoder_schedule(cond_stride, L_3D)
    out, frags = np.zeros(total, np.float32), {}
    for name, first, steps, m, off, fl in segs:
        if name == "tail":
            out[off:off + fl] = pack_tail(g)
            continue
        if name not in frags:
            st = table[name]
            frags[name] = _fragments(_stage_slice(g(st.weight), st), g(st.bias) if st.bias else None, st.cols, m)
        a = frags[name][first:first + steps]
        assert a.shape == (steps, 64, m), (name, a.shape, steps, m)
        out[off:off + a.size] = a.reshape(-1)
    return out, cond_dim, cond_stride


def _fragment_values(weight, cols, nmb, ew=0):
    """float32 [T, nmb, 64, 8]: 2^ew * W[32m + lane%32, cols[t, lane//32, j]]"""
    idx = fragment_index(cols, nmb, weight.shape[0], weight.shape[1], pad=weight.size)
    return _with_zero(np.ldexp(weight.astype(np.float32), ew))[idx]


def _fragments16(weight, cols, nmb):
    """uint16 [T, nmb, 3, 64, 8]: bf16 parts of W[32m + lane%32, cols[t, lane//32, j]]."""
    return np.stack(split_bf16x3(_fragment_values(weight, cols, nmb)), 2)


def _fragments_h(weight, cols, nmb, ew):
    """float16 [T, nmb, 2, 64, 8]: (hi, lo) parts of 2^ew * W[32m + lane%32, cols[t, lane//32, j]]."""
    return np.stack(split_f16x2(_fragment_values(weight, cols, nmb, ew)), 2)


def _pack_wstream_split(sd, n_views, cos_n_group, L_3D, legacy, prefix, parts):
    """the split-bf16 (parts = 3) or split-fp16 (parts = 2) decoder stream"""
    g = _reader(sd, prefix, L_3D)
    cond_dim, cond_stride = cond_dims(n_views, cos_n_group)
    table = decoder_stage_table(cond_dim, L_3D, legacy)
    segs, total = (decoder_schedule_h if parts == 2 else decoder_schedule16)(cond_dim, L_3D)
    out = np.zeros(total, np.float32)
    out16 = out.view(np.uint16)
    frags, ews = {}, {}
    for name, first, steps, m, off, fl, hdr in segs:
        if name == "tail":
            out[off:off + fl] = pack_tail(g)
            continue
        st = table[name]
        if parts == 2 and st.group not in ews:
            ews[st.group] = f16_weight_exponent(g(st.weight))
        if name not in frags:
            w = _stage_slice(g(st.weight), st)
            frags[name] = (_fragments_h(w, st.cols, m, ews[st.group]) if parts == 2 else _fragments16(w, st.cols, m)).view(np.uint16)
        if hdr:
            out[off:off + FRAG_FLOATS] = _bias_fragment(g(st.bias) if st.bias else None, m)  # floats [128, 256) are zero
            if parts == 2:
                out[off + 128] = np.ldexp(np.float32(1.0), -ews[st.group])
                out[off + 129] = np.float32(ews[st.group])   # the kernel reads the exponent (scales are tracked as integers)
            off += FRAG_FLOATS
        a = frags[name][first:first + steps]
        out16[2 * off:2 * off + a.size] = a.reshape(-1)
    return out, cond_dim, cond_stride


def pack_wstream16(sd, n_views, cos_n_group, L_3D=10, legacy=True, prefix="nerf_dec."):
    """state_dict -> (wstream as float32 words [total], cond_dim, cond_stride) in the split-bf16 format."""
    return _pack_wstream_split(sd, n_views, cos_n_group, L_3D, legacy, prefix, 3)


def pack_wstream_h(sd, n_views, cos_n_group, L_3D=10, legacy=True, prefix="nerf_dec."):
    """state_dict -> (wstream as float32 words [total], cond_dim, cond_stride) in the split-fp16 format."""
    return _pack_wstream_split(sd, n_views, cos_n_group, L_3D, legacy, prefix, 2)


def pack_for_math(math):
    return {"f32": pack_wstream, "bf16x6": pack_wstream16, "f16x3": pack_wstream_h, "f16": pack_wstream_h}[math]


def raytrans_table(n_samples, d_hid=16):
    """Sinusoid table of the ray transformer, float64 -> float32 as the reference builds it
    (cond_nerf.py:118-127)."""
    pos = np.arange(n_samples, dtype=np.float64)[:, None]
    j = np.arange(d_hid)[None, :]
    tab = pos / np.power(10000, 2 * (j // 2) / d_hid)
    tab[:, 0::2] = np.sin(tab[:, 0::2])
    tab[:, 1::2] = np.cos(tab[:, 1::2])
    return tab.astype(np.float32)


def pack_small(sd, n_samples, raytrans_posenc, prefix="nerf_dec."):
    """Parameters that are not matrix operands: [0:16) LayerNorm weight, [16:32) LayerNorm bias of
    the ray transformer, then the [S,16] sinusoid table when ``raytrans_posenc``."""
    out = np.zeros(SMALL_FIXED + (n_samples * 16 if raytrans_posenc else 0), np.float32)
    out[0:16] = as_f32(sd[prefix + "ray_attention.layer_norm.weight"]).reshape(-1)
    out[16:32] = as_f32(sd[prefix + "ray_attention.layer_norm.bias"]).reshape(-1)
    if raytrans_posenc:
        out[SMALL_FIXED:] = raytrans_table(n_samples).reshape(-1)
    return out


# ----------------------------------------------------------------------------- recipes of the split-fp16 unit streams
# A recipe is a list of units in stream order.  Unit: `tensor` - index into the recipe's tensor list (one exponent ew per
# tensor); `cols` [T, 2, 8]; `nmb` 32-row blocks; `rows` - stream row -> matrix row (None: as they are); `view(shape)` ->
# (n_rows, n_cols, flat_of) when the matrix is not the tensor itself (a convolution filter).  A unit is T * nmb * 512 words.

Unit = namedtuple("Unit", "tensor cols nmb rows view", defaults=(None, None))


def unit_index(u, shape, base=0, pad=-1):
    """fragment_index of unit `u` over a tensor of `shape` stored at `base`"""
    n_rows, n_cols, flat_of = (shape[0], shape[1], None) if u.view is None else u.view(shape)
    return fragment_index(u.cols, u.nmb, n_rows if u.rows is None else len(u.rows), n_cols, u.rows, flat_of, base, pad)


def stream_index(units, shapes, bases, pad=-1):
    """int64 [units x 512 words, 512]: a recipe's stream as positions in a concatenation where tensor i starts at bases[i]"""
    return np.concatenate([unit_index(u, shapes[u.tensor], bases[u.tensor], pad).reshape(-1, 512) for u in units], 0)


def pack_units(units, tensors):
    """A recipe on the host -> (wstream float32 words, one exponent per tensor)"""
    tensors = [as_f32(t) for t in tensors]
    ews = [f16_weight_exponent(t) for t in tensors]
    scaled = [_with_zero(np.ldexp(t, e)) for t, e in zip(tensors, ews)]
    halfs = [np.stack(split_f16x2(scaled[u.tensor][unit_index(u, tensors[u.tensor].shape, pad=tensors[u.tensor].size)]), 2)
             for u in units]                                     # fp16 [T, nmb, hi | lo, 64, 8] per unit
    return np.concatenate([h.reshape(-1) for h in halfs]).view(np.float32), tuple(ews)


def qkv_units(shapes):
    """q/k/v projection weights [128,128] for ``mnerf_qkv_projection`` (csrc/qkv.hip): three matrices of 8 K16-steps x 4 row
    blocks, input features in natural order, each with its own power-of-two scale; Wk's rows in K_ROW_ORDER (accumulator
    registers 8t..8t+7 of a lane = the attention's K16-step t)."""
    assert [tuple(s) for s in shapes] == [(128, 128)] * 3, shapes
    return [Unit(0, NATURAL, 4), Unit(1, NATURAL, 4, K_ROW_ORDER), Unit(2, NATURAL, 4)]


def encoder_block_units(shapes):
    """One transformer layer's post-attention chain (merge[, mlp.0, mlp.2]) for ``mnerf_encoder_block``
    (csrc/encoder_block.hip).  Segment order: merge (2 segments: input features 0-63, 64-127 in natural order), then for
    every 128-unit hidden chunk c: mlp.0 rows [128c, 128c+128) (4 segments: the 128 source features in natural order, then
    the 128 message features in accumulator order) and mlp.2 columns [128c, 128c+128) (2 segments, accumulator order)."""
    shapes = [tuple(s) for s in shapes]
    assert shapes in ([(128, 128)], [(128, 128), (1024, 256), (128, 1024)]), shapes
    units = [Unit(0, NATURAL, 4)]
    if len(shapes) == 3:
        acc_order = _reg_cols16(4)                               # accumulator-register order of a 128-row stage
        cols1 = np.concatenate([NATURAL, 128 + acc_order], 0)    # 16 steps over cat[source, message]
        for c in range(1024 // EB_CHUNK):
            units += [Unit(1, cols1, 4, EB_CHUNK * c + np.arange(EB_CHUNK)), Unit(2, EB_CHUNK * c + acc_order, 4)]
    assert sum(u.cols.size * u.nmb * 32 for u in units) % EB_SEG_FLOATS == 0
    return units


def _conv_taps(c_in_padded):
    def view(shape):  # the implicit-GEMM matrix: row = co, col = tap * c_in_padded + c  ->  W[co][c][ky][kx]
        co, ci, k, _ = shape

        def flat_of(row, col):
            tap, c = col // c_in_padded, col % c_in_padded
            return np.where(c < ci, row * (ci * k * k) + ((c * k + tap // k) * k + tap % k), -1)
        return co, k * k * c_in_padded, flat_of
    return view


def _conv_flipped(shape):  # the data gradient's matrix: row = ci, col = tap' * co + o  ->  W[o][ci][k-1-ky'][k-1-kx']
    co, ci, k, _ = shape

    def flat_of(row, col):
        tap, o = col // co, col % co
        return row * (k * k) + ((o * ci * k + (k - 1 - tap // k)) * k + (k - 1 - tap % k))
    return ci, k * k * co, flat_of


def conv_units(shape, block=None, pad_c_in=False):
    """Conv2d weight [c_out, c_in, k, k] for ``mnerf_conv2d`` / ``mnerf_conv_stem`` (csrc/conv.hip): the implicit-GEMM matrix
    W[out, tap * c_in + c] (tap = ky * k + kx), K16-step s = 16 consecutive columns (zeros behind the last), every `block`
    output rows a stream of their own, one after the other; `pad_c_in`: c_in counted up to a multiple of 32 with zeros."""
    c_out, c_in, k, _ = shape
    c_pad = c_in + (-c_in % 32 if pad_c_in else 0)
    cols = np.arange((k * k * c_pad + 15) // 16 * 16).reshape(-1, 2, 8)
    rows = min(block or c_out, c_out)
    return [Unit(0, cols, rows // 32, r + np.arange(rows), _conv_taps(c_pad)) for r in range(0, c_out, rows)]


def conv_backward_units(shape):
    """the ``conv_units`` stream of the flipped, transposed filter W'[ci, tap' * c_out + co] = W[co, ci, k-1-ky', k-1-kx']:
    ``mnerf_conv2d`` over dY with it IS dX of a stride-1 convolution"""
    c_out, c_in, k, _ = shape
    return [Unit(0, np.arange(k * k * c_out).reshape(-1, 2, 8), c_in // 32, None, _conv_flipped)]


def pack_qkv(wq, wk, wv):
    """-> (wstream float32 words, (ew_q, ew_k, ew_v)): ``qkv_units``"""
    ws = [as_f32(w) for w in (wq, wk, wv)]
    return pack_units(qkv_units([w.shape for w in ws]), ws)


def pack_encoder_block(merge_w, mlp0_w=None, mlp2_w=None):
    """-> (wstream float32 words, (ew_merge, ew_w1, ew_w2)): ``encoder_block_units``"""
    ws = [as_f32(w) for w in ((merge_w,) if mlp0_w is None else (merge_w, mlp0_w, mlp2_w))]
    stream, ews = pack_units(encoder_block_units([w.shape for w in ws]), ws)
    return stream, (ews + (0, 0))[:3]


def pack_conv(weight):
    """Conv2d weight [c_out, c_in, k, k] -> (wstream float32 words, ew) for ``mnerf_conv2d``: ``conv_units``"""
    w = as_f32(weight)
    c_out, c_in, kh, kw = w.shape
    assert kh == kw and c_in % 32 == 0 and c_out % 32 == 0, w.shape
    ws, (ew,) = pack_units(conv_units(w.shape), [w])
    return ws, ew


def pack_conv_blocks(weight, block=128):
    """Conv2d weight [c_out, c_in, k, k] of ANY width -> (wstream, ew) for ``mnerf_conv2d`` with c_out above 128 (csrc/conv.hip: the
    output channels run in blocks of ``block`` along a grid dimension): the ``pack_conv`` stream of every block of ``block`` rows,
    one after the other, all with ONE exponent ew (the kernel scales the result back by one power of two per layer).  c_in is
    zero-padded to a multiple of 32 (the first layer of LPIPS's VGG-16: 3 -> 32).  c_out <= ``block``: exactly ``pack_conv``."""
    w = as_f32(weight)
    c_out, c_in, kh, kw = w.shape
    assert kh == kw and c_out % 32 == 0 and (c_out <= block or c_out % block == 0), w.shape
    ws, (ew,) = pack_units(conv_units(w.shape, block, pad_c_in=True), [w])
    return ws, ew


def pack_conv_stem(weight):
    """The stem's weight [64, 3, 7, 7] -> (wstream, ew) for ``mnerf_conv_stem``: matrix [64, 3 tap + c], 147 columns
    padded with zeros to ten K16-steps."""
    w = as_f32(weight)
    assert w.shape == (64, 3, 7, 7), w.shape
    ws, (ew,) = pack_units(conv_units(w.shape), [w])
    return ws, ew
