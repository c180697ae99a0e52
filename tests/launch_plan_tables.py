"""Which kernel instance each float64 parity case launches: one table per dispatcher of csrc/ (mnerf_debug_launch_plan,
include/mnerf.h).  The GPU tests take their cases from here, tests/test_launch_plans.py asks the library's own selection function
for every case (no GPU needed) and fails when an instance is left without a case or a case drifts to another instance - a tuned
threshold moves rows of this file, visibly.

A table maps an instance to the parity cases that select it.  New cases are the smallest shapes that reach the instance with odd
sizes, more than one image where the row arithmetic has one, and a row of at least one full and one ragged 32-position segment."""

# ------------------------------------------------------------------------------------------------ mnerf_conv2d (conv.hip)
# case: n, c_in, c_out, k, stride, h, w, channels_last, upsample2x, leaky, bias      (tests/test_conv.py)
CONV_CASES = [
    (3, 64, 64, 3, 1, 64, 80, False, False, 1.0, False),
    (2, 64, 96, 3, 2, 64, 80, False, False, 1.0, False),
    (2, 64, 96, 1, 2, 64, 80, False, False, 1.0, True),
    (2, 96, 96, 3, 1, 32, 40, False, False, 1.0, False),
    (2, 96, 128, 3, 2, 33, 41, False, False, 1.0, False),   # odd sizes: ragged last tile, odd stride-2 geometry
    (1, 128, 128, 1, 1, 8, 10, False, False, 1.0, True),
    (2, 128, 128, 3, 1, 16, 20, True, False, 1.0, True),     # channel-last tokens in
    (2, 128, 128, 3, 1, 16, 20, True, True, 0.2, True),      # ... through a nearest 2x up-sampling, LeakyReLU epilogue
    (1, 128, 128, 3, 1, 9, 7, False, True, 0.2, True),
]
# two pixel tiles per wave (tpw = 2) start at 65 281 output pixels; every case has a ragged last workgroup (n_pix % 256 != 0)
CONV_TPW2_CASES = [
    (1, 64, 64, 3, 1, 255, 257, False, False, 1.0, False),   # 65 535 pixels: layer1 of the backbone on a full frame
    (1, 64, 96, 3, 2, 509, 515, False, False, 1.0, False),   # 255 x 258 = 65 790 out of an odd stride-2 geometry
    (1, 128, 128, 3, 1, 255, 257, False, False, 1.0, True),  # the up-sampler's NCHW convolution
    (1, 128, 128, 3, 1, 255, 257, True, False, 1.0, True),   # channel-last tokens in
    (1, 128, 128, 3, 1, 127, 129, True, True, 0.2, True),    # ... through the nearest 2x up-sampling: 254 x 258 = 65 532 out
]
# c_out above 128: blocks of 128 output channels along grid.y (n_blk), 1x1 to keep the float64 reference cheap
CONV_WIDE_CASES = [
    (1, 64, 256, 1, 1, 255, 257, False, False, 1.0, True),   # tpw 2, two blocks
    (2, 32, 256, 1, 1, 9, 11, False, False, 1.0, True),      # tpw 1, two blocks
    (1, 32, 512, 1, 1, 9, 11, False, False, 1.0, False),     # tpw 1, four blocks
]


def conv2d_args(case):
    n, ci, co, k, s, h, w, cl, up = case[:9]
    return (ci, co, k, s, n, h, w, int(cl), int(up))


# conv_kernel<NMB, TPW, CL> -> cases; the wide rows are the same <4, TPW, false> kernels over n_blk > 1 blocks
CONV2D_INSTANCES = [(nmb, tpw, 0) for nmb in (2, 3, 4) for tpw in (1, 2)] + [(4, 1, 1), (4, 2, 1)]
CONV2D_TABLE = {  # (nmb, tpw, cl, n_blk)
    (2, 1, 0, 1): [CONV_CASES[0]],
    (3, 1, 0, 1): [CONV_CASES[1], CONV_CASES[2], CONV_CASES[3]],
    (4, 1, 0, 1): [CONV_CASES[4], CONV_CASES[5], CONV_CASES[8]],
    (4, 1, 1, 1): [CONV_CASES[6], CONV_CASES[7]],
    (2, 2, 0, 1): [CONV_TPW2_CASES[0]],
    (3, 2, 0, 1): [CONV_TPW2_CASES[1]],
    (4, 2, 0, 1): [CONV_TPW2_CASES[2]],
    (4, 2, 1, 1): [CONV_TPW2_CASES[3], CONV_TPW2_CASES[4]],
    (4, 2, 0, 2): [CONV_WIDE_CASES[0]],
    (4, 1, 0, 2): [CONV_WIDE_CASES[1]],
    (4, 1, 0, 4): [CONV_WIDE_CASES[2]],
}

# ------------------------------------------------------------------------ conv_gemm_kernel / weight gradient (conv_backward.hip)
# case: n, c_in, c_out, h, w, k, stride      (tests/test_conv_backward.py)
CB_CASES = [
    (2, 64, 64, 20, 40, 3, 1), (1, 64, 96, 21, 37, 3, 2), (2, 96, 96, 12, 24, 3, 1), (1, 96, 128, 16, 24, 3, 2),
    (1, 128, 128, 9, 13, 3, 1), (2, 64, 96, 10, 18, 1, 2), (1, 96, 128, 11, 15, 1, 2), (2, 128, 128, 8, 10, 1, 1),
    (1, 32, 64, 7, 5, 3, 1), (1, 128, 32, 6, 70, 3, 1),
]
CB_STEM_FWD_CASES = [(2, 3, 64, 30, 44, 7, 2), (1, 3, 64, 17, 23, 7, 2)]
CB_BACKBONE_SHAPE = (3, 64, 64, 256, 320, 3, 1)   # test_conv_backward_at_the_backbone_shape

# conv_gemm_kernel<CIB, NB, FWD = false, TAIL = false>: mnerf_conv2d_backward_data.  The channel counts, filters and strides are the
# ones a 512 x 640 or 800 x 800 training step sends to the instance (FULL_FRAME below).
CB_DATA_NEW = {  # (cib, nb) -> cases
    (1, 2): [(2, 96, 96, 171, 65, 3, 1)],
    (2, 1): [(1, 128, 128, 513, 33, 3, 1), (1, 128, 128, 513, 33, 1, 1)],
    (2, 2): [(1, 64, 96, 513, 129, 3, 2), (1, 64, 96, 513, 129, 1, 2)],
    (3, 1): [(1, 96, 128, 513, 65, 3, 2), (1, 96, 128, 513, 65, 1, 2), (2, 96, 96, 513, 33, 3, 1)],
    (4, 1): [(2, 128, 128, 513, 33, 3, 1)],
}
# conv_gemm_kernel<CIB, NB, FWD = true, TAIL>: mnerf_conv2d_forward_f32.  TAIL = a source channel count that is no multiple of 8; the
# model has one such layer, the stem (3 -> 64, 7x7 stride 2), which reaches <1,1>, <1,2>, <2,1> and <2,2>.  <3,1> and <4,1> with TAIL
# need 3 -> 96 / 128 channels: no layer of the model does that, the entry point accepts it, so one 3x3 case each covers the instance.
CB_FWD_NEW = {  # (cib, nb, tail) -> cases
    (1, 2, 0): [(3, 64, 96, 227, 129, 3, 2), (2, 96, 96, 171, 65, 3, 1), (3, 64, 96, 227, 129, 1, 2)],
    (2, 1, 0): [(1, 128, 128, 513, 33, 3, 1), (1, 128, 128, 513, 33, 1, 1), (2, 96, 128, 511, 65, 3, 2), (2, 96, 128, 511, 65, 1, 2)],
    (2, 2, 0): [(2, 64, 64, 513, 65, 3, 1)],
    (3, 1, 0): [(3, 64, 96, 455, 129, 3, 2), (3, 64, 96, 455, 129, 1, 2), (2, 96, 96, 513, 33, 3, 1)],
    (4, 1, 0): [(2, 128, 128, 513, 33, 3, 1)],
    (1, 2, 1): [(2, 3, 64, 511, 129, 7, 2)],
    (2, 1, 1): [(3, 3, 64, 455, 129, 7, 2)],
    (2, 2, 1): [(3, 3, 64, 455, 257, 7, 2)],
    (3, 1, 1): [(2, 3, 96, 513, 33, 3, 1)],
    (4, 1, 1): [(2, 3, 128, 513, 33, 3, 1)],
}
CB_GEMM_INSTANCES = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 1), (4, 1)]
CB_DATA_TABLE = dict({(1, 1): list(CB_CASES), (2, 2): [CB_BACKBONE_SHAPE]})
for _k, _v in CB_DATA_NEW.items():
    CB_DATA_TABLE[_k] = CB_DATA_TABLE.get(_k, []) + _v
CB_FWD_TABLE = dict({(1, 1, 0): list(CB_CASES), (1, 1, 1): list(CB_STEM_FWD_CASES)})
CB_FWD_TABLE.update(CB_FWD_NEW)


def flat(table):
    return [case for cases in table.values() for case in cases]


# weight gradient: conv_wgrad_kernel<K, S> (exact f32) and conv_wgrad16_kernel<K, S> (split fp16) share cb_chunks.  Every case below
# has rows-per-chunk > 1, a short last chunk (rows % rpc != 0) and chunks that straddle two images (ho % rpc != 0, n > 1); every
# case of CB_CASES has rpc = 1.  Columns: case, chunks, rpc.
CB_WGRAD_NEW = {  # (K, S) -> [(case, chunks, rpc)]
    (3, 1): [((2, 128, 128, 61, 37, 3, 1), 41, 3)],
    (3, 2): [((2, 96, 128, 153, 75, 3, 2), 52, 3)],   # rpc = 3, what the stride-2 layers of a 512 x 640 training step run
    (1, 1): [((3, 128, 128, 87, 37, 1, 1), 131, 2)],
    (1, 2): [((3, 96, 128, 229, 75, 1, 2), 173, 2)],
}
CB_WGRAD_CASES = [case for rows in CB_WGRAD_NEW.values() for case, _, _ in rows]

# ------------------------------------------------------------------------------------------- instance norm (instance_norm.hip)
# (T, V) of the register-cached instance or (0, 0) for the streaming kernel -> shapes [N, C, H, W]; ("unaligned", shape): the same
# plane at a buffer that starts 4 bytes past a 16-byte boundary
IN_FWD_SHAPES = [(3, 64, 256, 320), (3, 96, 128, 160), (2, 128, 64, 80), (1, 5, 7, 9), (1, 3, 400, 400), (2, 4, 50, 50)]  # tests/test_instance_norm.py
IN_FWD_TABLE = {
    (256, 8): [IN_FWD_SHAPES[2], IN_FWD_SHAPES[5]],
    (256, 20): [IN_FWD_SHAPES[1]],
    (512, 40): [IN_FWD_SHAPES[0]],
    (0, 0): [IN_FWD_SHAPES[3], IN_FWD_SHAPES[4]],
}
IN_BWD_OLD = [(2, 5, 16, 24), (1, 3, 7, 9), (1, 2, 256, 320)]   # tests/test_conv_backward.py
IN_BWD_NEW = [(1, 2, 128, 160), (1, 3, 2, 4098), (1, 2, 127, 161), ("unaligned", (1, 2, 128, 160))]
IN_BWD_TABLE = {
    (256, 8): [IN_BWD_OLD[0]],
    (256, 20): [IN_BWD_NEW[0], IN_BWD_NEW[1]],           # both ends of (8 192, 20 480]
    (512, 40): [IN_BWD_OLD[2]],
    (0, 0): [IN_BWD_OLD[1], IN_BWD_NEW[2], IN_BWD_NEW[3]],
}


def instance_norm_args(entry):
    aligned = entry[0] != "unaligned"
    shape = entry if aligned else entry[1]
    return (shape[2] * shape[3], int(aligned))


# ------------------------------------------------------------------------------------------ window attention (window_attention.hip)
# case: b, h, w, splits, wa_min4 (None: the library's default, 200) -> 4 (128-query workgroups) or 2
WA_FORCED4 = (2, 20, 30, 2, 1)      # 150-token windows under the knob: a 22-row last query block, a 22-key last tile
WA_NATURAL4 = (6, 66, 70, 2, None)  # 1155-token windows: 240 workgroups of 128 queries, 3 live rows in the last block and key tile
WA_DTU_SHAPES = ((2, 64, 80, 2), (1, 50, 50, 2))   # b, h, w, splits: test_window_attention_dtu_shape_matches_oracle
WA_BWD_CASES = [  # b, h, w, splits, shifted: tests/test_window_attention_backward.py
    (2, 16, 24, 2, False),   # 96-token windows: one and a half 64-row tiles
    (2, 16, 24, 2, True),    # wrap-region mask
    (1, 12, 20, 1, False),   # one window = the whole map (global attention), 240 tokens
    (3, 24, 24, 2, True),    # 144-token windows, odd tile remainder
    (2, 32, 40, 4, True),    # attn_splits 4 (rect_wide / IBRNet-style)
    (6, 64, 80, 2, True),    # the DTU shape: 3 pairs x 2 directions, 1280-token windows
]
WA_TABLE = {
    4: [WA_FORCED4, WA_NATURAL4, WA_BWD_CASES[5][:4] + (None,)],
    2: [c + (None,) for c in WA_DTU_SHAPES] + [c[:4] + (None,) for c in WA_BWD_CASES[:5]],
}

# ------------------------------------------------------------------------------------- what full frames select, layer by layer
# the convolutions of GMFlow's CNN backbone (3 views) and up-sampler (6 maps: 3 pairs x 2 directions): name, n, c_in, c_out, k, stride
# and the input size as a divisor of the frame
LAYERS = [("layer1.0.conv1", 3, 64, 64, 3, 1, 2), ("layer1.0.conv2", 3, 64, 64, 3, 1, 2), ("layer1.1.conv1", 3, 64, 64, 3, 1, 2),
          ("layer1.1.conv2", 3, 64, 64, 3, 1, 2), ("layer2.0.conv1", 3, 64, 96, 3, 2, 2), ("layer2.0.conv2", 3, 96, 96, 3, 1, 4),
          ("layer2.0.downsample", 3, 64, 96, 1, 2, 2), ("layer2.1.conv1", 3, 96, 96, 3, 1, 4), ("layer2.1.conv2", 3, 96, 96, 3, 1, 4),
          ("layer3.0.conv1", 3, 96, 128, 3, 2, 4), ("layer3.0.conv2", 3, 128, 128, 3, 1, 8), ("layer3.0.downsample", 3, 96, 128, 1, 2, 4),
          ("layer3.1.conv1", 3, 128, 128, 3, 1, 8), ("layer3.1.conv2", 3, 128, 128, 3, 1, 8), ("conv2", 3, 128, 128, 1, 1, 8),
          ("featup.conv_l2rs.0", 6, 128, 128, 3, 1, 8), ("featup.conv_ls.0", 6, 128, 128, 3, 1, 4), ("featup.conv_l2rs.1", 6, 128, 128, 3, 1, 4)]
# per frame size, per layer: conv2d = (nmb, tpw, cl) of the inference pass (the split-fp16 training forward takes the same nmb, tpw
# from NCHW input), gemm_fwd / gemm_bwd = (cib, nb) of the exact-f32 training forward / the data gradient, wgrad = (chunks, rpc)
FULL_FRAME = {
    (512, 640): {
        "stem_gemm_fwd": (2, 2, 1),
        "layer1.0.conv1": dict(conv2d=(2, 2, 0), gemm_fwd=(2, 2), gemm_bwd=(2, 2), wgrad=(192, 4)),
        "layer1.0.conv2": dict(conv2d=(2, 2, 0), gemm_fwd=(2, 2), gemm_bwd=(2, 2), wgrad=(192, 4)),
        "layer1.1.conv1": dict(conv2d=(2, 2, 0), gemm_fwd=(2, 2), gemm_bwd=(2, 2), wgrad=(192, 4)),
        "layer1.1.conv2": dict(conv2d=(2, 2, 0), gemm_fwd=(2, 2), gemm_bwd=(2, 2), wgrad=(192, 4)),
        "layer2.0.conv1": dict(conv2d=(3, 1, 0), gemm_fwd=(1, 2), gemm_bwd=(2, 2), wgrad=(128, 3)),
        "layer2.0.conv2": dict(conv2d=(3, 1, 0), gemm_fwd=(1, 2), gemm_bwd=(1, 2), wgrad=(96, 4)),
        "layer2.0.downsample": dict(conv2d=(3, 1, 0), gemm_fwd=(1, 2), gemm_bwd=(2, 2), wgrad=(384, 1)),
        "layer2.1.conv1": dict(conv2d=(3, 1, 0), gemm_fwd=(1, 2), gemm_bwd=(1, 2), wgrad=(96, 4)),
        "layer2.1.conv2": dict(conv2d=(3, 1, 0), gemm_fwd=(1, 2), gemm_bwd=(1, 2), wgrad=(96, 4)),
        "layer3.0.conv1": dict(conv2d=(4, 1, 0), gemm_fwd=(1, 1), gemm_bwd=(3, 1), wgrad=(64, 3)),
        "layer3.0.conv2": dict(conv2d=(4, 1, 0), gemm_fwd=(1, 1), gemm_bwd=(1, 1), wgrad=(48, 4)),
        "layer3.0.downsample": dict(conv2d=(4, 1, 0), gemm_fwd=(1, 1), gemm_bwd=(3, 1), wgrad=(192, 1)),
        "layer3.1.conv1": dict(conv2d=(4, 1, 0), gemm_fwd=(1, 1), gemm_bwd=(1, 1), wgrad=(48, 4)),
        "layer3.1.conv2": dict(conv2d=(4, 1, 0), gemm_fwd=(1, 1), gemm_bwd=(1, 1), wgrad=(48, 4)),
        "conv2": dict(conv2d=(4, 1, 0), gemm_fwd=(1, 1), gemm_bwd=(1, 1), wgrad=(192, 1)),
        "featup.conv_l2rs.0": dict(conv2d=(4, 1, 1), gemm_fwd=(2, 1), gemm_bwd=(2, 1), wgrad=(55, 7)),
        "featup.conv_ls.0": dict(conv2d=(4, 2, 1), gemm_fwd=(4, 1), gemm_bwd=(4, 1), wgrad=(55, 14)),
        "featup.conv_l2rs.1": dict(conv2d=(4, 2, 0), gemm_fwd=(4, 1), gemm_bwd=(4, 1), wgrad=(55, 14)),
        "instance_norm": {64: (512, 40), 96: (256, 20), 128: (256, 8)},   # per channel count of the stage: planes at 1/2, 1/4, 1/8
        "window_attention": 4,
    },
    (800, 800): {
        "stem_gemm_fwd": (2, 2, 1),
        "layer1.0.conv1": dict(conv2d=(2, 2, 0), gemm_fwd=(2, 2), gemm_bwd=(2, 2), wgrad=(200, 6)),
        "layer1.0.conv2": dict(conv2d=(2, 2, 0), gemm_fwd=(2, 2), gemm_bwd=(2, 2), wgrad=(200, 6)),
        "layer1.1.conv1": dict(conv2d=(2, 2, 0), gemm_fwd=(2, 2), gemm_bwd=(2, 2), wgrad=(200, 6)),
        "layer1.1.conv2": dict(conv2d=(2, 2, 0), gemm_fwd=(2, 2), gemm_bwd=(2, 2), wgrad=(200, 6)),
        "layer2.0.conv1": dict(conv2d=(3, 2, 0), gemm_fwd=(3, 1), gemm_bwd=(2, 2), wgrad=(150, 4)),
        "layer2.0.conv2": dict(conv2d=(3, 2, 0), gemm_fwd=(3, 1), gemm_bwd=(3, 1), wgrad=(100, 6)),
        "layer2.0.downsample": dict(conv2d=(3, 2, 0), gemm_fwd=(3, 1), gemm_bwd=(2, 2), wgrad=(600, 1)),
        "layer2.1.conv1": dict(conv2d=(3, 2, 0), gemm_fwd=(3, 1), gemm_bwd=(3, 1), wgrad=(100, 6)),
        "layer2.1.conv2": dict(conv2d=(3, 2, 0), gemm_fwd=(3, 1), gemm_bwd=(3, 1), wgrad=(100, 6)),
        "layer3.0.conv1": dict(conv2d=(4, 1, 0), gemm_fwd=(2, 1), gemm_bwd=(3, 1), wgrad=(75, 4)),
        "layer3.0.conv2": dict(conv2d=(4, 1, 0), gemm_fwd=(2, 1), gemm_bwd=(2, 1), wgrad=(50, 6)),
        "layer3.0.downsample": dict(conv2d=(4, 1, 0), gemm_fwd=(2, 1), gemm_bwd=(3, 1), wgrad=(300, 1)),
        "layer3.1.conv1": dict(conv2d=(4, 1, 0), gemm_fwd=(2, 1), gemm_bwd=(2, 1), wgrad=(50, 6)),
        "layer3.1.conv2": dict(conv2d=(4, 1, 0), gemm_fwd=(2, 1), gemm_bwd=(2, 1), wgrad=(50, 6)),
        "conv2": dict(conv2d=(4, 1, 0), gemm_fwd=(2, 1), gemm_bwd=(2, 1), wgrad=(150, 2)),
        "featup.conv_l2rs.0": dict(conv2d=(4, 1, 1), gemm_fwd=(4, 1), gemm_bwd=(4, 1), wgrad=(55, 11)),
        "featup.conv_ls.0": dict(conv2d=(4, 2, 1), gemm_fwd=(4, 1), gemm_bwd=(4, 1), wgrad=(55, 22)),
        "featup.conv_l2rs.1": dict(conv2d=(4, 2, 0), gemm_fwd=(4, 1), gemm_bwd=(4, 1), wgrad=(55, 22)),
        "instance_norm": {64: (0, 0), 96: (512, 40), 128: (256, 20)},
        "window_attention": 4,
    },
}
