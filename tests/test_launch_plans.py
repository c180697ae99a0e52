"""Every kernel instance a dispatcher of csrc/ can launch has a float64 parity case, and the cases select what the tables say: the
library's own selection functions (mnerf_debug_launch_plan: the functions the launches call) asked on the CPU for every case of
tests/launch_plan_tables.py, and for every layer of a full-frame encoder pass and training step."""
import pytest

import launch_plan_tables as T
from matchnerf_amd import hip


def plan(what, *args, n=4):
    return hip.launch_plan(what, *args, n_plan=n)


def test_conv2d_cases_select_their_instances_and_none_is_left_out():
    for inst, cases in T.CONV2D_TABLE.items():
        assert cases, inst
        for case in cases:
            assert plan("conv2d", *T.conv2d_args(case)) == inst, (case, inst)
    assert {i[:3] for i in T.CONV2D_TABLE} == set(T.CONV2D_INSTANCES)            # every conv_kernel<NMB, TPW, CL>
    assert {i[3] for i in T.CONV2D_TABLE} == {1, 2, 4}                           # c_out 64-128, 256, 512
    assert {(i[1], i[3] > 1) for i in T.CONV2D_TABLE} >= {(1, True), (2, True)}  # blocks along grid.y under both tile counts
    listed = T.flat(T.CONV2D_TABLE)
    assert sorted(listed) == sorted(T.CONV_CASES + T.CONV_TPW2_CASES + T.CONV_WIDE_CASES)  # each parity case is in one row
    for case in T.CONV_TPW2_CASES + T.CONV_WIDE_CASES[:1]:  # the new large cases: just over the threshold, a ragged last workgroup, odd sizes
        n, ci, co, k, s, h, w, cl, up = case[:9]
        up = int(up)
        ho, wo = ((h << up) + 2 * (k // 2) - k) // s + 1, ((w << up) + 2 * (k // 2) - k) // s + 1
        assert 65281 <= n * ho * wo < 66000 and (n * ho * wo) % 256 and h % 2 and w % 2, case


def test_the_conv2d_threshold_is_where_the_table_says():
    # 255 workgroups of 256 pixels keep one tile per wave, the first pixel of the 256th takes two
    assert plan("conv2d", 64, 64, 3, 1, 1, 255, 256, 0, 0)[1] == 1
    assert plan("conv2d", 64, 64, 3, 1, 1, 1, 65281, 0, 0)[1] == 2
    with pytest.raises(hip.MnerfError):  # channel-last input is built for 128 output channels
        plan("conv2d", 64, 64, 3, 1, 1, 8, 8, 1, 0)
    with pytest.raises(hip.MnerfError):
        plan("conv2d", 64, 80, 3, 1, 1, 8, 8, 0, 0)


def _gemm(fwd, case):
    return plan("conv_gemm", fwd, *case)


def test_conv_gemm_cases_select_their_instances_and_none_is_left_out():
    for inst, cases in T.CB_DATA_TABLE.items():
        assert cases, inst
        for case in cases:
            assert _gemm(0, case) == inst + (0, 0), (case, inst)
    for inst, cases in T.CB_FWD_TABLE.items():
        assert cases, inst
        for case in cases:
            assert _gemm(1, case) == inst + (1,), (case, inst)
    assert set(T.CB_DATA_TABLE) == set(T.CB_GEMM_INSTANCES)  # the data gradient has no TAIL form: c_out is a multiple of 32
    assert set(T.CB_FWD_TABLE) == {i + (t,) for i in T.CB_GEMM_INSTANCES for t in (0, 1)}
    # every (instance, filter, stride) that a full frame sends there is among the cases
    layers = {name: (ci, co, k, s) for name, _, ci, co, k, s, _ in T.LAYERS}
    for frame in T.FULL_FRAME.values():
        for name, (ci, co, k, s) in layers.items():
            for key, table, pad in (("gemm_bwd", T.CB_DATA_TABLE, ()), ("gemm_fwd", T.CB_FWD_TABLE, (0,))):
                cases = table[frame[name][key] + pad]
                assert any(c[1:3] == (ci, co) and c[5:] == (k, s) for c in cases), (name, key, frame[name][key])
    for case in T.flat(T.CB_DATA_NEW) + T.flat(T.CB_FWD_NEW):  # a row holds a full and a ragged 32-position segment
        n, ci, co, h, w, k, s = case
        assert w > 32 and ((w + 2 * (k // 2) - k) // s + 1) % 32 and ((w + s - 1) // s) % 32 and h % 2 and w % 2, case


def test_weight_gradient_chunk_columns_are_hit_for_every_kernel_in_both_forms():
    for case in T.CB_CASES:  # what the older cases reach
        assert plan("conv_wgrad", *case, n=2)[1] == 1, case
    assert plan("conv_wgrad", *T.CB_BACKBONE_SHAPE, n=2) == (192, 4)   # rows % rpc == 0 and ho % rpc == 0: whole chunks inside an image
    assert set(T.CB_WGRAD_NEW) == {(3, 1), (3, 2), (1, 1), (1, 2)}
    for (k, s), rows in T.CB_WGRAD_NEW.items():
        hit = dict(multi_row=False, ragged_last=False, straddles=False)
        for case, chunks, rpc in rows:
            n, ci, co, h, w, kk, ss = case
            assert (kk, ss) == (k, s)
            assert plan("conv_wgrad", *case, n=2) == (chunks, rpc), case
            ho = (h + 2 * (k // 2) - k) // s + 1
            hit["multi_row"] |= rpc > 1
            hit["ragged_last"] |= rpc > 1 and (n * ho) % rpc != 0
            hit["straddles"] |= rpc > 1 and n > 1 and ho % rpc != 0
        # both forms (conv_wgrad_kernel, conv_wgrad16_kernel) run every case of the row: tests/test_conv_backward.py
        assert all(hit.values()), ((k, s), hit)
    # the rows per chunk that the 3x3 stride-2 layers of the 512 x 640 training step run are among the cases
    train = T.FULL_FRAME[(512, 640)]
    for name, _, ci, co, k, s, _ in T.LAYERS:
        if (k, s) == (3, 2):
            assert train[name]["wgrad"][1] in {rpc for _, _, rpc in T.CB_WGRAD_NEW[(3, 2)]}, name


def test_instance_norm_cases_select_their_instances_and_none_is_left_out():
    for what, table in (("instance_norm", T.IN_FWD_TABLE), ("instance_norm_backward", T.IN_BWD_TABLE)):
        assert set(table) == {(256, 8), (256, 20), (512, 40), (0, 0)}
        for inst, entries in table.items():
            assert entries, (what, inst)
            for e in entries:
                assert plan(what, *T.instance_norm_args(e), n=2) == inst, (what, e)
        # both ends of every range, and what falls out of the register-cached form
        for n, inst in ((4, (256, 8)), (8192, (256, 8)), (8196, (256, 20)), (20480, (256, 20)), (20484, (512, 40)), (81920, (512, 40)),
                        (81924, (0, 0)), (20478, (0, 0))):
            assert plan(what, n, 1, n=2) == inst, (what, n)
        assert plan(what, 20480, 0, n=2) == (0, 0)
    assert sorted(map(str, T.flat(T.IN_BWD_TABLE))) == sorted(map(str, T.IN_BWD_OLD + T.IN_BWD_NEW))


def test_window_attention_cases_select_their_instances():
    assert set(T.WA_TABLE) == {4, 2}
    for inst, cases in T.WA_TABLE.items():
        assert cases, inst
        for b, h, w, splits, min4 in cases:
            if min4 is None:
                assert plan("window_attention", b, h, w, splits, n=1) == (inst,), (b, h, w, splits)
            else:
                with hip.knob("wa_min4", min4):
                    assert plan("window_attention", b, h, w, splits, n=1) == (inst,), (b, h, w, splits, min4)
                assert plan("window_attention", b, h, w, splits, n=1) == (2,)  # without the knob the small case takes <2>
    # the <4> instances see a partly dead last query block and key tile in the forced and in the natural case
    for b, h, w, splits, _ in (T.WA_FORCED4, T.WA_NATURAL4):
        lw = (h // splits) * (w // splits)
        assert lw % 128 and lw % 64
    b, h, w, splits, _ = T.WA_NATURAL4
    assert -(-(h // splits) * (w // splits) // 128) * splits * splits * b >= 200
    # the threshold itself: 200 workgroups of 128 queries
    assert plan("window_attention", 50, 16, 16, 2, n=1) == (4,) and plan("window_attention", 49, 16, 16, 2, n=1) == (2,)


@pytest.mark.parametrize("frame", sorted(T.FULL_FRAME))
def test_what_a_full_frame_selects_layer_by_layer(frame):
    """a 3-view encoder pass and training step at 512 x 640 and 800 x 800: the expected selection is written out per layer in
    launch_plan_tables.FULL_FRAME, so that a tuned threshold shows as a diff there"""
    H, W = frame
    want = T.FULL_FRAME[frame]
    down = lambda v: (v - 1) // 2 + 1
    size = {1: (H, W)}
    for d in (2, 4, 8):
        size[d] = (down(size[d // 2][0]), down(size[d // 2][1]))
    assert plan("conv_gemm", 1, 3, 3, 64, H, W, 7, 2)[:3] == want["stem_gemm_fwd"]
    got = {}
    for name, n, ci, co, k, s, div in T.LAYERS:
        h, w = size[div]
        cl, up = name in ("featup.conv_l2rs.0", "featup.conv_ls.0"), name == "featup.conv_ls.0"
        hi, wi = (h // 2, w // 2) if up else (h, w)   # conv_ls reads the tokens through the nearest 2x up-sampling
        inference = plan("conv2d", ci, co, k, s, n, hi, wi, int(cl), int(up))
        assert inference[3] == 1 and plan("conv2d", ci, co, k, s, n, h, w, 0, 0)[:2] == inference[:2]
        got[name] = dict(conv2d=inference[:3], gemm_fwd=plan("conv_gemm", 1, n, ci, co, h, w, k, s)[:2],
                         gemm_bwd=plan("conv_gemm", 0, n, ci, co, h, w, k, s)[:2], wgrad=plan("conv_wgrad", n, ci, co, h, w, k, s, n=2))
        assert got[name] == want[name], (name, got[name], want[name])
    for c, div in ((64, 2), (96, 4), (128, 8)):
        h, w = size[div]
        for what in ("instance_norm", "instance_norm_backward"):
            assert plan(what, h * w, 1, n=2) == want["instance_norm"][c], (what, c)
    h, w = size[8]
    assert plan("window_attention", 6, h, w, 2, n=1) == (want["window_attention"],)
    # and every selection of the frame has a parity case
    for name, sel in got.items():
        assert sel["conv2d"] + (1,) in T.CONV2D_TABLE and sel["gemm_bwd"] in T.CB_DATA_TABLE and sel["gemm_fwd"] + (0,) in T.CB_FWD_TABLE


def test_the_query_refuses_what_it_does_not_know():
    with pytest.raises(hip.MnerfError, match="unknown dispatcher"):
        plan("no_such_launch", 1)
    with pytest.raises(hip.MnerfError):
        plan("conv_gemm", 0, 1, 64, 64, 8, 8)          # an argument short
    with pytest.raises(hip.MnerfError):
        plan("conv_wgrad", 1, 64, 64, 8, 8, 3, 1, n=1)  # room for one value of two
    with pytest.raises(hip.MnerfError):
        plan("conv_gemm", 0, 1, 3, 64, 8, 8, 7, 2)     # the data gradient has no 3-channel form
