"""The convolution plans (vbg.ops.ConvPlan, DESIGN.md "Convolution plans") without a GPU: the launch trace recorded before the plans
existed replays entry for entry, the plans say who wants an amax word, and the BatchNorm route of ConvBnFn.forward names what the nested
branches it replaced chose."""
import itertools
import json
import os
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gen():
    sys.path.insert(0, GOLDEN)
    try:
        import make_golden_conv_trace as m
    finally:
        sys.path.remove(GOLDEN)
    return m


@pytest.fixture
def defaults():
    """the switches the plan tests below assume, whatever the environment set; what was found is put back"""
    from vbg import ops
    boxes = (ops._CONV3, ops._CONV3_F16, ops._CONV3_SPLITK, ops._AMP_FAST, ops._CONV3_MIN_TILES, ops._CONV3_MIN_TILES_FWD, ops._CONV3_MIN_TILES_BWD,
             ops._CONV3W_MIN)
    was = [b[0] for b in boxes]
    for b, v in zip(boxes, (True, True, True, True, 480, 256, 0, 8)):
        b[0] = v
    yield
    for b, v in zip(boxes, was):
        b[0] = v


def test_launch_trace_replays(gen, defaults):
    """every call of tests/golden/conv_launch_trace.json -- each route's shape and each convolution of the bench step, under each switch,
    with and without a filter owner -- reaches the same leaf wrappers in the same order with the same kernel-selecting arguments"""
    from vbg import functions as Fn
    from vbg import ops
    with open(os.path.join(GOLDEN, "conv_launch_trace.json")) as f:
        want = gen.unpack(json.load(f))
    got = json.loads(json.dumps(gen.trace(ops, Fn)))
    assert sorted(got) == sorted(want)
    assert len(want) > 1000 and {e[0] for log in want.values() for e in log} >= {"conv3x3", "conv3x3_wgrad", "conv3x3_wflip", "conv3_planes", "amax",
                                                                                  "im2col", "gemm_raw", "zero_"}
    for key in sorted(want):
        assert len(got[key]) == len(want[key]), (key, got[key], want[key])
        for i, (a, b) in enumerate(zip(got[key], want[key])):
            assert a == b, (key, i, a, b)


def test_switches_are_left_as_found(gen):
    from vbg import ops
    before = (ops._CONV3[0], ops._CONV3_F16[0], ops._CONV3_SPLITK[0], ops._AMP_FAST[0], ops.amp_enabled(), ops.deterministic_active())
    for name in gen.SETTINGS:
        with gen.setting(ops, name):
            pass
    assert before == (ops._CONV3[0], ops._CONV3_F16[0], ops._CONV3_SPLITK[0], ops._AMP_FAST[0], ops.amp_enabled(), ops.deterministic_active())


WIDE = (1, 128, 128, 256, 128, 3, 3, 1, 1)          # B, H, W, Cin, Cout, kh, kw, stride, pad: row-reuse forward, input and weight gradient
LATE = (8, 32, 32, 256, 256, 3, 3, 1, 1)


def test_wants_amax_one_case_per_plan_kind(defaults):
    """only a product that scales a GRADIENT operand wants the word: the fp16 form of the row-reuse input / weight gradient"""
    from vbg import ops
    fwd, dgrad, wgrad = ops.conv_fwd_plan, ops.conv_dgrad_plan, ops.conv_wgrad_plan
    assert fwd(*WIDE) == ops.ConvPlan("conv3", True, planes="plain") and fwd(*WIDE, True) == ops.ConvPlan("conv3", True, planes="plain", fuse_stats=True)
    assert dgrad(*WIDE) == ops.ConvPlan("conv3", True, planes="plain", wants_amax=True)
    assert wgrad(*WIDE) == ops.ConvPlan("conv3", True, wants_amax=True)
    assert fwd(*LATE, True) == ops.ConvPlan("conv3", True, 64, 1, "late", fuse_stats=True) and not fwd(*LATE, True).wants_amax
    assert dgrad(*LATE) == ops.ConvPlan("conv3", True, 64, 1, "late", wants_amax=True)
    assert dgrad(1, 32, 32, 256, 256, 3, 3, 1, 1) == ops.ConvPlan("conv3", True, 64, 4, "late", wants_amax=True)
    g1, g3, stem = (1, 16, 16, 64, 32, 1, 1, 1, 0), (1, 16, 16, 16, 32, 3, 3, 2, 1), (1, 32, 32, 3, 64, 7, 7, 2, 3)
    for plan in (fwd, dgrad, wgrad):
        assert plan(*g1).kernel == "gemm1x1" and not plan(*g1).wants_amax
        assert plan(*g3).kernel == "gemm_conv" and not plan(*g3).wants_amax
    assert fwd(*stem).kernel == wgrad(*stem).kernel == "im2col" and not fwd(*stem).wants_amax and not wgrad(*stem).wants_amax
    assert not fwd(1, 16, 16, 512, 512, 3, 3, 1, 1, True).fuse_stats and fwd(*g1, True).fuse_stats and not fwd(*g1).fuse_stats         # (K = 4608 on 8 tiles: one the library splits)
    # the row-reuse kernels in their six-product form take no scale ...
    big = (8, 128, 128, 256, 256, 3, 3, 1, 1)          # (without the fp16 form the forward, too, asks for 480 tiles)
    was = ops._CONV3_F16[0]
    ops.set_conv3_f16(False)
    try:
        assert dgrad(*big) == ops.ConvPlan("conv3") and wgrad(*big) == ops.ConvPlan("conv3") and fwd(*big, True) == ops.ConvPlan("conv3", fuse_stats=True)
        assert fwd(*WIDE).kernel == "gemm_conv"
    finally:
        ops.set_conv3_f16(was)
    # ... and the statistics are never fused in deterministic mode (read at call time, like every switch)
    with ops.deterministic_scope(True):
        assert not fwd(*WIDE, True).fuse_stats
    assert fwd(*WIDE, True).fuse_stats


def test_every_switch_of_the_memo_key_acts_on_a_cached_shape(defaults):
    """the plans are memoised per (shape, ops._plan_switches()): each of its ten switches is flipped on shapes whose plans are already
    cached, and the plan must follow at once, and come back with the switch"""
    from vbg import ops
    fwd, dgrad, wgrad = ops.conv_fwd_plan, ops.conv_dgrad_plan, ops.conv_wgrad_plan
    big, last = (8, 128, 128, 256, 256, 3, 3, 1, 1), (8, 16, 16, 512, 512, 3, 3, 1, 1)

    def plans():
        return [f(*s) for s in (WIDE, LATE, big, last) for f in (lambda *a: fwd(*a, True), dgrad, wgrad)]

    warm = plans()
    assert plans() == warm and len(ops._plan_switches()) == 10

    def flipped(box, value, changed):
        """`changed()` holds only while box[0] is `value`"""
        assert not changed()
        was, box[0] = box[0], value
        try:
            assert changed(), (box, value)
        finally:
            box[0] = was
        assert not changed() and plans() == warm

    flipped(ops._CONV3, False, lambda: fwd(*WIDE).kernel == "gemm_conv" and wgrad(*WIDE).kernel == "gemm_conv")
    flipped(ops._CONV3_F16, False, lambda: dgrad(*big) == ops.ConvPlan("conv3"))
    flipped(ops._CONV3_SPLITK, False, lambda: fwd(*LATE).bn == 0 and fwd(*last).kernel == "gemm_conv")
    flipped(ops._SPLIT3, False, lambda: dgrad(*big).kernel == "gemm_conv")                    # set_precision("fp32")
    flipped(ops._DET, True, lambda: not fwd(*WIDE, True).fuse_stats)
    flipped(ops._CONV3_MIN_TILES, 10 ** 6, lambda: dgrad(*big).kernel == "gemm_conv")
    flipped(ops._CONV3_MIN_TILES_FWD, 10 ** 6, lambda: fwd(*big).kernel == "gemm_conv")
    flipped(ops._CONV3_MIN_TILES_BWD, 10 ** 6, lambda: dgrad(*big).kernel == "gemm_conv")
    flipped(ops._CONV3W_MIN, 10 ** 6, lambda: wgrad(*big).kernel == "gemm_conv")
    # the fifth entry of the key: an autocast region with the fast kernels' one-product forms off
    assert wgrad(*big).kernel == "conv3"
    with ops.amp_scope(True):
        assert wgrad(*big).kernel == "conv3"
        flipped(ops._AMP_FAST, False, lambda: wgrad(*big).kernel == "gemm_conv" and fwd(*big).kernel == "gemm_conv")
    assert plans() == warm


def test_the_stem_directly_with_and_without_a_col_buffer(gen):
    """ops.conv2d_fwd / conv2d_wgrad on 3 input channels: they build the col buffer themselves unless handed one, and the weight gradient
    takes the split-k / zero / accumulate rule of every other generic product"""
    import torch
    from vbg import ops
    from vbg.lib import OP_DENSE_K, OP_DENSE_R
    meta = dict(device="meta", dtype=torch.float32)
    x, w, dy = torch.empty((2, 32, 32, 3), **meta), torch.empty((64, 7, 7, 3), **meta), torch.empty((2, 16, 16, 64), **meta)
    M, K, Kp = 2 * 16 * 16, 147, 148
    sk = ops._pick_splitk(64, K, M)

    def run(thunk):
        log = []
        with gen.recorders(ops, log), torch.no_grad():
            thunk()
        return [[n, {k: v for k, v in a.items() if k in ("Kpad", "mnk", "ld", "a_kind", "b_kind", "accumulate", "splitk", "f16", "geo")}] for n, a in log]

    im2col = ["im2col", dict(Kpad=Kp)]
    fwd = ["gemm_raw", dict(mnk=[M, 64, K], ld=[Kp, K, 64], a_kind=OP_DENSE_K, b_kind=OP_DENSE_K, accumulate=False, splitk=1, f16=False, geo=None)]
    assert run(lambda: ops.conv2d_fwd(x, w, 2, 3)) == [im2col, fwd]
    col = torch.empty((M, Kp), **meta)
    assert run(lambda: ops.conv2d_fwd(x, w, 2, 3, col=col)) == [fwd]
    for acc in (False, True):
        wg = ["gemm_raw", dict(mnk=[64, K, M], ld=[64, Kp, K], a_kind=OP_DENSE_R, b_kind=OP_DENSE_R, accumulate=acc or sk > 1, splitk=sk, f16=False, geo=None)]
        zero = [["zero_", {}]] if (sk > 1 and not acc) else []
        assert run(lambda: ops.conv2d_wgrad(dy, x, torch.empty((64, 7, 7, 3), **meta), 2, 3, accumulate=acc)) == [im2col] + zero + [wg]
        assert run(lambda: ops.conv2d_wgrad(dy, x, torch.empty((64, 7, 7, 3), **meta), 2, 3, accumulate=acc, col=col)) == zero + [wg]


def test_predicates_are_the_plans(defaults):
    """the predicates that tools and tests call say what the plans say (their argument order: the convolution's own Cin / Cout for the
    weight gradient, swapped for the input gradient)"""
    from vbg import ops
    shapes = [WIDE, LATE, (1, 128, 128, 128, 128, 3, 3, 1, 1), (2, 128, 128, 64, 64, 3, 3, 1, 1), (480, 7, 7, 128, 128, 3, 3, 1, 1),
              (8, 128, 128, 32, 64, 3, 3, 1, 1), (1, 16, 16, 64, 32, 1, 1, 1, 0), (8, 64, 64, 128, 256, 3, 3, 1, 1)]
    for B, H, W, Ci, Co, kh, kw, s, p in shapes:
        d, w, f = ops.conv_dgrad_plan(B, H, W, Ci, Co, kh, kw, s, p), ops.conv_wgrad_plan(B, H, W, Ci, Co, kh, kw, s, p), ops.conv_fwd_plan(B, H, W, Ci, Co, kh, kw, s, p, True)
        assert ops.conv3_f16_bwd_ok(B, H, W, Co, Ci, kh, kw, s, p) == d.wants_amax == (ops._CONV3_F16[0] and ops.conv3_ok(B, H, W, Co, Ci, kh, kw, s, p))
        assert ops.conv3_f16_wgrad_ok(B, H, W, Ci, Co, kh, kw, s, p) == w.wants_amax == (ops._CONV3_F16[0] and ops.conv3w_ok(B, H, W, Ci, Co, kh, kw, s, p))
        assert (f.kernel == "conv3") == ops.conv3_ok(B, H, W, Ci, Co, kh, kw, s, p, fwd=True)
        assert (d.kernel == "conv3") == ops.conv3_ok(B, H, W, Co, Ci, kh, kw, s, p) and (w.kernel == "conv3") == ops.conv3w_ok(B, H, W, Ci, Co, kh, kw, s, p)
        Ho, Wo = ops.conv_out_hw(H, W, kh, s, p)
        assert f.fuse_stats == ops.fuse_stats_ok(B * Ho * Wo, Co, kh * kw * Ci)


def _route_of_the_nested_branches(ops, training, sync, C, needs_input_grad):
    """ConvBnFn.forward's BatchNorm branches as they stood before bn_route, returning the name of the leaf they reach"""
    fold = training and ops.bn_fold_ok(C, sync)
    if ops.bn_epilogue_route(training, needs_input_grad, sync):
        return "epilogue"
    if fold:
        return "fold"
    else:
        if training:
            if sync:
                if ops.bn_fold_ok(C):
                    return "sync_fold"
                else:
                    return "sync"
            else:
                return "stats"
        else:
            return "frozen"


def test_bn_route_truth_table():
    from vbg import functions as Fn
    from vbg import ops
    none, some = (False,) * 14, (True,) + (False,) * 13
    was = ops.bn_epilogue_enabled()
    try:
        for epi in (False, True):
            ops.set_bn_epilogue(epi)
            for training, sync, C, nig in itertools.product((False, True), (False, True), (64, 128, 32, 40, 3), (none, some)):
                assert Fn.bn_route(training, sync, C, nig) == _route_of_the_nested_branches(ops, training, sync, C, nig), (epi, training, sync, C, nig)
        # ... and the table itself, row by row: (epilogue switch, training, sync, C, a backward will come) -> route
        rows = [(True, False, False, 64, False, "epilogue"), (True, False, False, 40, False, "epilogue"), (True, False, False, 64, True, "frozen"),
                (True, False, True, 64, False, "frozen"), (True, True, False, 64, False, "fold"), (False, False, False, 64, False, "frozen"),
                (False, False, True, 64, True, "frozen"), (False, True, False, 64, True, "fold"), (False, True, False, 128, False, "fold"),
                (False, True, False, 40, True, "stats"), (False, True, True, 64, True, "sync_fold"), (False, True, True, 40, True, "sync")]
        for epi, training, sync, C, grad, want in rows:
            ops.set_bn_epilogue(epi)
            assert Fn.bn_route(training, sync, C, some if grad else none) == want, (epi, training, sync, C, grad)
    finally:
        ops.set_bn_epilogue(was)


def test_functions_ask_the_plans_only():
    """vbg/functions.py calls none of the shape / switch predicates the plans are built from: what a node needs to know it reads off a plan"""
    import re
    from vbg import functions as Fn
    with open(Fn.__file__) as f:
        src = f.read()
    names = ("conv3_ok", "conv3w_ok", "conv3_late_choice", "conv3_pw_ok", "conv3_split", "conv3_f16_bwd_ok", "conv3_f16_wgrad_ok", "conv3_f16_enabled",
             "conv3_f16_bwd_enabled", "fuse_stats_ok")
    assert not [n for n in names if re.search(r"\bops\." + n + r"\b", src)]
