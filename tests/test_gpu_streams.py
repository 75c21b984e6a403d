"""The default side streams against the one-stream step AT THE BENCHMARK'S SIZE.

Round 5's committed evidence (profiles/r05_stream_race.txt line 10) held one run in 22 whose CNN gradients sat 7.9e-4 from the
one-stream step -- 700x the float-atomics noise floor -- with the convolution weight gradients on their own stream (the default).  Nothing
in the suite could see it: the toy test (r18, 96 x 128) never has three busy streams, and 7.9e-4 slides under the 1e-3 gates of the
full-scale fixtures.  Root cause (profiles/r06_stream_race.txt; NOT the amax slots VERDICT / ADVICE r5 suspected, though those are now
reserved for the side stream as well): the pipelined pre-split convolution kernel (csrc/conv3.hip, PW) read k-tile 0 of its filter
ring behind the prologue barrier and let the first k-tile of the loop refill the same stage with k-tile 4 -- no barrier in between; on
64-filter tiles (six MFMAs per k-tile) a wave that fell one k-tile behind multiplied the wrong filter slice.  It takes three busy streams.

test_default_streams_equal_one_stream_at_batch8 runs the cfg2 batch-8 step (bench.py's model and batch: resnet-34 + 12-layer BERT,
8 x 512 x 512) 48 times with every default stream on, with 16-slot amax pools (a pool then turns over ~20 times inside one backward
instead of once per step), against the same step on ONE stream from identical state, and gates at 1e-5 (noise floor 1.3e-6).  Without
the guard barrier this test failed on the GPU box (12 outliers in 160 runs); with it: 0 in 400."""
import contextlib
import os
import random
import sys
import tempfile

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


RUNS = int(os.environ.get("VBG_STREAM_TEST_RUNS", "48"))      # (the race sat in ~7 % of the steps: 48 runs see it with 97 %)


def test_default_streams_equal_one_stream_at_batch8():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    from vbg import ops
    from vbg.batch import PackedBatch
    from vbg.optim import FusedAdamW, FusedSGD, split_parameters
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from stream_race_check import group_report

    dev = torch.device("cuda", 0)
    with contextlib.redirect_stdout(sys.stderr):
        torch.manual_seed(42)
        net = bench.build_model(tempfile.mkdtemp(prefix="vbg_streams_")).to(dev).train()
    cnn, bert = split_parameters(net)
    opts = [FusedSGD(cnn, dev, lr=0.0), FusedAdamW(bert, dev, lr=0.0)]
    groups = [o.group for o in opts]
    batch = PackedBatch.pack(*bench.synthetic_batch(8, 512, 512, 512, 128, bench.NCLS, bench.VOCAB, 1234)).to(dev)
    gen = net.BERTgrid_generator
    was = (ops.overlap_enabled(), ops._CONV_WGRAD_STREAM[0], ops._AMAX_POOL_SLOTS[0])

    def one(streams):
        ops.set_overlap(streams)
        ops._CONV_WGRAD_STREAM[0] = 2 if streams else 0
        for o in opts:
            o.zero_grad()
        gen._step_seed = 0x5EED
        random.seed(7)
        loss = net(*batch)
        loss.backward()
        out = [o.group.gflat.clone() for o in opts]          # (enqueued right behind backward(): the end-of-backward join must cover it)
        torch.cuda.synchronize()
        return float(loss), out

    try:
        ops._AMAX_POOL_SLOTS[0] = 16
        ops._AMAX_POOL.clear()
        one(False)                                            # warm-up: flat storage, plane images
        l0, g0 = one(False)
        floor = [0.0, 0.0]
        for _ in range(2):                                    # the noise floor of the float atomics, for the record
            l, g = one(False)
            assert l == l0
            for k, (rl2, _, wp, _) in enumerate(group_report(groups, g0, g)):
                floor[k] = max(floor[k], rl2)
        worst = [(0.0, 0.0, "")] * 2
        for r in range(RUNS):
            l, g = one(True)
            assert l == l0, (r, l, l0)                        # the forward does not depend on the streams
            for k, (rl2, mx, wp, wn) in enumerate(group_report(groups, g0, g)):
                worst[k] = max(worst[k], (rl2, wp, wn))
                assert rl2 < 1e-5, f"run {r}: {('cnn', 'bert')[k]} gradients {rl2:.2e} from the one-stream step (noise floor {floor[k]:.1e}); worst parameter {wn} {wp:.2e}"
        print(f"default streams vs one stream, {RUNS} runs, 16-slot amax pools: cnn {worst[0][0]:.2e} (floor {floor[0]:.1e}; worst parameter {worst[0][2]} "
              f"{worst[0][1]:.2e}), bert {worst[1][0]:.2e} (floor {floor[1]:.1e}; worst parameter {worst[1][2]} {worst[1][1]:.2e})")
    finally:
        ops.set_overlap(was[0])
        ops._CONV_WGRAD_STREAM[0] = was[1]
        ops._AMAX_POOL_SLOTS[0] = was[2]
        ops._AMAX_POOL.clear()


def _ring_contention_mismatches(reps=400):
    """the 64-filter pipelined pre-split convolution (conv3x3_kernel<128, 64, true, 2>: six MFMAs per k-tile, the launches the round-5
    outlier sat in) `reps` times on one stream while two other streams keep the chip and the memory system busy; every output must
    equal the first BIT FOR BIT (same pieces, same products, same order).  -> number of launches whose output differs"""
    from vbg import ops
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(611)
    B, H, W, C = 8, 128, 128, 64
    dy = (torch.randn(B, H, W, C, generator=g) * 2.0 ** -20).to(dev)
    wd = (torch.randn(C, C, 3, 3, generator=g) / 24.0).to(dev).contiguous(memory_format=torch.channels_last)
    w4 = wd.permute(0, 2, 3, 1)
    am = ops.amax(dy)
    wpf = ops.conv3_planes(wd, w4, True)
    assert wpf is not None and ops.conv3_pw_ok(B, H, W, C, C)
    ref = ops.conv3x3(dy, w4, f16x2=True, x_amax=am, w_planes=wpf, n_out=C)
    torch.cuda.synchronize()
    # the neighbours: what shares the chip with these launches in a training step -- the same node's weight gradient (row-reuse kernel,
    # 256 strips, slabs) on one stream, large plane products on another
    x = torch.randn(B, H, W, C, generator=g).to(dev)
    xam = ops.amax(x)
    dw = torch.zeros((C, 3, 3, C), device=dev)
    a = ops.split_planes_pair(torch.randn(4128, 768, generator=g).to(dev))
    bq = ops.split_planes_pair(torch.randn(3072, 768, generator=g).to(dev))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    main = torch.cuda.current_stream()
    s1.wait_stream(main)
    s2.wait_stream(main)
    outs = []
    for r in range(reps):
        with torch.cuda.stream(s1):
            ops.conv3x3_wgrad(dy, x, dw, f16x2=True, dy_amax=am, x_amax=xam)
        with torch.cuda.stream(s2):
            ops.plane_gemm(a, bq, torch.empty((4128, 3072), device=dev), form=1, tile=ops.pair_tile(4128, 3072, True))
        outs.append(ops.conv3x3(dy, w4, f16x2=True, x_amax=am, w_planes=wpf, n_out=C))
        if len(outs) == 16 or r + 1 == reps:
            bad = getattr(_ring_contention_mismatches, "_bad", 0)
            for o in outs:
                bad += int(not torch.equal(o, ref))
            _ring_contention_mismatches._bad = bad
            outs = []
    torch.cuda.synchronize()
    bad = _ring_contention_mismatches._bad
    _ring_contention_mismatches._bad = 0
    return bad


def test_pipelined_conv3_ring_is_safe_under_contention():
    """Root cause of the round-5 outlier (csrc/conv3.hip, PW prologue): k-tile 0's fragments were read behind the prologue barrier
    and the first k-tile of the loop ended with the DMA of k-tile 4 into the same ring stage, with no barrier between the two -- a wave
    that fell one (six-MFMA) k-tile behind read the wrong filter slice.  With the guard barrier every one of 400 contended launches is
    bit-identical to the first."""
    assert _ring_contention_mismatches(400) == 0


def test_no_kernel_reads_memory_nobody_wrote():
    """In a loop of identical steps the caching allocator hands every call site the block it had one step earlier, so "uninitialised"
    memory holds exactly what the same tensor held before: a kernel that reads past what was written, or leaves part of its output
    unwritten, is invisible until the allocation pattern shifts (another batch, another stream holding blocks longer).  Here every
    fresh `torch.empty` / `empty_like` of the package is filled with NaN (ints: 0x7f7f7f7f) for one cfg2 batch-8 training step on ONE
    stream: loss and every gradient must equal the unpoisoned step's (tools/poison_check.py does the same site by site)."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench
    import poison_check as PC
    from vbg import ops
    from vbg.batch import PackedBatch
    from vbg.optim import FusedAdamW, FusedSGD, split_parameters

    dev = torch.device("cuda", 0)
    with contextlib.redirect_stdout(sys.stderr):
        torch.manual_seed(42)
        net = bench.build_model(tempfile.mkdtemp(prefix="vbg_poison_")).to(dev).train()
    cnn, bert = split_parameters(net)
    opts = [FusedSGD(cnn, dev, lr=0.0), FusedAdamW(bert, dev, lr=0.0)]
    batch = PackedBatch.pack(*bench.synthetic_batch(8, 512, 512, 512, 128, bench.NCLS, bench.VOCAB, 1234)).to(dev)
    gen = net.BERTgrid_generator
    was = (ops.overlap_enabled(), ops._CONV_WGRAD_STREAM[0])
    ops.set_overlap(False)
    ops._CONV_WGRAD_STREAM[0] = 0

    def one():
        for o in opts:
            o.zero_grad()
        gen._step_seed = 0x5EED
        random.seed(7)
        loss = net(*batch)
        loss.backward()
        out = [o.group.gflat.clone() for o in opts]
        torch.cuda.synchronize()
        return float(loss.detach()), out

    e0, e1 = torch.empty, torch.empty_like
    try:
        one()
        l0, g0 = one()
        torch.empty, torch.empty_like = PC._wrap(e0), PC._wrap(e1)
        PC.STATE["mode"] = "all"
        l1, g1 = one()
    finally:
        PC.STATE["mode"] = "off"
        torch.empty, torch.empty_like = e0, e1
        ops.set_overlap(was[0])
        ops._CONV_WGRAD_STREAM[0] = was[1]
    assert l1 == l0, (l1, l0)
    for o, a, b in zip(opts, g0, g1):
        assert int(torch.isnan(b).sum()) == 0
        grp = o.group
        for n, p, off in zip(grp.names, grp.params, grp.offsets):
            if "key.bias" in n:          # analytically zero (softmax is shift-invariant): what is there is rounding noise
                continue
            x, y = a[off:off + p.numel()], b[off:off + p.numel()]
            nx = float(x.norm())
            if nx > 0:
                assert float((x - y).norm()) / nx < 2e-5, n
