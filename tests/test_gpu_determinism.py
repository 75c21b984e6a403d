"""Deterministic mode (vbg.ops.set_deterministic / VBG_DETERMINISTIC / torch.use_deterministic_algorithms): identical training steps
return identical bits (torch.equal, no tolerance), no launch of the step takes a float-atomic form, and each fixed-order kernel form
agrees with an fp64 restatement of what it computes."""
import os
import pathlib
import random
import tempfile

import numpy as np
import pytest
import torch

from test_gpu_model import build_product, load_synth, to_dev
from test_oracle_golden import _e2e_inputs, e2e_cfg
from vbg import ops
from vbg.optim import FusedAdamW, FusedSGD, clip_grad_norm_, split_parameters

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda")
AMP = {"fp32": None, "amp_fp16": torch.float16, "amp_bf16": torch.bfloat16}


def _e2e_batch():
    g = np.load(os.path.join(ROOT, "tests", "golden", "e2e.npz"))
    return to_dev(_e2e_inputs(g), DEV)


def _fresh(dropout=0.1):
    cfg = e2e_cfg("resnet_18_fpn")
    net = build_product(pathlib.Path(tempfile.mkdtemp(prefix="vbg_det_")), "resnet_18_fpn", cfg, layers=2, dropout=dropout)
    torch.manual_seed(0)
    load_synth(net, cfg, 1200)
    return net.to(DEV).train()


def _run(batch, amp_dtype, steps=2):
    """one fresh model, `steps` fused-optimizer steps -> list of flat snapshots (loss, clip norm, grads, params after step)"""
    net = _fresh()
    cnn, bert = split_parameters(net)
    opts = [FusedSGD(cnn, DEV, lr=1e-3, momentum=0.9), FusedAdamW(bert, DEV, lr=1e-4)]
    out = []
    for s in range(steps):
        for o in opts:
            o.zero_grad()
        net.BERTgrid_generator._step_seed = 41 + s
        random.seed(7 + s)
        torch.manual_seed(11 + s)
        with torch.autocast("cuda", dtype=amp_dtype or torch.float16, enabled=amp_dtype is not None):
            loss = net(*batch)
        loss.backward()
        norm = clip_grad_norm_(opts, 2.0)
        grads = [o.group.gflat.clone() for o in opts]
        for o in opts:
            o.step()
        torch.cuda.synchronize()
        out.append((loss.detach().clone(), norm, grads, [o.group.pflat.clone() for o in opts]))
    return out


def _assert_equal_runs(a, b):
    for (la, na, ga, pa), (lb, nb, gb, pb) in zip(a, b):
        assert torch.equal(la, lb), (float(la), float(lb))
        assert na == nb, (na, nb)
        for x, y in zip(ga, gb):
            assert torch.equal(x, y), float((x - y).norm() / x.norm().clamp_min(1e-30))
        for x, y in zip(pa, pb):
            assert torch.equal(x, y), float((x - y).norm() / x.norm().clamp_min(1e-30))


@pytest.mark.parametrize("form", list(AMP))
def test_step_is_bitwise_reproducible(form):
    batch = _e2e_batch()
    with ops.deterministic_scope(True):
        runs = [_run(batch, AMP[form]) for _ in range(3)]
    _assert_equal_runs(runs[0], runs[1])
    _assert_equal_runs(runs[0], runs[2])


def _step_keys(det, amp_dtype=None):
    batch = _e2e_batch()
    net = _fresh()
    cnn, bert = split_parameters(net)
    opts = [FusedSGD(cnn, DEV, lr=1e-3), FusedAdamW(bert, DEV, lr=1e-4)]
    log = ops.dispatch_log(True)
    try:
        with ops.deterministic_scope(det):
            random.seed(7)
            with torch.autocast("cuda", dtype=amp_dtype or torch.float16, enabled=amp_dtype is not None):
                loss = net(*batch)
            loss.backward()
            clip_grad_norm_(opts, 2.0)
        torch.cuda.synchronize()
        return dict(log)
    finally:
        ops.dispatch_log(False)
        ops.set_pair(os.environ.get("VBG_PAIR", "1") != "0", force=False)


# the fixed-order form that replaces each float-atomic site (the fused BN-statistics epilogues are not fused in the mode: bn_stats runs)
DET_OF = {"gemm_stats": "bn_reduce", "conv3_stats": "bn_reduce"}


def _assert_covered(on, off):
    """mode on: no float-atomic form; every site the same work reaches in the default mode has its det:* form in the on log"""
    assert not [k for k in on if k.startswith("fatomic:")], sorted(on)
    sites = [k[len("fatomic:"):] for k in off if k.startswith("fatomic:")]
    assert sites, sorted(off)                                   # the tags are live
    for site in sites:
        assert "det:" + DET_OF.get(site, site) in on, (site, sorted(on))
    assert not [k for k in off if k.startswith("det:")], sorted(off)


@pytest.mark.parametrize("amp", [False, True])
def test_no_float_atomics_in_deterministic_mode(amp):
    dt = torch.float16 if amp else None
    on = _step_keys(True, dt)
    for k in ("det:roi_align_bwd", "det:ce_bwd", "det:embed_ln_bwd", "det:bn_reduce", "det:sum", "det:sumsq"):
        assert k in on, (k, sorted(on))
    _assert_covered(on, _step_keys(False, dt))


def test_torch_flag_turns_it_on():
    prev = torch.are_deterministic_algorithms_enabled()
    assert not ops._DET_USER[0]
    try:
        torch.use_deterministic_algorithms(True)
        keys = _step_keys_flag_only()
        assert not [k for k in keys if k.startswith("fatomic:")], sorted(keys)
        assert "det:roi_align_bwd" in keys and "det:ce_bwd" in keys, sorted(keys)
    finally:
        torch.use_deterministic_algorithms(prev)
        ops._set_det_active(ops._DET_USER[0])


def _step_keys_flag_only():
    batch = _e2e_batch()
    net = _fresh()
    cnn, bert = split_parameters(net)
    opts = [FusedSGD(cnn, DEV, lr=1e-3), FusedAdamW(bert, DEV, lr=1e-4)]
    log = ops.dispatch_log(True)
    try:
        random.seed(7)
        loss = net(*batch)
        loss.backward()
        clip_grad_norm_(opts, 2.0)
        for o in opts:
            o.step()
        torch.cuda.synchronize()
        return dict(log)
    finally:
        ops.dispatch_log(False)
        ops.set_pair(os.environ.get("VBG_PAIR", "1") != "0", force=False)


# ---- kernel forms against fp64 restatements; two launches bitwise equal -----------------------------------------------------------
def _twice(fn):
    a, b = fn(), fn()
    assert torch.equal(a, b)
    return a


def _roi_bwd_ref(dy, shape, boxes, doc, out, scale):
    """fp64 restatement of torchvision RoIAlign backward (aligned=False, sampling_ratio=-1) on the NHWC map"""
    B, H, W, C = shape
    df = torch.zeros((B, H, W, C), dtype=torch.float64)
    dy = dy.double().cpu()
    for r in range(boxes.shape[0]):
        x1, y1, x2, y2 = [float(np.float32(v) * np.float32(scale)) for v in boxes[r].tolist()]
        rw, rh = max(x2 - x1, 1.0), max(y2 - y1, 1.0)
        bh, bw = rh / out, rw / out
        gh, gw = int(np.ceil(rh / out)), int(np.ceil(rw / out))
        cnt = max(gh * gw, 1)
        for ph in range(out):
            for pw in range(out):
                g = dy[r, ph * out + pw] / cnt
                for iy in range(gh):
                    y = y1 + ph * bh + (iy + 0.5) * bh / gh
                    for ix in range(gw):
                        x = x1 + pw * bw + (ix + 0.5) * bw / gw
                        if y < -1.0 or y > H or x < -1.0 or x > W:
                            continue
                        yy, xx = max(y, 0.0), max(x, 0.0)
                        y0, x0 = int(yy), int(xx)
                        if y0 >= H - 1:
                            y0 = y1_ = H - 1
                            yy = float(y0)
                        else:
                            y1_ = y0 + 1
                        if x0 >= W - 1:
                            x0 = x1_ = W - 1
                            xx = float(x0)
                        else:
                            x1_ = x0 + 1
                        ly, lx = yy - y0, xx - x0
                        hy, hx = 1 - ly, 1 - lx
                        b = int(doc[r])
                        df[b, y0, x0] += hy * hx * g
                        df[b, y0, x1_] += hy * lx * g
                        df[b, y1_, x0] += ly * hx * g
                        df[b, y1_, x1_] += ly * lx * g
    return df


def test_deterministic_kernels_vs_fp64_roi_align_bwd():
    torch.manual_seed(0)
    B, H, W, C, out = 2, 40, 56, 64, 7
    boxes = [[0, 0, 220, 150], [4, 8, 40, 20], [4, 8, 40, 20], [30, 30, 31, 31], [-20, -10, 60, 30], [200, 140, 300, 200],
             [10, 12, 100, 30], [12, 10, 90, 40], [0, 0, 0, 0], [100, 60, 224, 160]]
    doc = [0, 0, 0, 1, 1, 0, 1, 1, 0, 1]
    bx = torch.tensor(boxes, dtype=torch.int32, device=DEV)
    bd = torch.tensor(doc, dtype=torch.int32, device=DEV)
    dy = torch.randn((len(boxes), out * out, C), device=DEV)

    def go():
        df = torch.zeros((B, H, W, C), device=DEV)
        with ops.deterministic_scope(True):
            ops.roi_align_bwd(dy, (B, H, W, C), bx, bd, out, 0.25, df)
        torch.cuda.synchronize()
        return df
    got = _twice(go).double().cpu()
    ref = _roi_bwd_ref(dy, (B, H, W, C), bx.cpu(), bd.cpu(), out, 0.25)
    assert float((got - ref).abs().max()) <= 1e-4 * max(1.0, float(ref.abs().max()))


def test_deterministic_kernels_vs_fp64_rows_add_sorted():
    """embedding / gather_rows backward form: repeated ids, one id repeated 3000 times (the skew case)"""
    torch.manual_seed(1)
    n, C, V = 5000, 96, 300
    idx = torch.randint(0, V, (n,), dtype=torch.int32)
    idx[:3000] = 17
    idx = idx[torch.randperm(n)]
    src = torch.randn((n, C), device=DEV)
    idx_d = idx.to(DEV)

    def go():
        dst = torch.ones((V, C), device=DEV)
        with ops.deterministic_scope(True):
            ops.scatter_rows_add(src, idx_d, dst)
        torch.cuda.synchronize()
        return dst
    got = _twice(go).double().cpu()
    ref = torch.ones((V, C), dtype=torch.float64).index_add_(0, idx.long(), src.double().cpu())
    assert float((got - ref).abs().max()) <= 1e-4 * float(ref.abs().max())


def test_deterministic_kernels_vs_fp64_ce_bwd():
    """up_shift > 0 (four pixels per logits row) and repeated selections"""
    torch.manual_seed(2)
    B, H, W, ncls, up = 2, 32, 24, 5, 1
    rows = B * (H >> up) * (W >> up)
    logits = torch.randn((rows, ncls), device=DEV)
    labels = torch.randint(0, ncls, (B * H * W,), dtype=torch.int32, device=DEV)
    labels[::37] = ncls + 3                                   # out of range: skipped, as by the default form
    elem = torch.randint(0, B * H * W, (3000,), dtype=torch.int32, device=DEV)
    elem[:500] = 5
    gdev = torch.tensor([0.37], device=DEV)

    def go():
        dl = torch.zeros_like(logits)
        with ops.deterministic_scope(True):
            ops.ce_bwd(logits, elem, labels, elem.numel(), None, gdev, 0.5, up, H, W, dl)
        torch.cuda.synchronize()
        return dl
    got = _twice(go).double().cpu()
    e = elem.long().cpu()
    x = e % W
    t = e // W
    y, b = t % H, t // H
    r = (b * (H >> up) + (y >> up)) * (W >> up) + (x >> up)
    lg = logits.double().cpu()[r]
    p = torch.softmax(lg, 1)
    lab = labels.long().cpu()[e]
    ok = lab < ncls
    oh = torch.nn.functional.one_hot(lab.clamp_max(ncls - 1), ncls).double()
    ref = torch.zeros((rows, ncls), dtype=torch.float64).index_add_(0, r[ok], (0.37 * 0.5 * (p - oh))[ok])
    assert float((got - ref).abs().max()) <= 1e-5 * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("shape", [(8 * 512, 768), (131072, 256), (3, 5), (0, 64)])
def test_deterministic_kernels_vs_fp64_colsum(shape):
    torch.manual_seed(3)
    x = torch.randn(shape, device=DEV) + 0.5

    def go():
        out = torch.full((shape[1],), 0.25, device=DEV)
        with ops.deterministic_scope(True):
            ops.colsum(x, out=out, accumulate=True)
        torch.cuda.synchronize()
        return out
    got = _twice(go).double().cpu()
    ref = x.double().cpu().sum(0) + 0.25
    assert float((got - ref).abs().max()) <= 1e-6 * max(1.0, float(ref.abs().max()))


def test_deterministic_kernels_vs_fp64_sums():
    torch.manual_seed(4)
    x = torch.randn((3_000_001,), device=DEV)

    def go(sq):
        out = torch.full((1,), 2.0, device=DEV)
        with ops.deterministic_scope(True):
            (ops.sumsq if sq else ops.sum_f32)(x, out)
        torch.cuda.synchronize()
        return out
    for sq in (False, True):
        got = float(_twice(lambda: go(sq)))
        xd = x.double().cpu()
        ref = float((xd * xd).sum() if sq else xd.sum()) + 2.0
        assert abs(got - ref) <= 1e-5 * max(1.0, float((xd * xd).sum())), (sq, got, ref)


def test_deterministic_kernels_vs_fp64_bn_stats():
    torch.manual_seed(5)
    M, C = 70000, 64
    x = torch.randn((M, C), device=DEV) * 3 + 1

    def go():
        with ops.deterministic_scope(True):
            slots = ops.bn_stats(x, ops.bn_zero_slots(DEV, C))
            folded = ops.bn_fold(slots, C)
        torch.cuda.synchronize()
        return folded
    got = _twice(go).cpu()
    xd = x.double().cpu()
    ref = torch.cat([xd.sum(0), (xd * xd).sum(0)])
    assert float(((got - ref).abs() / ref.abs().clamp_min(1.0)).max()) <= 1e-6


def test_deterministic_kernels_vs_fp64_bn_bwd_reduce():
    torch.manual_seed(6)
    M, C = 90000, 128
    x = torch.randn((M, C), device=DEV)
    y = torch.relu(torch.randn((M, C), device=DEV))
    dy = torch.randn((M, C), device=DEV)
    mean, invstd = x.mean(0), 1.0 / (x.var(0) + 1e-5).sqrt()

    def go():
        with ops.deterministic_scope(True):
            slots = ops.bn_bwd_reduce(dy, y, x, mean, invstd, True, ops.bn_zero_slots(DEV, C))
            folded = ops.bn_fold(slots, C)
        torch.cuda.synchronize()
        return folded
    got = _twice(go).cpu()
    g = dy.double().cpu() * (y.cpu() > 0)
    xh = (x.double().cpu() - mean.double().cpu()) * invstd.double().cpu()
    ref = torch.cat([g.sum(0), (g * xh).sum(0)])
    assert float((got - ref).abs().max()) <= 1e-6 * float(ref.abs().max())


def test_deterministic_kernels_vs_atomic_form_embed_ln_bwd():
    """dz rows + block partials -> table rows by sorted id, (dgamma, dbeta, dtype0) by block: against the default atomic form (held to
    the reference by the encoder tests) and bitwise twice; word id 3 repeated 1500 times"""
    torch.manual_seed(7)
    ntok, hidden, V, npos = 2048, 768, 500, 512
    ids = torch.randint(0, V, (ntok,), dtype=torch.int32, device=DEV)
    ids[::2][:1500] = 3
    pos = (torch.arange(ntok, device=DEV) % npos).to(torch.int32)
    dout, xhat = torch.randn((ntok, hidden), device=DEV), torch.randn((ntok, hidden), device=DEV)
    rstd, gamma = torch.rand((ntok,), device=DEV) + 0.5, torch.randn((hidden,), device=DEV)

    def go(det):
        outs = [torch.zeros((V, hidden), device=DEV), torch.zeros((npos, hidden), device=DEV)] + [torch.zeros((hidden,), device=DEV) for _ in range(3)]
        with ops.deterministic_scope(det):
            ops.embed_ln_bwd(dout, xhat, rstd, ids, pos, gamma, 0.1, 5, 9, *outs)
        torch.cuda.synchronize()
        return torch.cat([o.view(-1) for o in outs])
    got = _twice(lambda: go(True))
    ref = go(False)
    assert float((got - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


def test_deterministic_kernels_vs_atomic_form_crf_nll_bwd():
    """per-document transition-gradient partials added in document order: against the default atomic form (held to the reference by
    the crf-head tests), bitwise twice; one empty document"""
    torch.manual_seed(8)
    ntag, lens = 9, [37, 0, 120, 5, 64]
    off = torch.tensor(np.cumsum([0] + lens), dtype=torch.int32, device=DEV)
    N = int(off[-1])
    em = torch.randn((N, ntag), device=DEV)
    tags = torch.randint(0, ntag - 2, (N,), dtype=torch.int32, device=DEV)
    trans = torch.randn((ntag, ntag), device=DEV)
    start, stop = ntag - 2, ntag - 1
    nll, alpha, logz = ops.crf_nll_fwd(em, tags, off, trans, start, stop)
    gout = torch.rand((len(lens),), device=DEV) + 0.5

    def go(det):
        dtrans = torch.full((ntag, ntag), 0.5, device=DEV)
        with ops.deterministic_scope(det):
            dem = ops.crf_nll_bwd(em, tags, off, trans, start, stop, alpha, logz, gout, dtrans)
        torch.cuda.synchronize()
        return torch.cat([dtrans.view(-1), dem.view(-1)])
    got = _twice(lambda: go(True))
    ref = go(False)
    assert float((got - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


# ---- two-stage heads, the stock loop, the benchmark's batch, parity ---------------------------------------------------------------
def _mode_step_grads(mode, tmp):
    from test_gpu_model import build_product_mode
    from test_oracle_golden import modes_state
    g = np.load(os.path.join(ROOT, "tests", "golden", "e2e_modes.npz"))
    cfg, sd = modes_state(g, mode)
    net = build_product_mode(pathlib.Path(tmp), mode, cfg)
    net.load_state_dict(sd, strict=False)
    net = net.to(DEV).train()
    batch = _e2e_batch()
    out = []
    for s in range(2):
        net.zero_grad(set_to_none=True)
        random.seed(7 + s)
        torch.manual_seed(11 + s)
        loss = net(*batch)
        loss.backward()
        torch.cuda.synchronize()
        out.append((loss.detach().clone(), [(n, None if p.grad is None else p.grad.clone()) for n, p in net.named_parameters()]))
    return out


def _mode_keys(mode, det):
    from test_gpu_model import build_product_mode
    from test_oracle_golden import modes_state
    g = np.load(os.path.join(ROOT, "tests", "golden", "e2e_modes.npz"))
    cfg, sd = modes_state(g, mode)
    net = build_product_mode(pathlib.Path(tempfile.mkdtemp(prefix="vbg_det_")), mode, cfg)
    net.load_state_dict(sd, strict=False)
    net = net.to(DEV).train()
    log = ops.dispatch_log(True)
    try:
        with ops.deterministic_scope(det):
            random.seed(7)
            net(*_e2e_batch()).backward()
        torch.cuda.synchronize()
        return dict(log)
    finally:
        ops.dispatch_log(False)
        ops.set_pair(os.environ.get("VBG_PAIR", "1") != "0", force=False)


@pytest.mark.parametrize("mode", ["full", "crf"])
def test_step_is_bitwise_reproducible_modes(mode):
    with ops.deterministic_scope(True):
        a = _mode_step_grads(mode, tempfile.mkdtemp(prefix="vbg_det_"))
        b = _mode_step_grads(mode, tempfile.mkdtemp(prefix="vbg_det_"))
    for (la, ga), (lb, gb) in zip(a, b):
        assert torch.equal(la, lb), (float(la), float(lb))
        for (n, x), (_, y) in zip(ga, gb):
            assert (x is None) == (y is None), n
            assert x is None or torch.equal(x, y), (n, float((x - y).abs().max()))


@pytest.mark.parametrize("mode", ["full", "crf"])
def test_no_float_atomics_in_deterministic_mode_heads(mode):
    on = _mode_keys(mode, True)
    _assert_covered(on, _mode_keys(mode, False))
    assert ("det:crf_nll_bwd" if mode == "crf" else "det:scatter_rows_add") in on, sorted(on)


def test_no_float_atomics_in_deterministic_mode_inference():
    net = _fresh(dropout=0.0).eval()
    imgs, segs, classes, coors, corpus, mask = _e2e_batch()
    outs = []
    log = ops.dispatch_log(True)
    try:
        with ops.deterministic_scope(True):
            for _ in range(2):
                with torch.no_grad():
                    outs.append(net.inference(imgs, segs, coors, corpus, mask).clone())
        torch.cuda.synchronize()
        on = dict(log)
    finally:
        ops.dispatch_log(False)
        ops.set_pair(os.environ.get("VBG_PAIR", "1") != "0", force=False)
    assert torch.equal(outs[0], outs[1])
    assert not [k for k in on if k.startswith("fatomic:")], sorted(on)


def _stock_run(tmp):
    net = _fresh()
    pc = [p for n, p in net.named_parameters() if "bert_model" not in n]
    pb = [p for n, p in net.named_parameters() if "bert_model" in n]
    oc = torch.optim.SGD(pc, lr=0.005, momentum=0.9, weight_decay=0.005)
    ob = torch.optim.AdamW(pb, lr=5e-5, weight_decay=0.01)
    scaler = torch.cuda.amp.GradScaler()
    batch = _e2e_batch()
    out = []
    for s in range(2):
        oc.zero_grad(set_to_none=True)
        ob.zero_grad(set_to_none=True)
        net.BERTgrid_generator._step_seed = 41 + s
        random.seed(7 + s)
        torch.manual_seed(11 + s)
        with torch.autocast("cuda", dtype=torch.float16):
            loss = net(*batch)
        scaler.scale(loss).backward()
        scaler.unscale_(oc)
        scaler.unscale_(ob)
        norm = torch.nn.utils.clip_grad_norm_(net.parameters(), max_norm=2)
        grads = [None if p.grad is None else p.grad.clone() for p in net.parameters()]
        scaler.step(oc)
        scaler.step(ob)
        scaler.update()
        torch.cuda.synchronize()
        out.append((loss.detach().clone(), norm.clone(), grads, [p.detach().clone() for p in net.parameters()]))
    return out


def test_stock_loop_bitwise_reproducible():
    with ops.deterministic_scope(True):
        a, b = _stock_run(None), _stock_run(None)
    for (la, na, ga, pa), (lb, nb, gb, pb) in zip(a, b):
        assert torch.equal(la, lb) and torch.equal(na, nb), (float(la), float(lb), float(na), float(nb))
        for x, y in zip(ga, gb):
            assert (x is None) == (y is None) and (x is None or torch.equal(x, y))
        for x, y in zip(pa, pb):
            assert torch.equal(x, y)


@pytest.mark.parametrize("amp", [False, True])
def test_cfg2_batch8_bitwise_reproducible(amp):
    """bench.py's model and batch: one step with every stream switch on is bitwise equal to the same step with them off, and to its own
    repeat (the mode fixes the placement: one stream); the float-atomic sites the default mode reaches at this size all take their
    fixed-order forms"""
    import contextlib
    import sys
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    from vbg.batch import PackedBatch

    with contextlib.redirect_stdout(sys.stderr):
        torch.manual_seed(42)
        net = bench.build_model(tempfile.mkdtemp(prefix="vbg_det_")).to(DEV).train()
    cnn, bert = split_parameters(net)
    opts = [FusedSGD(cnn, DEV, lr=0.0), FusedAdamW(bert, DEV, lr=0.0)]
    batch = PackedBatch.pack(*bench.synthetic_batch(8, 512, 512, 512, 128, bench.NCLS, bench.VOCAB, 1234)).to(DEV)
    gen = net.BERTgrid_generator
    was = (ops.overlap_enabled(), ops._CONV_WGRAD_STREAM[0])

    def one(streams, det=True, log=False):
        ops.set_overlap(streams)
        ops._CONV_WGRAD_STREAM[0] = 2 if streams else 0
        for o in opts:
            o.zero_grad()
        gen._step_seed = 0x5EED
        random.seed(7)
        seen = ops.dispatch_log(True) if log else None
        try:
            with ops.deterministic_scope(det):
                with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
                    loss = net(*batch)
                loss.backward()
            out = [o.group.gflat.clone() for o in opts]
            torch.cuda.synchronize()
        finally:
            if log:
                ops.dispatch_log(False)
        return loss.detach().clone(), out, (dict(seen) if log else None)

    try:
        one(True)                                              # warm-up: flat storage, plane images
        l1, g1, on = one(True, log=True)
        l0, g0, _ = one(False)
        assert torch.equal(l0, l1), (float(l0), float(l1))
        for x, y in zip(g0, g1):
            assert torch.equal(x, y), float((x - y).norm() / x.norm())
        l2, g2, _ = one(True)
        assert torch.equal(l1, l2) and all(torch.equal(x, y) for x, y in zip(g1, g2))
        _, _, off = one(True, det=False, log=True)
        _assert_covered(on, off)
        assert not ops.overlap_enabled() or not ops.deterministic_active()
    finally:
        ops.set_overlap(was[0])
        ops._CONV_WGRAD_STREAM[0] = was[1]


def test_deterministic_mode_keeps_parity_e2e(golden, tmp_path):
    import test_gpu_model as M
    with ops.deterministic_scope(True):
        M.test_e2e_vs_reference_golden_and_oracle(golden, tmp_path, "r18", "resnet_18_fpn")


@pytest.mark.parametrize("mode", ["full", "crf"])
def test_deterministic_mode_keeps_parity_modes(golden, tmp_path, mode):
    import test_gpu_model as M
    with ops.deterministic_scope(True):
        M.test_e2e_modes_vs_reference_golden_and_oracle(golden, tmp_path, mode)


def test_deterministic_mode_keeps_parity_cfg2e8(golden, tmp_path):
    import test_gpu_full_scale as F
    try:
        with ops.deterministic_scope(True):
            F.test_full_scale_every_gradient_vs_reference(golden, tmp_path, "cfg2e8")
    finally:
        ops.dispatch_log(False)
        ops.set_pair(os.environ.get("VBG_PAIR", "1") != "0", force=False)
