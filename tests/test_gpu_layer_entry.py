"""The one-call encoder layer (include/vbg.h vbg_bert_layer_fwd, csrc/encoder.hip) launches the same seven kernels with the same
descriptors as the per-launch path, vbg/ops.py bert_layer_launches: results must be BIT-identical in every form the layer runs
(three bf16 planes / fp16 pairs / the one-product forms of an autocast region; with and without dropout; training and inference), and
the entry must actually be the path taken.  Needs a real MI355X."""
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_model import build_product, load_synth, to_dev
from test_oracle_golden import _e2e_inputs, e2e_cfg

LAYERS = 2


def _net(tmp_path, dropout):
    cfg = e2e_cfg("resnet_18_fpn")
    net = build_product(tmp_path, "resnet_18_fpn", cfg, layers=LAYERS, dropout=dropout)
    load_synth(net, cfg, 1200)
    return net


def _batch(dev):
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "e2e.npz"))
    return to_dev(_e2e_inputs(g), dev)


@pytest.mark.parametrize("form", ["bf16x3", "pair", "amp"])
@pytest.mark.parametrize("dropout", [0.0, 0.1])
def test_training_step_is_bit_identical_through_the_layer_entry(tmp_path, form, dropout):
    from vbg import ops
    from vbg.optim import FusedAdamW, FusedSGD, split_parameters
    dev = torch.device("cuda")
    net = _net(tmp_path, dropout).to(dev).train()
    cnn, bert = split_parameters(net)
    opts = [FusedSGD(cnn, dev, lr=0.0), FusedAdamW(bert, dev, lr=0.0)]
    dbatch = _batch(dev)
    gen = net.BERTgrid_generator
    was_entry, was_overlap = ops._LAYER_ENTRY[0], ops.overlap_enabled()
    ops.set_overlap(False)                       # one stream: the comparison is about the launches, not their interleaving
    ops.set_pair(True, force=form != "bf16x3")   # (the fixture is smaller than the tiles the pair form waits for)
    if form == "bf16x3":
        ops.set_pair(False)
    res = {}
    try:
        for run, entry in enumerate((False, True, False)):
            ops.set_layer_entry(entry)
            for o in opts:
                o.zero_grad()
            gen._step_seed = 41
            random.seed(7)
            log = ops.dispatch_log(True)
            with torch.autocast("cuda", dtype=torch.float16, enabled=form == "amp"):
                loss = net(*dbatch)
            ops.dispatch_log(False)
            loss.backward()
            torch.cuda.synchronize()
            assert log.get("bert_layer_fwd:entry", 0) == (LAYERS if entry else 0), log
            want = {"bf16x3": "plane_gemm:bf16x3", "pair": "plane_gemm:pair", "amp": "plane_gemm:onep"}[form]
            assert log.get(want, 0) >= 3 * LAYERS, log
            res[run] = (float(loss.detach()), dict(log), [o.group.gflat.clone() for o in opts])
    finally:
        ops.set_layer_entry(was_entry); ops.set_overlap(was_overlap); ops.set_pair(True, force=False); ops.set_amp(False)
    (l0, log0, g0), (l1, log1, g1), (l2, log2, g2) = res[0], res[1], res[2]
    assert l0 == l1 == l2, (l0, l1, l2)          # the forward is deterministic: same kernels, same arguments -> the same bits
    log1.pop("bert_layer_fwd:entry")
    assert log0 == log1 == log2, (log0, log1)    # ... and the same kernel families / tiles, launch for launch
    for a, b, c in zip(g0, g1, g2):
        assert float(a.abs().max()) > 0
        # backward: float atomics, order differs run to run; the third run is the per-launch path again: the yardstick.  Inside an
        # autocast region two runs of the SAME path already differ by the fp16 rounding error itself: a difference d in a gradient flips
        # the rounding of a fraction d / 2^-11 of the elements of the next product's operand, which moves that product's result by
        # sqrt(d 2^-11) -- 5e-8 of atomics noise is 5e-3 six nodes later (tools/bwd_diff.py, profiles/r06_amp_reproducibility.txt)
        tol = 2e-2 if form == "amp" else 1e-5
        noise = float((a - c).norm() / a.norm())
        assert noise < tol, noise
        assert float((a - b).norm() / a.norm()) < max(tol, 3 * noise)


@pytest.mark.parametrize("pair", [False, True])
def test_inference_is_bit_identical_and_runs_one_qkv_product(tmp_path, pair):
    """no flat buffers in evaluation mode: the stacked planes of the three projections come from the cache on the weights
    (vbg.ops.stacked_qkv), refreshed when a weight changes"""
    from vbg import ops
    dev = torch.device("cuda")
    net = _net(tmp_path, 0.0).to(dev).eval()
    imgs, segs, classes, coors, corpus, mask = _batch(dev)
    was = ops._LAYER_ENTRY[0]
    ops.set_pair(True, force=pair)
    if not pair:
        ops.set_pair(False)
    out, logs = {}, {}
    try:
        with torch.no_grad():
            for entry in (False, True):
                ops.set_layer_entry(entry)
                log = ops.dispatch_log(True)
                out[entry] = net.inference(imgs, segs, coors, corpus, mask).clone()
                ops.dispatch_log(False)
                assert log.pop("bert_layer_fwd:entry", 0) == (LAYERS if entry else 0), log
                logs[entry] = dict(log)
            assert logs[False] == logs[True], logs            # the same kernel families and tiles, launch for launch
            assert torch.equal(out[False], out[True])
            for layer in net.BERTgrid_generator.model.encoder.layer:          # one Q/K/V product per layer, from the stacked planes
                cache = layer.attention.self.query.weight.__dict__.get("_vbg_wplanes", {})
                assert any(k[0] == "qkv" for k in cache), list(cache)
            # a weight updated in place is seen by the cache
            q = net.BERTgrid_generator.model.encoder.layer[0].attention.self.query.weight
            q.mul_(1.5)
            moved = net.inference(imgs, segs, coors, corpus, mask)
            assert not torch.equal(moved, out[True])
            q.div_(1.5)
            back = net.inference(imgs, segs, coors, corpus, mask)
            assert torch.allclose(back, out[True], rtol=1e-5, atol=1e-6)
    finally:
        ops.set_layer_entry(was); ops.set_pair(True, force=False)


def test_inference_inside_autocast_takes_the_one_product_forms_on_the_small_tile(tmp_path):
    """`amp: True` validation / inference of a document or two: the encoder's products run form 2 on the 64 x 64 tile (round 6), through
    the layer entry; probabilities stay within the fp16 operand rounding of the fp32-grade call"""
    from vbg import ops
    dev = torch.device("cuda")
    net = _net(tmp_path, 0.0).to(dev).eval()
    imgs, segs, classes, coors, corpus, mask = _batch(dev)
    with torch.no_grad():
        ref = net.inference(imgs, segs, coors, corpus, mask).clone()
        log = ops.dispatch_log(True)
        with torch.autocast("cuda", dtype=torch.float16):
            got = net.inference(imgs, segs, coors, corpus, mask).clone()
        ops.dispatch_log(False)
    ops.set_amp(False)
    assert log.get("bert_layer_fwd:entry", 0) == LAYERS and log.get("plane_gemm:onep", 0) >= 3 * LAYERS and log.get("attn:onep", 0) == LAYERS, log
    assert log.get("plane_gemm:tile64004", 0) >= 3 * LAYERS, log
    assert bool(torch.isfinite(got).all()) and torch.allclose(got.sum(1), torch.ones(got.shape[0], device=dev), atol=1e-5)
    assert float((got - ref).abs().max()) < 2e-2 and float((got - ref).abs().max()) > 0.0


def test_layer_entry_rejects_a_descriptor_without_its_operands():
    import ctypes as C
    from vbg.lib import BertLayerFwdDesc, lib
    d = BertLayerFwdDesc()
    d.ntok, d.hidden, d.inter, d.heads = 128, 768, 3072, 12
    assert lib.vbg_bert_layer_fwd(C.byref(d), None) == -1          # argument error, nothing launched
    assert lib.vbg_bert_layer_fwd(None, None) == -1


# ---- every route of BertLayerFn against HF BertModel (fp32, CPU) ----------------------------------------------------------------------
# dense: intermediate size not a multiple of 32; planes_unfused: head width 128 (the LayerNorm kernels take hidden sizes that are multiples
# of 256, so the hidden size cannot select the dense route); the three fused-attention routes run the homed full-net fixture
# (route 3 with the pair form off, or with the pair forward and the bf16 backward: mixed; route 4 all-pair)
ROUTES = ["dense", "planes_unfused", "planes_fused", "planes_fused_mixed", "pair"]
NT = 40                 # tokens per document (one window); two documents


def _route_tags_ok(route, grad, log):
    fam = {k for k in log if k.startswith(("gemm:", "plane_gemm:", "attn:"))}
    if route == "dense":
        return bool(fam) and all(k.startswith("gemm:") for k in fam)
    if route == "planes_unfused":
        return any(k.startswith("plane_gemm:") for k in fam) and not any(k.startswith("attn:") for k in fam)
    pair_fwd = route != "planes_fused"
    attn = "attn:pair" if (route == "pair" or (pair_fwd and not grad)) else "attn:bf16x3"
    want = {attn, "plane_gemm:pair" if pair_fwd else "plane_gemm:bf16x3"}
    if grad:
        want.add("plane_gemm:grouped_pair" if route == "pair" else "plane_gemm:grouped_bf16x3")
    grouped = {k for k in fam if k.startswith("plane_gemm:grouped_")}
    return want <= fam and grouped <= want and {k for k in fam if k.startswith("attn:")} == {attn}


def _route_model(tmp_path, route, grad, dev):
    """(HF BertModel on the device inside a BERTgridGenerator, optimizer or None)"""
    from transformers import BertConfig, BertModel
    from model.BERTgrid_generator import BERTgridGenerator
    from vbg.optim import FusedAdamW, split_parameters
    if route in ("dense", "planes_unfused"):
        hidden, inter = 256, (1000 if route == "dense" else 1024)
        torch.manual_seed(0)
        hf = BertModel(BertConfig(vocab_size=1200, hidden_size=hidden, num_attention_heads=2, intermediate_size=inter, num_hidden_layers=LAYERS,
                                  hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0))
        return BERTgridGenerator(bert_model=hf, grid_mode="mean", stride=8).to(dev), None
    net = _net(tmp_path, 0.0).to(dev)
    opt = FusedAdamW(split_parameters(net)[1], dev, lr=0.0) if grad else None          # homed: every layer gradient sunk, Q/K/V stacked
    return net.BERTgrid_generator, opt


@pytest.mark.parametrize("grad", [True, False])
@pytest.mark.parametrize("route", ROUTES)
def test_every_layer_route_vs_hf_bert(tmp_path, route, grad):
    from transformers import BertModel
    from vbg import ops
    dev = torch.device("cuda")
    gen, opt = _route_model(tmp_path, route, grad, dev)
    gen.train(grad)
    g = torch.Generator().manual_seed(3)
    corpus = torch.randint(1000, 1200, (2, NT), generator=g)
    mask = torch.ones_like(corpus)
    segs = tuple(torch.arange(NT, dtype=torch.int32) for _ in range(2))          # one segment per token: the mean is the token state
    R = torch.randn(2 * NT, gen.model.config.hidden_size, generator=g)
    was_bwd = ops._PAIR_BWD[0]
    ops.set_pair(route != "planes_fused", force=route in ("planes_fused_mixed", "pair"))
    ops._PAIR_BWD[0] = route != "planes_fused_mixed"
    try:
        if opt is not None:
            opt.zero_grad()
        log = ops.dispatch_log(True)
        with torch.set_grad_enabled(grad):
            got = torch.cat(gen.BERT_embedding(corpus.to(dev), mask.to(dev), tuple(s.to(dev) for s in segs)), 0)
            if grad:
                (got * R.to(dev)).sum().backward()
        torch.cuda.synchronize()
        ops.dispatch_log(False)
    finally:
        ops.dispatch_log(False); ops.set_pair(True, force=False); ops._PAIR_BWD[0] = was_bwd
    assert _route_tags_ok(route, grad, log), (route, grad, log)

    ref = BertModel(gen.model.config)
    ref.load_state_dict({k: v.detach().cpu() for k, v in gen.model.state_dict().items()}, strict=False)
    ref.train(False)
    ids = torch.cat([torch.full((2, 1), 101), corpus, torch.full((2, 1), 102)], 1)
    with torch.set_grad_enabled(grad):
        want = ref(input_ids=ids, attention_mask=torch.ones_like(ids), token_type_ids=torch.zeros_like(ids)).last_hidden_state[:, 1:-1]
        want = want.reshape(2 * NT, -1)
        if grad:
            (want * R).sum().backward()
    err = float((got.detach().cpu() - want.detach()).abs().max())
    print(f"{route} grad={grad}: output max abs err {err:.3e}")
    assert torch.allclose(got.detach().cpu(), want.detach(), rtol=2e-4, atol=2e-5), err
    if not grad:
        return
    worst, bad = 0.0, []
    mine = dict(gen.model.named_parameters())
    for name, p in ref.named_parameters():
        if p.grad is None or name.endswith("key.bias"):          # (key.bias: an analytically zero gradient, rounding noise on both sides)
            continue
        a, b = mine[name].grad.detach().cpu().double(), p.grad.double()
        rel = float((a - b).norm() / (b.norm() + 1e-30))
        worst = max(worst, rel)
        if rel > 1e-3:
            bad.append((name, rel))
    print(f"{route}: worst parameter gradient rel L2 err {worst:.3e}")
    assert not bad, bad
