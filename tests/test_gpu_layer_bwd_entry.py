"""The one-call encoder layer backward (include/vbg.h vbg_bert_layer_bwd, csrc/encoder.hip) launches the same kernels with the same
descriptors, in the same order, as the per-launch path (vbg/ops.py bert_layer_bwd_launches): in deterministic mode a training step must be
BIT-identical through either, in the default mode identical to the float atomics' own noise; the entry must be the path taken, must
tell the gradient sink about the same parameters in the same order, and must step aside where it does not apply.  Needs a real MI355X.

The fixture is the two-layer bert-base-width net of tests/test_gpu_layer_entry.py on golden/e2e.npz: 84 packed tokens, a multiple of
neither 32 nor any tile (where a descriptor's row stride or padding can be wrong); the pair form is forced (the fixture is smaller than
the tiles it waits for), which makes every layer run the all-pair backward on the bound route."""
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_layer_entry import LAYERS, NT, _batch, _net, _route_model

TAG = "bert_layer_bwd:entry"
_CACHE = {}


@pytest.fixture(scope="module")
def fixture(tmp_path_factory):
    """(net, optimizers, batch) per dropout rate, built once: the optimizers never step (the tests compare gradients), so every test sees
    the same weights"""
    def get(dropout):
        if dropout not in _CACHE:
            from vbg.optim import FusedAdamW, FusedSGD, split_parameters
            dev = torch.device("cuda")
            net = _net(tmp_path_factory.mktemp(f"net{int(dropout * 10)}"), dropout).to(dev).train()
            cnn, bert = split_parameters(net)
            _CACHE[dropout] = (net, [FusedSGD(cnn, dev, lr=0.0), FusedAdamW(bert, dev, lr=0.0)], _batch(dev))
        return _CACHE[dropout]
    yield get
    _CACHE.clear()


class _switches:
    """the process-wide switches the tests move, put back on exit"""

    def __enter__(self):
        from vbg import ops
        self.saved = (ops._LAYER_ENTRY[0], ops._LAYER_BWD_ENTRY[0], ops.overlap_enabled(), ops._DET_USER[0], ops._DET[0], ops._AMAX_POOL_SLOTS[0])
        ops.set_overlap(False)                       # one stream: the comparison is about the launches, not their interleaving
        ops.set_pair(True, force=True)
        return ops

    def __exit__(self, *exc):
        from vbg import functions, ops
        ops.dispatch_log(False)
        ops.set_gemm_profiler(None)
        functions.GRAD_READY[0] = None
        ops.set_layer_entry(self.saved[0]); ops.set_layer_bwd_entry(self.saved[1]); ops.set_overlap(self.saved[2])
        ops._DET_USER[0], ops._DET[0], ops._AMAX_POOL_SLOTS[0] = self.saved[3:]
        ops.set_pair(True, force=False); ops.set_amp(False)


def _step(fx, form, entry_bwd):
    """one training step of the fixture with the backward entry on or off -> (loss, dispatch log of forward AND backward, flat gradients)"""
    from vbg import ops
    net, opts, dbatch = fx
    ops.set_layer_bwd_entry(entry_bwd)
    for o in opts:
        o.zero_grad()
    net.BERTgrid_generator._step_seed = 41
    random.seed(7)
    log = ops.dispatch_log(True)
    with torch.autocast("cuda", dtype=torch.float16, enabled=form == "amp"):
        loss = net(*dbatch)
    loss.backward()
    torch.cuda.synchronize()
    ops.dispatch_log(False)
    return loss.detach().clone(), dict(log), [o.group.gflat.clone() for o in opts]


def _assert_bitwise(off, on):
    (l0, log0, g0), (l1, log1, g1) = off, on
    assert TAG not in log0, log0
    assert log1.pop(TAG, 0) == LAYERS, log1
    assert log0 == log1, (log0, log1)               # the same kernel families, tiles and reduction forms, launch for launch
    assert torch.equal(l0, l1), (float(l0), float(l1))
    for a, b in zip(g0, g1):
        assert float(a.abs().max()) > 0 and bool(torch.isfinite(a).all())
        assert torch.equal(a, b), float((a - b).norm() / a.norm())


@pytest.mark.parametrize("form", ["pair", "amp"])
@pytest.mark.parametrize("dropout", [0.0, 0.1])
def test_deterministic_step_is_bit_identical_through_the_bwd_entry(fixture, form, dropout):
    with _switches() as ops:
        ops.set_deterministic(True)
        off = _step(fixture(dropout), form, False)
        on = _step(fixture(dropout), form, True)
    want = "plane_gemm:grouped_onep" if form == "amp" else "plane_gemm:grouped_pair"
    assert off[1].get(want, 0) == LAYERS, off[1]                    # every layer ran the all-pair backward
    assert off[1].get("det:plane_colsum", 0) == LAYERS and off[1].get("det:split_colsum", 0) >= LAYERS, off[1]
    assert not [k for k in off[1] if k.startswith("fatomic:plane_") or k.startswith("fatomic:split_")], off[1]
    _assert_bitwise(off, on)


@pytest.mark.parametrize("form", ["pair", "amp"])
def test_default_mode_step_matches_to_the_atomics_noise(fixture, form):
    """the yardstick of tests/test_gpu_layer_entry.py::test_training_step_is_bit_identical_through_the_layer_entry: off, on, off"""
    with _switches():
        res = [_step(fixture(0.1), form, entry) for entry in (False, True, False)]
    (l0, log0, g0), (l1, log1, g1), (l2, log2, g2) = res
    assert torch.equal(l0, l1) and torch.equal(l0, l2), (float(l0), float(l1), float(l2))
    assert TAG not in log0 and TAG not in log2 and log1.pop(TAG, 0) == LAYERS, (log0, log1)
    assert log0 == log1 == log2, (log0, log1)
    assert log0.get("fatomic:plane_colsum", 0) >= LAYERS and log0.get("fatomic:split_colsum", 0) >= LAYERS, log0
    for a, b, c in zip(g0, g1, g2):
        assert float(a.abs().max()) > 0
        tol = 2e-2 if form == "amp" else 1e-5           # (that test's tolerances: inside autocast two runs of one path differ by fp16 rounding)
        noise = float((a - c).norm() / a.norm())
        diff = float((a - b).norm() / a.norm())
        print(f"{form}: off-vs-off noise {noise:.3e}, off-vs-on {diff:.3e}")
        assert noise < tol, noise
        assert diff < max(tol, 3 * noise), (diff, noise)


def test_pair_route_vs_hf_bert_through_the_bwd_entry(tmp_path):
    """the `pair` case of tests/test_gpu_layer_entry.py::test_every_layer_route_vs_hf_bert with the backward entry on: same bounds"""
    from transformers import BertModel
    dev = torch.device("cuda")
    with _switches() as ops:
        ops.set_layer_bwd_entry(True)
        gen, opt = _route_model(tmp_path, "pair", True, dev)
        gen.train(True)
        g = torch.Generator().manual_seed(3)
        corpus = torch.randint(1000, 1200, (2, NT), generator=g)
        mask = torch.ones_like(corpus)
        segs = tuple(torch.arange(NT, dtype=torch.int32) for _ in range(2))          # one segment per token: the mean is the token state
        R = torch.randn(2 * NT, gen.model.config.hidden_size, generator=g)
        opt.zero_grad()
        log = ops.dispatch_log(True)
        got = torch.cat(gen.BERT_embedding(corpus.to(dev), mask.to(dev), tuple(s.to(dev) for s in segs)), 0)
        (got * R.to(dev)).sum().backward()
        torch.cuda.synchronize()
        ops.dispatch_log(False)
    assert log.get(TAG, 0) == LAYERS and log.get("plane_gemm:grouped_pair", 0) == LAYERS and log.get("attn:pair", 0) == 3 * LAYERS, log

    ref = BertModel(gen.model.config)
    ref.load_state_dict({k: v.detach().cpu() for k, v in gen.model.state_dict().items()}, strict=False)
    ref.train(False)
    ids = torch.cat([torch.full((2, 1), 101), corpus, torch.full((2, 1), 102)], 1)
    want = ref(input_ids=ids, attention_mask=torch.ones_like(ids), token_type_ids=torch.zeros_like(ids)).last_hidden_state[:, 1:-1]
    want = want.reshape(2 * NT, -1)
    (want * R).sum().backward()
    err = float((got.detach().cpu() - want.detach()).abs().max())
    print(f"output max abs err {err:.3e}")
    assert torch.allclose(got.detach().cpu(), want.detach(), rtol=2e-4, atol=2e-5), err
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
    print(f"worst parameter gradient rel L2 err {worst:.3e}")
    assert not bad, bad


def test_slot_pools_turn_over_inside_one_backward(fixture):
    """four slots per pool: the nine slots of one call come from three pools, and pools are replaced between the layers"""
    with _switches() as ops:
        ops.set_deterministic(True)
        ops._AMAX_POOL_SLOTS[0] = 4
        ops._AMAX_POOL.clear()
        try:
            off = _step(fixture(0.1), "pair", False)
            on = _step(fixture(0.1), "pair", True)
        finally:
            ops._AMAX_POOL.clear()                  # (the next caller starts a pool of the usual size)
    _assert_bitwise(off, on)


def test_the_gradient_sink_is_told_the_same_parameters_in_the_same_order(fixture):
    from vbg import functions
    told = {}
    with _switches():
        for entry in (False, True):
            seq = told[entry] = []
            functions.GRAD_READY[0] = lambda p, seq=seq: seq.append(id(p))
            _, log, _ = _step(fixture(0.1), "pair", entry)
            functions.GRAD_READY[0] = None
            assert log.get(TAG, 0) == (LAYERS if entry else 0), log
    net = fixture(0.1)[0]
    layer_params = {id(p) for layer in net.BERTgrid_generator.model.encoder.layer for p in layer.parameters()}
    assert len(layer_params) == 16 * LAYERS and layer_params <= set(told[True])          # every parameter of every layer was reported
    assert told[False] == told[True]


@pytest.mark.parametrize("case", ["bf16_route", "switch_off", "gemm_profiler"])
def test_the_entry_steps_aside(fixture, case):
    from vbg.lib import OP_DENSE_K
    with _switches() as ops:
        prof = None
        if case == "bf16_route":
            ops.set_pair(False)
        elif case == "gemm_profiler":
            prof = ops.GemmProfiler(OP_DENSE_K, OP_DENSE_K)
            ops.set_gemm_profiler(prof)
        loss, log, grads = _step(fixture(0.1), "pair", case != "switch_off")
        ops.set_gemm_profiler(None)
        if prof is not None:
            assert prof.summary()[0] > 0                # the hook timed single launches
    assert TAG not in log, log
    assert case != "gemm_profiler" or "bert_layer_fwd:entry" not in log, log
    assert log.get("plane_gemm:grouped_bf16x3" if case == "bf16_route" else "plane_gemm:grouped_pair", 0) == LAYERS, log
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in grads)


def test_the_two_halves_are_independent(fixture):
    with _switches() as ops:
        ops.set_layer_entry(False)
        loss, log, grads = _step(fixture(0.1), "pair", True)
    assert log.get(TAG, 0) == LAYERS and "bert_layer_fwd:entry" not in log, log
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(g).all()) for g in grads)
