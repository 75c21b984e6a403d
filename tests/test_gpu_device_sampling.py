"""Device sampling (vbg.ops.set_device_sampling / VBG_DEVICE_SAMPLING=1): the sampled and OHEM cross-entropy losses with their draws,
selections and denominators on the device -- loss modules against torch fp64 over exactly the lists the plans report, and the whole
simp-mode training step without a host read.  Needs a real MI355X."""
import random
import types

import pytest
import torch
import torch.nn.functional as F

import sample_restate as S
from test_gpu_model import build_product, build_product_mode, load_synth, to_dev
from test_oracle_golden import _e2e_inputs, e2e_cfg, modes_state

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from vbg import ops as _ops
    return _ops


@pytest.fixture()
def sampling_on(ops):
    was = ops.device_sampling_enabled()
    ops.set_device_sampling(True)
    yield
    ops.set_device_sampling(was)


def dev():
    return torch.device("cuda")


def close(a, b, rtol, atol):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    d = (a - b).abs()
    ok = a.shape == b.shape and bool((d <= atol + rtol * b.abs()).all())
    if not ok:
        print("max abs", float(d.max()), "ref", float(b.flatten()[d.argmax()]))
    return ok


def reported(lists):
    """[(elements, keep)] device tensors -> [python list of the first keep elements]"""
    return [e[:int(k)].cpu().tolist() for e, k in lists]


def fp64_ce(logits, labels, lists, weight=None):
    """sum of torch's fp64 cross entropy over the listed elements -> (sum, leaf)"""
    x = logits.detach().cpu().double().requires_grad_(True)
    pick = torch.tensor([i for l in lists for i in l], dtype=torch.long)
    lab = labels.cpu().long()
    s = F.cross_entropy(x[pick], lab[pick], weight=None if weight is None else weight.cpu().double(), reduction="sum")
    return s, x


# ---- the loss modules ------------------------------------------------------------------------------------------------------------------
def test_switch_and_seed_rule(ops):
    assert ops.device_sampling_enabled() is False                          # the default
    torch.manual_seed(0x1_2345_6789)
    ops.reset_sample_counter()
    assert ops.next_sample_seed() == S.step_seed(0, 0x1_2345_6789) == 0x23456789
    assert ops.next_sample_seed() == S.step_seed(1, 0x1_2345_6789)
    ops.reset_sample_counter(7)
    assert ops.next_sample_seed() == S.step_seed(7, 0x1_2345_6789)


def test_random_sample_loss_on_the_device(ops, sampling_on):
    """sample_list [4, 8, 4] over three classes: class 0 empty, class 1 with 5 elements (below k = 8), class 2 with the rest"""
    from pipeline.custom_loss import CrossEntropyLossRandomSample
    d = dev()
    n = 3001
    g = torch.Generator().manual_seed(1)
    labels = torch.full((n,), 2, dtype=torch.int32)
    ones = torch.randperm(n, generator=g)[:5]
    labels[ones] = 1
    logits = (torch.randn(n, 3, generator=g) * 2).to(d).requires_grad_(True)
    w = torch.tensor([0.5, 2.0, 1.5])
    mod = CrossEntropyLossRandomSample([4, 8, 4], weight=w).to(d)
    torch.manual_seed(11)
    ops.reset_sample_counter()
    plan = mod.plan(labels.to(d), 3)
    assert plan.device and plan.count_tensors() == []
    lists = reported(plan.lists())
    want_lists, want_keep, want_n = S.sample_select(labels.numpy(), [(0, 1, 4), (1, 1, 8), (2, 1, 4)], S.step_seed(0, 11))
    assert [sorted(l) for l in lists] == [sorted(l.tolist()) for l in want_lists]          # the restatement's draw
    assert [len(l) for l in lists] == [0, 5, 4] and plan.n.cpu().tolist() == [0, 5, n - 5] == want_n
    loss = mod(logits, labels.to(d), plan)
    assert loss.dtype == torch.float64 and loss.shape == (1,)
    loss.backward()
    s, x = fp64_ce(logits, labels, lists, w)
    ref = s / 9
    ref.backward()
    assert close(loss, ref.reshape(1), 1e-5, 1e-6) and close(logits.grad, x.grad, 1e-4, 1e-6)


def test_random_sample_nothing_kept_is_nan(ops, sampling_on):
    from pipeline.custom_loss import CrossEntropyLossRandomSample
    d = dev()
    labels = torch.full((100,), 7, dtype=torch.int32, device=d)          # in no category
    mod = CrossEntropyLossRandomSample([4, 8, 4]).to(d)
    loss = mod(torch.randn(100, 3, device=d), labels)
    assert loss.shape == (1,) and bool(torch.isnan(loss).all())          # 0 / 0, as on the host route


@pytest.mark.parametrize("rand", [True, False])
@pytest.mark.parametrize("negatives", [3, 0, 500])
def test_ohem_loss_on_the_device(ops, sampling_on, negatives, rand):
    """num_hard 4 / 4: positives (label != 0) far above it; negatives below k, absent, or above 2k.  rand: the random pre-sample of 8
    per category; without it the candidates are the whole categories in compaction order."""
    from pipeline.custom_loss import CrossEntropyLossOHEM
    d = dev()
    n, ncls = 2000, 5
    g = torch.Generator().manual_seed(2 + negatives)
    labels = torch.randint(1, ncls, (n,), generator=g).int()
    labels[torch.randperm(n, generator=g)[:negatives]] = 0
    logits = (torch.randn(n, ncls, generator=g) * 2).to(d).requires_grad_(True)
    w = torch.tensor([0.5, 0.0, 2.0, 1.5, 1.0])
    mod = CrossEntropyLossOHEM(4, 4, weight=w, random=rand).to(d)
    torch.manual_seed(12)
    ops.reset_sample_counter(3)
    plan = mod.plan(labels.to(d))
    assert plan.device and plan.bounded == rand and plan.count_tensors() == []
    pre = reported(plan.lists())
    if rand:
        want_lists, _, _ = S.sample_select(labels.numpy(), [(0, 0, 8), (0, 1, 8)], S.step_seed(3, 12))
    else:
        want_lists = [S.members(labels.numpy(), 0, 0), S.members(labels.numpy(), 0, 1)]
    assert pre == [l.tolist() for l in want_lists]                          # order included: the quirk indexes positions
    loss = mod(logits, labels.to(d), plan)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    loss.backward()
    chosen = reported(plan.chosen)
    assert [len(c) for c in chosen] == [4, min(4, negatives)]
    # the choice itself, from fp64 losses of the pre-sampled lists (no ties in random logits): the reference's double indexing
    xl = logits.detach().cpu().double()
    for lst, got in zip(pre, chosen):
        if len(lst) <= 4:
            assert got == lst
            continue
        idx = torch.tensor(lst)
        v = F.cross_entropy(xl[idx], labels[idx].long(), weight=w.double(), reduction="none")
        assert got == [lst[i] for i in S.ohem_choice(v.float().numpy(), 4)]
    s, x = fp64_ce(logits, labels, chosen, w)
    ref = s / (4 + min(4, negatives))
    ref.backward()
    assert close(loss, ref, 1e-5, 1e-6) and close(logits.grad, x.grad, 1e-4, 1e-6)


def test_ohem_nothing_kept_is_zero_times_the_logits(ops, sampling_on):
    from pipeline.custom_loss import CrossEntropyLossOHEM
    d = dev()
    labels = torch.full((64,), 2, dtype=torch.int32, device=d)          # keyed labels: neither positive (1) nor negative (0)
    logits = torch.randn(64, 2, device=d).requires_grad_(True)
    mod = CrossEntropyLossOHEM(4, 4, random=True).to(d)
    plan = mod.plan(labels, keyed=True)
    assert plan.device
    loss = mod(logits, labels, plan)
    loss.backward()
    assert float(loss) == 0.0 and float(logits.grad.abs().max()) == 0.0


def test_switch_off_builds_host_plans(ops):
    from pipeline.custom_loss import BCELossOHEM, CrossEntropyLossOHEM, CrossEntropyLossRandomSample
    d = dev()
    labels = torch.randint(0, 3, (500,), dtype=torch.int32, device=d)
    assert not ops.device_sampling_enabled()
    p1 = CrossEntropyLossRandomSample([4, 8, 4]).plan(labels, 3)
    p2 = CrossEntropyLossOHEM(4, 4, random=True).plan(labels)
    assert not p1.device and not p2.device and len(p1.count_tensors()) == 3 and len(p2.count_tensors()) == 2
    ops.set_device_sampling(True)
    try:
        assert CrossEntropyLossOHEM(4, 4, random=True).plan(labels).device
        p3 = CrossEntropyLossOHEM(4, 4, random=False).plan(labels)                         # no pre-sample: sorted at the capacity
        assert p3.device and not p3.bounded and p3.count_tensors() == []
        assert not CrossEntropyLossOHEM(4096, 4, random=True).plan(labels).device         # 2k > 4096
        assert not CrossEntropyLossRandomSample(None).plan(labels, 3).device              # plain path
        assert not BCELossOHEM(4, 4, random=True).ce.plan(labels, keyed=True).device      # the binary losses keep the host route
    finally:
        ops.set_device_sampling(False)


# ---- the model -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def simp_net(golden, tmp_path_factory):
    cfg = e2e_cfg("resnet_18_fpn")
    net = build_product(tmp_path_factory.mktemp("dsamp"), "resnet_18_fpn", cfg)
    load_synth(net, cfg, 1200)
    net = net.to(dev()).train()
    return net, to_dev(_e2e_inputs(golden("e2e.npz")), dev())


class _Recorder:
    """records every plan the loss modules build (pipeline.custom_loss looks its plan classes up by name)"""

    def __init__(self, monkeypatch):
        import pipeline.custom_loss as CL
        self.plans = plans = []

        class RS(CL.RandomSamplePlan):
            def __init__(self, *a, **k):
                super().__init__(*a, **k)
                plans.append(self)

        class OH(CL.OhemPlan):
            def __init__(self, *a, **k):
                super().__init__(*a, **k)
                plans.append(self)

        monkeypatch.setattr(CL, "RandomSamplePlan", RS)
        monkeypatch.setattr(CL, "OhemPlan", OH)

    def take(self):
        out = []
        for p in self.plans:
            assert p.device
            out.append(reported(p.lists()) + (reported(p.chosen) if hasattr(p, "chosen") else []))
        del self.plans[:]
        return out


def _step(ops, net, batch, seed):
    net.zero_grad(set_to_none=True)
    torch.manual_seed(seed)
    ops.reset_sample_counter()
    loss = net(*batch)
    loss.backward()
    torch.cuda.synchronize()
    grads = {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in net.named_parameters()}
    return loss.detach().clone(), grads


def _forbid_host_route(monkeypatch):
    import pipeline.custom_loss as CL

    def boom(*a, **k):
        raise AssertionError("the host route was reached")

    monkeypatch.setattr(CL.PendingCounts, "__init__", boom)
    monkeypatch.setattr(random, "sample", boom)
    # the losses' upload of drawn positions is `ops.h2d` as pipeline.custom_loss sees it (the encoder's own index tables go through
    # the same function from model/BERTgrid_generator.py and stay allowed)
    real = CL.ops
    proxy = types.SimpleNamespace(**{k: getattr(real, k) for k in dir(real) if not k.startswith("__")})
    proxy.h2d = boom
    monkeypatch.setattr(CL, "ops", proxy)


def test_training_step_without_a_host_read(ops, sampling_on, simp_net, monkeypatch):
    net, batch = simp_net
    rec = _Recorder(monkeypatch)
    random.seed(7)
    ops.set_device_sampling(False)
    _, host_grads = _step(ops, net, batch, 5)                                # the host route: which parameters get a gradient
    del rec.plans[:]
    ops.set_device_sampling(True)
    _forbid_host_route(monkeypatch)
    loss, grads = _step(ops, net, batch, 5)
    lists = rec.take()
    assert len(lists) == 4 and bool(torch.isfinite(loss).all())
    for n, g in grads.items():
        assert (g is None) == (host_grads[n] is None), n
        assert g is None or bool(torch.isfinite(g).all()), n
    assert any(g is not None and float(g.abs().max()) > 0 for g in grads.values())
    # the same seed and counter: the same lists; another seed: other lists
    loss2, _ = _step(ops, net, batch, 5)
    assert rec.take() == lists
    assert abs(float(loss2) - float(loss)) <= 1e-5 * abs(float(loss))
    _step(ops, net, batch, 6)
    assert rec.take() != lists


def test_deterministic_mode_repeats_bitwise(ops, sampling_on, simp_net, monkeypatch):
    net, batch = simp_net
    rec = _Recorder(monkeypatch)
    with ops.deterministic_scope(True):
        la, ga = _step(ops, net, batch, 9)
        a = rec.take()
        lb, gb = _step(ops, net, batch, 9)
        b = rec.take()
    assert a == b and torch.equal(la, lb)
    for n in ga:
        assert (ga[n] is None) == (gb[n] is None) and (ga[n] is None or torch.equal(ga[n], gb[n])), n


def test_heads_stream_with_small_pools_equals_one_stream(ops, sampling_on, simp_net, monkeypatch):
    """the device plans are built on the heads' stream and read on the caller's: with 16-slot amax pools (tests/test_gpu_streams.py)
    blocks turn over quickly, so a tensor missing from reserve_for shows as other lists or another loss"""
    net, batch = simp_net
    rec = _Recorder(monkeypatch)
    was = (ops._OVERLAP[0], ops._AMAX_POOL_SLOTS[0])
    try:
        ops._AMAX_POOL_SLOTS[0] = 16
        ops._AMAX_POOL.clear()
        ops.set_overlap(False)
        l0, _ = _step(ops, net, batch, 21)
        one = rec.take()
        ops.set_overlap(True)
        for _ in range(3):
            l1, _ = _step(ops, net, batch, 21)
            assert rec.take() == one
            assert float(l1) == float(l0)
    finally:
        ops.set_overlap(was[0])
        ops._AMAX_POOL_SLOTS[0] = was[1]
        ops._AMAX_POOL.clear()


def test_full_mode_keeps_the_host_route(ops, golden, tmp_path, monkeypatch):
    """classifier_mode "full": its losses read prediction-dependent sizes on the host anyway; the switch changes nothing"""
    g = golden("e2e_modes.npz")
    cfg, sd = modes_state(g, "full")
    net = build_product_mode(tmp_path, "full", cfg)
    net.load_state_dict(sd, strict=False)
    net = net.to(dev()).train()
    batch = to_dev(_e2e_inputs(golden("e2e.npz")), dev())
    calls = []
    real = random.sample
    monkeypatch.setattr(random, "sample", lambda pop, k: (calls.append((len(pop), k)), real(pop, k))[1])
    out = []
    for on in (False, True):
        ops.set_device_sampling(on)
        try:
            del calls[:]
            random.seed(7)
            with ops.deterministic_scope(True):
                loss = net(*batch)
                loss.backward()
            torch.cuda.synchronize()
            out.append((float(loss), list(calls)))
        finally:
            ops.set_device_sampling(False)
    assert out[0][1] and out[0][1] == out[1][1]                              # the same host draws, from the same populations
    assert out[0][0] == out[1][0]
