"""vbg.optim.clip_in_step(norm_type=..., when=(loss, threshold)), the host side (no GPU, no launch): the fp32 arithmetic of the finish
(vbg_clip_coef_gate) restated for the three norm kinds with the gate and held against `coef_ref` of tests/test_clip_step_host.py and
against torch.nn.utils.clip_grad_norm_(norm_type=...); the gate's decision as the kernels take it against torch's own `loss > threshold`
on the CPU; the calls clip_in_step issues, with the ops wrappers replaced by recorders -- today's names without the new arguments, one
vbg_grad_norm_seg per optimizer and one vbg_clip_coef_gate with them; what is refused; and the argument checks of the two new entries,
which return before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_clip_step_host import STEP_WRAPPERS, _bits, _flat_pair, _stock, coef_ref, names

f32 = np.float32
INF = float("inf")
KINDS = {2.0: 2, 1.0: 1, INF: 0}


def finish_ref(partials, kind, max_norm, norm_scale=1.0, grad_scale=None, gate=None):
    """vbg_clip_coef_gate restated, one fp32 operation per line -> (total, coefficient, gate).  partials: fp32 values; gate: None (no
    gate), True (open) or False (closed: no partial is read)"""
    if gate is False:
        return f32(0.0), f32(1.0), f32(0.0)
    p = np.asarray(partials, dtype=np.float32)
    with np.errstate(all="ignore"):
        if kind == 2:
            root = f32(np.sqrt(p.astype(np.float64).sum()))
        elif kind == 1:
            root = f32(p.astype(np.float64).sum())
        else:
            root = f32(np.nan) if np.isnan(p).any() else f32(max([0.0] + [float(x) for x in p]))
        t = f32(root * f32(norm_scale))
        if grad_scale is not None:
            t = f32(t * f32(1.0 / float(f32(grad_scale))))
        d = f32(t + f32(1e-6))
        r = f32(f32(1.0) / d)
        c = f32(r * f32(max_norm))
    return t, (f32(1.0) if c > f32(1.0) else c), f32(1.0)


def gate_ref(loss, threshold):
    """the kernels' decision for a one-element fp64 / fp32 tensor: `*loss > threshold` in double, or `*loss > (float)threshold` in
    fp32 -- the host hands the threshold over as a double (vbg.ops: float(threshold)) and the library rounds it to fp32 with a C cast"""
    thr = float(threshold)
    with np.errstate(all="ignore"):
        if loss.dtype == torch.float64:
            return bool(np.float64(loss.item()) > np.float64(thr))
        return bool(loss.numpy().reshape(()).astype(np.float32) > np.float64(thr).astype(np.float32))


# ------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------
def test_kind_2_without_a_gate_is_coef_ref():
    part = torch.randint(0, 1000, (700,), generator=torch.Generator().manual_seed(7)).float().numpy()
    root = f32(np.sqrt(float(part.astype(np.float64).sum())))
    for max_norm, norm_scale, scale in ((2.0, 1.0, None), (1e4, 1.0, None), (2.0, 0.5, None), (0.37, 1.0, 1024.0), (0.37, 1.0, 1000.0), (0.13, 0.5, 1000.0)):
        t, c, gate = finish_ref(part, 2, max_norm, norm_scale, scale)
        t0, c0 = coef_ref(root, max_norm, norm_scale, scale)
        assert (_bits(t), _bits(c), float(gate)) == (_bits(t0), _bits(c0), 1.0)
        assert finish_ref(part, 2, max_norm, norm_scale, scale, gate=True) == (t, c, gate)
        assert [float(x) for x in finish_ref(part, 2, max_norm, norm_scale, scale, gate=False)] == [0.0, 1.0, 0.0]
    assert [float(x) for x in finish_ref([], 2, 2.0)] == [0.0, 1.0, 1.0]              # n == 0
    assert [float(x) for x in finish_ref([], 0, 2.0)] == [0.0, 1.0, 1.0] and [float(x) for x in finish_ref([], 1, 2.0, gate=False)] == [0.0, 1.0, 0.0]


@pytest.mark.parametrize("norm_type", [1.0, INF])
@pytest.mark.parametrize("case", ["biting", "not_biting", "zero", "inf", "nan"])
def test_coefficient_arithmetic_is_torchs_for_the_other_norms(norm_type, case):
    """the restated finish, fed exact per-tensor partials (small integers over 8: every fp32 sum is exact), reproduces the total torch
    returns and the factor it multiplied the gradients by"""
    g = torch.Generator().manual_seed(6)
    grads = [torch.randint(-40, 41, s, generator=g).float() / 8 for s in ((37, 5), (13,), (3, 64), (1,))]
    max_norm = {"biting": 2.0, "not_biting": 1e5, "zero": 2.0, "inf": 2.0, "nan": 2.0}[case]
    if case == "zero":
        grads = [torch.zeros_like(t) for t in grads]
    if case == "inf":
        grads[1][3] = -INF
    if case == "nan":
        grads[2][1, 7] = float("nan")
    params = [torch.nn.Parameter(torch.zeros_like(t)) for t in grads]
    for p, t in zip(params, grads):
        p.grad = t.clone()
    probe = torch.nn.Parameter(torch.zeros(3))
    probe.grad = torch.tensor([1.0, 0.75, -3.0])
    total = torch.nn.utils.get_total_norm([p.grad for p in params], norm_type)
    torch.nn.utils.clip_grads_with_norm_(params + [probe], max_norm, total)
    part = [float(t.abs().sum()) if norm_type == 1.0 else float(t.abs().max()) for t in grads]          # (tensor.max keeps a NaN)
    t, c, gate = finish_ref(part, KINDS[norm_type], max_norm)
    factor = probe.grad[0].item()
    assert gate == 1.0
    if case == "nan":
        assert np.isnan(t) and np.isnan(c) and np.isnan(total.item()) and np.isnan(factor)
    else:
        assert _bits(t) == _bits(total.item()) and _bits(c) == _bits(factor), (float(t), total.item(), float(c), factor)
    if case == "biting":
        assert 0 < c < 1
    if case in ("not_biting", "zero"):
        assert c == 1.0
    if case == "inf":
        assert c == 0.0 and t == INF


# ------------------------------------------------------------------------------------------
# the gate's decision
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("threshold", [10, 0.1, float(np.float32(0.1))])
def test_gate_decision_is_torchs_comparison(dtype, threshold):
    npdt = np.float64 if dtype == torch.float64 else np.float32
    at = npdt(threshold)                                                             # the threshold in the loss tensor's dtype
    values = [at, np.nextafter(at, npdt(np.inf)), np.nextafter(at, npdt(-np.inf)), npdt(np.nan), npdt(np.inf), npdt(-np.inf),
              npdt(float(threshold) * 2), npdt(0.0)]
    if dtype == torch.float32:                                                        # ... and the doubles around it, rounded as a caller's cast would
        values += [npdt(np.nextafter(np.float64(threshold), np.inf)), npdt(np.nextafter(np.float64(threshold), -np.inf))]
    seen = set()
    for v in values:
        loss = torch.tensor([float(v)], dtype=torch.float64).to(dtype)
        assert loss.dtype == dtype and (np.isnan(v) or loss.item() == float(v))
        want = bool((loss > threshold).item())                                       # torch's own decision, on the CPU
        assert gate_ref(loss, threshold) == want, (dtype, threshold, float(v))
        seen.add((("nan" if np.isnan(v) else float(v)), want))
    assert ("nan", False) in seen and (INF, True) in seen and (-INF, False) in seen  # a NaN loss closes the gate, +inf opens it
    assert (float(np.nextafter(at, npdt(np.inf))), True) in seen and (float(np.nextafter(at, npdt(-np.inf))), False) in seen
    assert (float(at), False) in seen or float(at) > float(threshold)                # strictly greater, in the tensor's dtype


def test_an_fp32_loss_is_compared_with_the_rounded_threshold():
    """float32(0.1) is above the double 0.1; torch rounds the threshold to fp32 for the comparison, so the gate stays closed there --
    and an fp64 loss of the same value opens it"""
    x = float(np.float32(0.1))
    assert x > 0.1
    assert not bool((torch.tensor([x], dtype=torch.float32) > 0.1).item()) and not gate_ref(torch.tensor([x], dtype=torch.float32), 0.1)
    assert bool((torch.tensor([x], dtype=torch.float64) > 0.1).item()) and gate_ref(torch.tensor([x], dtype=torch.float64), 0.1)
    big = torch.tensor([3e38], dtype=torch.float32)                                   # a threshold past fp32's range rounds to inf
    assert not bool((big > 1e39).item()) and not gate_ref(big, 1e39)
    assert not gate_ref(torch.tensor([INF], dtype=torch.float32), 1e39) and not bool((torch.tensor([INF]) > 1e39).item())


# ------------------------------------------------------------------------------------------
# the calls clip_in_step issues
# ------------------------------------------------------------------------------------------
@pytest.fixture
def rec(monkeypatch):
    """every optimizer wrapper of vbg.ops, the old and the new norm wrappers and both finishes record instead of launching; the finishes
    return host tensors (total 4, coefficient 0.5[, gate 1])"""
    from vbg import ops
    calls = []
    for name in STEP_WRAPPERS + ("grad_sumsq_seg_inf",):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: calls.append((_n, a, k)))

    def rows(g, table, partials, kind=2, found_inf=None, gate=None):
        calls.append(("grad_norm_seg", (g, table, partials, kind, found_inf, gate), {}))

    def finish(partials, n, max_norm, norm_scale=1.0, grad_scale=None, out=None):
        calls.append(("clip_coef", (partials, n, max_norm, norm_scale, grad_scale), {}))
        return torch.tensor([4.0, 0.5])

    def finish_gate(partials, n, max_norm, norm_scale=1.0, grad_scale=None, kind=2, gate=None, out=None):
        calls.append(("clip_coef_gate", (partials, n, max_norm, norm_scale, grad_scale, kind, gate), {}))
        return torch.tensor([4.0, 0.5, 1.0])

    monkeypatch.setattr(ops, "grad_norm_seg", rows)
    monkeypatch.setattr(ops, "clip_coef", finish)
    monkeypatch.setattr(ops, "clip_coef_gate", finish_gate)
    return calls


@pytest.mark.parametrize("norm_type", [2, 2.0])
def test_a_call_without_the_new_arguments_issues_the_old_calls(rec, norm_type):
    from vbg.optim import clip_in_step
    sgd, adam = _flat_pair(False)
    clip_in_step([sgd, adam], 2.0, norm_scale=0.5, norm_type=norm_type, when=None)
    assert names(rec) == ["grad_sumsq_seg", "grad_sumsq_seg", "clip_coef"]
    assert sgd._vbg_clip is adam._vbg_clip and sgd._vbg_clip.numel() == 1 and float(sgd._vbg_clip) == 0.5


@pytest.mark.parametrize("segmented", [False, True])
@pytest.mark.parametrize("norm_type,gated", [(1, False), (1.0, True), (INF, False), (INF, True), (2, True), (2.0, True)])
def test_new_arguments_issue_the_new_pair(rec, segmented, norm_type, gated):
    from vbg.optim import clip_in_step
    sgd, adam = _flat_pair(segmented)
    loss = torch.tensor(12.5, dtype=torch.float64)
    when = (loss, 10) if gated else None
    total = clip_in_step([sgd, adam], 2.0, norm_scale=0.5, norm_type=norm_type, when=when)
    assert names(rec) == ["grad_norm_seg", "grad_norm_seg", "clip_coef_gate"]       # one row launch per optimizer, one finish
    (g1, t1, part1, k1, f1, gate1), (g2, t2, part2, k2, f2, gate2) = rec[0][1], rec[1][1]
    assert g1 is sgd.group.gflat and g2 is adam.group.gflat and t1 is sgd._clip_table() and t2 is adam._clip_table()
    assert k1 == k2 == KINDS[float(norm_type)] and f1 is None and f2 is None
    assert part1.numel() == t1.n and part2.numel() == t2.n and part2.data_ptr() == part1.data_ptr() + 4 * t1.n          # side by side
    partials, n, max_norm, norm_scale, grad_scale, kind, gate = rec[2][1]
    assert n == t1.n + t2.n and partials.data_ptr() == part1.data_ptr() and (max_norm, norm_scale, grad_scale, kind) == (2.0, 0.5, None, k1)
    for gt in (gate1, gate2, gate):
        if gated:
            assert gt[0].data_ptr() == loss.data_ptr() and gt[0].dtype == torch.float64 and gt[1] == 10      # the tensor itself, unread
        else:
            assert gt is None
    assert total.dim() == 0 and float(total) == 4.0
    coef = sgd._vbg_clip
    assert coef is adam._vbg_clip and coef.numel() == 1 and float(coef) == 0.5       # the second float of the output
    with pytest.raises(RuntimeError, match="pending"):                               # a second call before step()
        clip_in_step([adam], 2.0, when=when)
    del rec[:]
    sgd.step()
    adam.step()
    assert names(rec) == ["sgd_step_seg_clip", "adam_step_seg_clip"]                 # the coefficient reaches the step as it does today
    assert rec[0][1][7] is coef and rec[1][1][9] is coef and sgd._vbg_clip is None and adam._vbg_clip is None
    clip_in_step([sgd], 2.0, when=(loss.float(), 0.5))                               # zero_grad() drops it
    sgd.zero_grad()
    assert sgd._vbg_clip is None


def test_a_fuse_scaler_scaler_passes_one_flag_per_optimizer(rec):
    from vbg.optim import _CLIP_FLAG, clip_in_step, fuse_scaler
    named, group, a = _stock(torch.optim.SGD, amp=True, lr=0.1, momentum=0.9)
    named_b, group_b, b = _stock(torch.optim.AdamW, amp=True, lr=1e-3)
    scaler = torch.amp.GradScaler("cpu", init_scale=1024.0)
    scaler.scale(torch.zeros(()))
    scaler = fuse_scaler(scaler)
    loss = torch.tensor([3.0])
    clip_in_step([a, b], 1.0, scaler=scaler, norm_type=INF, when=(loss, 2.5))
    assert names(rec) == ["grad_norm_seg", "grad_norm_seg", "clip_coef_gate"]
    fa, fb = rec[0][1][4], rec[1][1][4]
    assert fa.numel() == fb.numel() == 1 and float(fa) == float(fb) == 0.0 and fa.dtype == torch.float32
    assert fa.data_ptr() != fb.data_ptr() and fa.untyped_storage().data_ptr() == fb.untyped_storage().data_ptr()          # one torch.zeros
    assert rec[2][1][4] is scaler._scale and rec[2][1][5] == 0
    assert scaler._per_optimizer_states[id(a)][_CLIP_FLAG][0] is fa and scaler._per_optimizer_states[id(b)][_CLIP_FLAG][0] is fb
    assert scaler._per_optimizer_states[id(a)][_CLIP_FLAG][1] is a._vbg_clip
    # a plain GradScaler: no flags, the scale still reaches the finish
    del rec[:]
    a.zero_grad(set_to_none=False)
    b.zero_grad(set_to_none=False)
    plain = torch.amp.GradScaler("cpu", init_scale=512.0)
    plain.scale(torch.zeros(()))
    clip_in_step([a, b], 1.0, scaler=plain, norm_type=1)
    assert names(rec) == ["grad_norm_seg", "grad_norm_seg", "clip_coef_gate"] and rec[0][1][4] is None and rec[1][1][4] is None
    assert rec[2][1][4] is plain._scale and rec[2][1][5] == 1


def test_a_closure_step_multiplies_by_the_pending_coefficient(rec):
    """a fallback step after a gated call: the present gradients times the device scalar, whatever the gate made of it"""
    from vbg.optim import clip_in_step
    named, group, opt = _stock(torch.optim.SGD, lr=0.1)
    g0 = group.gflat.clone()
    clip_in_step([opt], 1.0, when=(torch.tensor(3.0, dtype=torch.float64), 2))
    del rec[:]
    opt.step(lambda: torch.tensor(1.0))
    assert rec == [] and opt._vbg_fused.last_fallback == "closure" and opt._vbg_clip is None
    assert torch.equal(group.gflat[:4712], (g0 * 0.5)[:4712])                        # the recorder's coefficient


# ------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------
def test_what_the_new_arguments_refuse(rec):
    from vbg.optim import clip_in_step
    named, group, opt = _stock(torch.optim.SGD, lr=0.1)
    loss = torch.tensor(3.0, dtype=torch.float64)
    for bad in (3, 0, 0.5, -1, float("nan"), "2", None, True):
        with pytest.raises(ValueError, match="2, 1 or float"):
            clip_in_step([opt], 1.0, norm_type=bad)
    for bad in (loss, (loss,), (loss, 1.0, 2.0), 10.0):                              # not a 2-tuple
        with pytest.raises(TypeError):
            clip_in_step([opt], 1.0, when=bad)
    with pytest.raises(ValueError, match="one element"):
        clip_in_step([opt], 1.0, when=(torch.zeros(2, dtype=torch.float64), 1.0))
    with pytest.raises(ValueError, match="one element"):
        clip_in_step([opt], 1.0, when=(torch.zeros(0), 1.0))
    with pytest.raises(ValueError, match="lives on"):                                # a loss on another device than the flat buffers
        clip_in_step([opt], 1.0, when=(torch.zeros((), device="meta"), 1.0))
    for bad in (torch.tensor(3), torch.tensor(3.0, dtype=torch.float16), torch.tensor(True)):
        with pytest.raises(TypeError, match="fp64 or fp32"):
            clip_in_step([opt], 1.0, when=(bad, 1.0))
    for bad in (3.0, np.float64(3.0)):                                               # the loss is a tensor
        with pytest.raises(TypeError):
            clip_in_step([opt], 1.0, when=(bad, 1.0))
    for bad in (torch.tensor(1.0), "10", None, True):                                # the threshold is a Python number
        with pytest.raises(TypeError, match="Python number"):
            clip_in_step([opt], 1.0, when=(loss, bad))
    assert rec == [] and opt._vbg_clip is None
    clip_in_step([opt], 1.0, norm_type=1, when=(loss, 1))
    with pytest.raises(RuntimeError, match="pending"):                               # a second pending call
        clip_in_step([opt], 1.0, norm_type=1, when=(loss, 1))


def test_a_loss_on_the_cpu_is_refused_for_buffers_elsewhere():
    """a `meta` device stands in for the GPU the flat buffers live on (tests/test_gpu_clip_gate.py refuses a real one): a loss on the
    CPU is not on their device"""
    from vbg import optim as vo
    elsewhere = torch.zeros(8, device="meta").device
    with pytest.raises(ValueError, match="lives on cpu"):
        vo._clip_gate((torch.tensor(3.0, dtype=torch.float64), 1.0), elsewhere)
    assert vo._clip_gate(None, elsewhere) is None


def test_ops_wrappers_check_kind_gate_and_buffers():
    from vbg import ops
    ok = ops.chunk_table([(0, 8, 0), (8, 64, 1)], 2, 72, "cpu")
    z = lambda n=72: torch.zeros(n)
    loss = torch.tensor(3.0, dtype=torch.float64)
    with pytest.raises(ValueError, match="kind"):
        ops.grad_norm_seg(z(), ok, z(2), kind=3)
    with pytest.raises(ValueError, match="kind"):
        ops.clip_coef_gate(z(4), 4, 1.0, kind=-1)
    with pytest.raises(ValueError):                                                  # buffers shorter than the table's range
        ops.grad_norm_seg(z(64), ok, z(2), 1)
    with pytest.raises(ValueError):                                                  # one partial per row
        ops.grad_norm_seg(z(), ok, z(1), 0)
    with pytest.raises(ValueError):
        ops.grad_norm_seg(z().double(), ok, z(2), 1)
    with pytest.raises(ValueError, match="found_inf"):
        ops.grad_norm_seg(z(), ok, z(2), 1, found_inf=torch.zeros(2))
    with pytest.raises(ValueError, match="found_inf"):
        ops.grad_norm_seg(z(), ok, z(2), 1, found_inf=torch.zeros(1, dtype=torch.float64))
    for wrapper in (lambda gate: ops.grad_norm_seg(z(), ok, z(2), 1, gate=gate), lambda gate: ops.clip_coef_gate(z(4), 4, 1.0, gate=gate)):
        with pytest.raises(TypeError):
            wrapper(loss)
        with pytest.raises(TypeError):
            wrapper((3.0, 1.0))
        with pytest.raises(TypeError, match="fp64 or fp32"):
            wrapper((torch.tensor(3), 1.0))
        with pytest.raises(ValueError, match="one element"):
            wrapper((torch.zeros(2), 1.0))
        with pytest.raises(ValueError, match="device"):
            wrapper((torch.zeros((), device="meta"), 1.0))
        with pytest.raises(TypeError, match="Python number"):
            wrapper((loss, torch.tensor(1.0)))
    # well-formed arguments in host memory: refused with an exception before a pointer leaves Python (an `assert` would be gone under -O)
    for gate in (None, (loss, 1.0)):
        with pytest.raises(TypeError, match="device memory"):
            ops.grad_norm_seg(z(), ok, z(2), 1, gate=gate)
        with pytest.raises(TypeError, match="device memory"):
            ops.grad_norm_seg(z(), ok, z(2), 0, found_inf=torch.zeros(1), gate=gate)
        with pytest.raises(TypeError, match="device memory"):
            ops.clip_coef_gate(z(4), 4, 1.0, kind=0, gate=gate)
    with pytest.raises(ValueError):
        ops.clip_coef_gate(z(4), 5, 1.0)
    with pytest.raises(ValueError, match="three"):
        ops.clip_coef_gate(z(4), 4, 1.0, out=z(2))
    with pytest.raises(ValueError):
        ops.clip_coef_gate(z(4), 4, 1.0, grad_scale=torch.ones(2))
    # the rejecting cases of test_what_the_new_arguments_refuse, on the wrappers
    for wrapper in (lambda gate: ops.grad_norm_seg(z(), ok, z(2), 1, gate=gate), lambda gate: ops.clip_coef_gate(z(4), 4, 1.0, gate=gate)):
        for _, make, exc, words in BAD_GATES:
            with pytest.raises(exc, match=words):
                wrapper(make(loss))


# (what, the gate made of a good loss, what clip_in_step raises on it in test_what_the_new_arguments_refuse, its words)
BAD_GATES = [("a bare tensor", lambda loss: loss, TypeError, None), ("one element", lambda loss: (loss,), TypeError, None),
             ("three elements", lambda loss: (loss, 1.0, 2.0), TypeError, None), ("a number", lambda loss: 10.0, TypeError, None),
             ("a float loss", lambda loss: (3.0, 1.0), TypeError, None), ("a numpy loss", lambda loss: (np.float64(3.0), 1.0), TypeError, None),
             ("an integer loss", lambda loss: (torch.tensor(3), 1.0), TypeError, "fp64 or fp32"),
             ("a half loss", lambda loss: (torch.tensor(3.0, dtype=torch.float16), 1.0), TypeError, "fp64 or fp32"),
             ("a bool loss", lambda loss: (torch.tensor(True), 1.0), TypeError, "fp64 or fp32"),
             ("two losses", lambda loss: (torch.zeros(2, dtype=torch.float64), 1.0), ValueError, "one element"),
             ("no loss", lambda loss: (torch.zeros(0), 1.0), ValueError, "one element"),
             ("a loss elsewhere", lambda loss: (torch.zeros((), device="meta"), 1.0), ValueError, "lives on"),
             ("a tensor threshold", lambda loss: (loss, torch.tensor(1.0)), TypeError, "Python number"),
             ("a str threshold", lambda loss: (loss, "10"), TypeError, "Python number"),
             ("no threshold", lambda loss: (loss, None), TypeError, "Python number"), ("a bool threshold", lambda loss: (loss, True), TypeError, "Python number")]


@pytest.mark.parametrize("what,make,exc,words", BAD_GATES, ids=[b[0] for b in BAD_GATES])
def test_one_verdict_on_a_bad_gate(what, make, exc, words):
    """vbg.optim._clip_gate and the two gated ops wrappers run one statement: the same exception and the same words after the caller's
    name on every bad gate; a good gate passes all three (the wrappers get as far as refusing host memory)"""
    from vbg import ops
    from vbg import optim as vo
    ok = ops.chunk_table([(0, 8, 0), (8, 64, 1)], 2, 72, "cpu")
    cpu = torch.device("cpu")
    gate = make(torch.tensor(3.0, dtype=torch.float64))
    verdicts = []
    for call in (lambda: vo._clip_gate(gate, cpu), lambda: ops.grad_norm_seg(torch.zeros(72), ok, torch.zeros(2), 1, gate=gate),
                 lambda: ops.clip_coef_gate(torch.zeros(4), 4, 1.0, gate=gate)):
        with pytest.raises(exc, match=words) as e:
            call()
        verdicts.append((type(e.value), str(e.value).split(": ", 1)[1]))
    assert verdicts[0] == verdicts[1] == verdicts[2] and "device memory" not in verdicts[0][1], verdicts
    good = (torch.tensor(3.0), 1)
    assert vo._clip_gate(good, cpu)[1] == 1 and vo._clip_gate(list(good), cpu)[0].dtype == torch.float32
    with pytest.raises(TypeError, match="device memory"):
        ops.clip_coef_gate(torch.zeros(4), 4, 1.0, gate=good)


def _wrapper_calls():
    """every optimizer wrapper of vbg.ops that takes buffers against a chunk table: name -> (call(**buffers), its buffer arguments)"""
    from vbg import ops
    ok = ops.chunk_table([(0, 8, 0), (8, 64, 1)], 2, 72, "cpu")
    one = torch.ones(1)
    s3, a5 = [(0.1, 0.9, 0.0)] * 2, [(1e-3, 0.9, 0.999, 1e-8, 0.0)] * 2
    so, ao = [(0.1, 0.9, 0.0, 0.0, 0)] * 2, [(1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1)] * 2          # (amsgrad: vmax is a buffer of the launch)
    return {
        "sgd_step_seg": (lambda p, g, mom: ops.sgd_step_seg(p, g, mom, ok, s3, True), "p g mom"),
        "adamw_step_seg": (lambda p, g, m, v: ops.adamw_step_seg(p, g, m, v, ok, a5, 1), "p g m v"),
        "sgd_step_seg_opt": (lambda p, g, mom: ops.sgd_step_seg_opt(p, g, mom, ok, so), "p g mom"),
        "adam_step_seg_opt": (lambda p, g, m, v, vmax: ops.adam_step_seg_opt(p, g, m, v, vmax, ok, ao), "p g m v vmax"),
        "sgd_step_seg_amp": (lambda p, g, mom: ops.sgd_step_seg_amp(p, g, mom, ok, so, one, one), "p g mom"),
        "adam_step_seg_amp": (lambda p, g, m, v, vmax: ops.adam_step_seg_amp(p, g, m, v, vmax, ok, ao, one, one), "p g m v vmax"),
        "sgd_step_seg_clip": (lambda p, g, mom: ops.sgd_step_seg_clip(p, g, mom, ok, so, one, one, one), "p g mom"),
        "adam_step_seg_clip": (lambda p, g, m, v, vmax: ops.adam_step_seg_clip(p, g, m, v, vmax, ok, ao, one, one, one), "p g m v vmax"),
        "grad_sumsq_seg": (lambda g, partials: ops.grad_sumsq_seg(g, ok, partials), "g partials"),
        "grad_sumsq_seg_inf": (lambda g, partials: ops.grad_sumsq_seg_inf(g, ok, partials, one), "g partials"),
        "grad_norm_seg": (lambda g, partials: ops.grad_norm_seg(g, ok, partials, 1, one), "g partials"),
        "grad_unscale_check_seg": (lambda g: ops.grad_unscale_check_seg(g, ok, one, one), "g"),
        "clip_coef": (lambda partials, out: ops.clip_coef(partials, 2, 1.0, out=out), "partials out"),
        "clip_coef_gate": (lambda partials, out: ops.clip_coef_gate(partials, 2, 1.0, out=out), "partials out"),
    }


@pytest.mark.parametrize("name", sorted(_wrapper_calls()))
def test_every_wrapper_refuses_a_bad_buffer(name):
    """each buffer argument of each wrapper in turn: fp64, one element short, strided -- a ValueError before a pointer leaves Python"""
    call, names = _wrapper_calls()[name]
    names = names.split()
    need = {"partials": 2, "out": 3 if name == "clip_coef_gate" else 2}
    with pytest.raises((AssertionError, TypeError)):                                 # well-formed host buffers pass every check but the last
        call(**{k: torch.zeros(need.get(k, 72)) for k in names})
    for which in names:
        n = need.get(which, 72)
        for bad in (torch.zeros(n, dtype=torch.float64), torch.zeros(n - 1), torch.zeros(2 * n)[::2]):
            args = {k: (bad if k == which else torch.zeros(need.get(k, 72))) for k in names}
            with pytest.raises(ValueError):
                call(**args)


# ------------------------------------------------------------------------------------------
# the library without a GPU
# ------------------------------------------------------------------------------------------
def test_argument_errors_of_the_new_entries():
    from vbg import lib as L
    rows, coef = L.lib.vbg_grad_norm_seg, L.lib.vbg_clip_coef_gate
    buf = (C.c_float * 64)()
    a = C.cast(C.addressof(buf) + (-C.addressof(buf)) % 16, C.c_void_p)
    odd, four = C.c_void_p(a.value + 2), C.c_void_p(a.value + 4)
    for kind in (0, 1, 2):
        assert rows(None, None, 0, None, kind, None, None, 0, 0.0, None) == 0          # nchunks == 0 is a no-op
        assert rows(None, None, 0, None, kind, a, a, 1, 10.0, None) == 0
    assert rows(None, None, 0, None, 3, None, None, 0, 0.0, None) == -1 and rows(None, None, 0, None, -1, None, None, 0, 0.0, None) == -1
    assert rows(a, a, -1, a, 2, None, None, 0, 0.0, None) == -1
    assert rows(a, a, 1, None, 2, None, None, 0, 0.0, None) == -1                      # no partials
    assert rows(None, a, 1, a, 2, None, None, 0, 0.0, None) == -1 and rows(a, None, 1, a, 2, None, None, 0, 0.0, None) == -1
    assert rows(four, a, 1, a, 2, None, None, 0, 0.0, None) == -1                      # g: 16-byte alignment
    assert rows(a, a, 1, odd, 2, None, None, 0, 0.0, None) == -1                       # partials: 4-byte alignment
    assert rows(None, None, 0, None, 2, odd, None, 0, 0.0, None) == -1                 # the scalars are aligned, whatever nchunks is
    assert rows(None, None, 0, None, 2, None, odd, 0, 0.0, None) == -1
    assert rows(None, None, 0, None, 2, None, four, 1, 0.0, None) == -1                # an fp64 loss: 8 bytes
    assert rows(None, None, 0, None, 2, None, four, 0, 0.0, None) == 0
    assert rows(None, None, 0, None, 2, None, a, 2, 0.0, None) == -1                   # the dtype flag is 0 or 1
    assert coef(None, 1, 2, 2.0, 1.0, None, None, 0, 0.0, a, None) == -1               # partials missing with n > 0
    assert coef(a, 1, 2, 2.0, 1.0, None, None, 0, 0.0, None, None) == -1               # no out
    assert coef(a, -1, 2, 2.0, 1.0, None, None, 0, 0.0, a, None) == -1
    assert coef(a, 1, 3, 2.0, 1.0, None, None, 0, 0.0, a, None) == -1                  # kind
    assert coef(a, 1, 2, 2.0, 1.0, None, None, 0, 0.0, odd, None) == -1                # out, grad_scale, partials, loss: aligned
    assert coef(a, 1, 2, 2.0, 1.0, odd, None, 0, 0.0, a, None) == -1
    assert coef(odd, 1, 2, 2.0, 1.0, None, None, 0, 0.0, a, None) == -1
    assert coef(a, 1, 2, 2.0, 1.0, None, odd, 0, 0.0, a, None) == -1
    assert coef(a, 1, 2, 2.0, 1.0, None, four, 1, 0.0, a, None) == -1
    assert coef(a, 1, 2, 2.0, 1.0, None, a, 5, 0.0, a, None) == -1
