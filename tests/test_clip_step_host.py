"""vbg.optim.clip_in_step, the host side (no GPU, no launch): the fp32 arithmetic of the finish (vbg_clip_coef) restated and held against
the factor torch.nn.utils.clip_grad_norm_ applies, bit for bit; the pending coefficient with the ops wrappers replaced by recorders
(the `recorder` pattern of tests/test_stock_optim_host.py) -- one norm call per optimizer and one finish, the next step() through the
*_seg_clip wrapper with that tensor, the step after it through the plain wrapper, a second call raising, zero_grad() dropping it, a
closure step multiplying the gradients, `.grad is None` parameters in no row of the norm table; and the argument checks of the four new
entries, which return before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_optim_groups_host import CHUNK, LAYOUT, TOTAL, expected_chunks, six_params, split
from test_stock_optim_host import homed, two_groups

f32 = np.float32


def coef_ref(total, max_norm, norm_scale=1.0, grad_scale=None):
    """vbg_clip_coef's arithmetic after the sum, one fp32 operation per line: total = (float)sqrt(sum) as handed in; -> (total, coef).
    torch evaluates `max_norm / (total_norm + 1e-6)` as `(total_norm + 1e-6).reciprocal() * max_norm` (Tensor.__rdiv__), and
    `clamp(max=1.0)` keeps a NaN"""
    with np.errstate(all="ignore"):
        t = f32(f32(total) * f32(norm_scale))
        if grad_scale is not None:
            t = f32(t * f32(1.0 / float(f32(grad_scale))))
        d = f32(t + f32(1e-6))
        r = f32(f32(1.0) / d)
        c = f32(r * f32(max_norm))
    return t, (f32(1.0) if c > f32(1.0) else c)


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.int32).item()


@pytest.mark.parametrize("case", ["biting", "biting_0.37", "not_biting", "zero", "inf", "nan"])
def test_coefficient_arithmetic_is_torchs(case):
    """the restated finish, fed torch's own total_norm, reproduces the factor clip_grad_norm_ multiplied the gradients by"""
    g = torch.Generator().manual_seed(5)
    grads = [torch.randn(s, generator=g) for s in ((37, 5), (13,), (3, 64), (1,))]
    max_norm = {"biting": 2.0, "biting_0.37": 0.37, "not_biting": 1e3, "zero": 2.0, "inf": 2.0, "nan": 2.0}[case]
    if case == "zero":
        grads = [torch.zeros_like(t) for t in grads]
    if case == "inf":
        grads[1][3] = float("inf")
    if case == "nan":
        grads[2][1, 7] = float("nan")
    params = [torch.nn.Parameter(torch.zeros_like(t)) for t in grads]
    probe = torch.nn.Parameter(torch.zeros(3))          # a finite gradient that shows the factor itself: (1, 0.75, -3) * factor
    for p, t in zip(params, grads):
        p.grad = t.clone()
    probe.grad = torch.tensor([1.0, 0.75, -3.0])
    # (the probe is clipped by the same call but must not count towards the norm: torch's two halves, called as clip_grad_norm_ calls them)
    total = torch.nn.utils.get_total_norm([p.grad for p in params], 2.0)
    torch.nn.utils.clip_grads_with_norm_(params + [probe], max_norm, total)
    assert total.dtype == torch.float32
    t, c = coef_ref(total.item(), max_norm)
    assert _bits(t) == _bits(total.item())
    factor = probe.grad[0].item()
    if case == "nan":
        assert np.isnan(c) and np.isnan(factor) and bool(torch.isnan(probe.grad).all())
    else:
        assert _bits(c) == _bits(factor), (float(c), factor)
        assert torch.equal(probe.grad, torch.tensor([1.0, 0.75, -3.0]) * torch.tensor(float(c)))
    if case.startswith("biting"):
        assert 0 < c < 1 and not torch.equal(params[0].grad, grads[0])
    if case in ("not_biting", "zero"):
        assert c == 1.0 and all(torch.equal(p.grad, t) for p, t in zip(params, grads))
    if case == "inf":
        assert c == 0.0 and np.isinf(t)
    # ... and clip_grad_norm_ itself is those two halves
    for p, t in zip(params, grads):
        p.grad = t.clone()
    assert _bits(torch.nn.utils.clip_grad_norm_(params, max_norm).item()) == _bits(total.item())
    if case not in ("nan", "inf"):
        assert all(torch.equal(p.grad, t * torch.tensor(float(c))) for p, t in zip(params, grads))


def test_the_scaled_total_of_the_restatement():
    """with a scale the total is divided on the device: torch's inverse, `scale.double().reciprocal().float()`, one rounded product"""
    for scale in (1024.0, 1000.0):
        inv = torch.full((), scale).double().reciprocal().float()
        for max_norm in (0.37, 2.0):
            t, c = coef_ref(3.5 * scale, max_norm, 0.5, scale)
            assert _bits(t) == _bits((torch.tensor(3.5 * scale) * 0.5 * inv).item())
            assert _bits(c) == _bits(torch.clamp(max_norm / (torch.tensor(float(t)) + 1e-6), max=1.0).item())
            assert (c == 1.0) == (max_norm == 2.0)


# ------------------------------------------------------------------------------------------
# the pending coefficient
# ------------------------------------------------------------------------------------------
STEP_WRAPPERS = ("sgd_step", "adamw_step", "sgd_step_seg", "adamw_step_seg", "sgd_step_seg_opt", "adam_step_seg_opt", "sgd_step_seg_amp",
                 "adam_step_seg_amp", "sgd_step_seg_clip", "adam_step_seg_clip", "grad_sumsq_seg")


@pytest.fixture
def rec(monkeypatch):
    """every optimizer wrapper of vbg.ops and the two clip wrappers record their arguments instead of launching; the finish returns a
    host tensor (total 4, coefficient 0.5)"""
    from vbg import ops
    calls = []
    for name in STEP_WRAPPERS:
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: calls.append((_n, a, k)))

    def finish(partials, n, max_norm, norm_scale=1.0, grad_scale=None, out=None):
        calls.append(("clip_coef", (partials, n, max_norm, norm_scale, grad_scale), {}))
        return torch.tensor([4.0, 0.5])

    monkeypatch.setattr(ops, "clip_coef", finish)
    return calls


def names(calls):
    return [c[0] for c in calls]


def _flat_pair(segmented):
    from vbg.optim import FusedAdamW, FusedSGD
    n1, l1 = six_params("cpu", seed=1)
    n2, l2 = six_params("cpu", seed=2)
    if segmented:
        return (FusedSGD(split(n1, l1, weight_decay=0.0), "cpu", lr=0.1, momentum=0.9, seg_chunk=CHUNK, layout=n1),
                FusedAdamW(split(n2, l2, weight_decay=0.0), "cpu", lr=1e-3, seg_chunk=CHUNK, layout=n2))
    return FusedSGD(n1, "cpu", lr=0.1, momentum=0.9), FusedAdamW(n2, "cpu", lr=1e-3)


@pytest.mark.parametrize("segmented", [False, True])
def test_flat_optimizers_norm_calls_then_clip_step_then_plain_step(rec, segmented):
    from vbg import ops
    from vbg.optim import clip_in_step
    sgd, adam = _flat_pair(segmented)
    total = clip_in_step([sgd, adam], 2.0, norm_scale=0.5)
    assert names(rec) == ["grad_sumsq_seg", "grad_sumsq_seg", "clip_coef"]          # one norm call per optimizer, one finish
    (g1, t1, part1), (g2, t2, part2) = rec[0][1], rec[1][1]
    assert g1 is sgd.group.gflat and g2 is adam.group.gflat
    assert part1.numel() == t1.n and part2.numel() == t2.n
    assert part2.data_ptr() == part1.data_ptr() + 4 * t1.n                          # side by side in one buffer
    partials, n, max_norm, norm_scale, grad_scale = rec[2][1]
    assert n == t1.n + t2.n and partials.data_ptr() == part1.data_ptr() and (max_norm, norm_scale, grad_scale) == (2.0, 0.5, None)
    if segmented:
        assert t1 is sgd.table and t2 is adam.table
    else:                                                                            # one kernel group over the whole layout, rows of SEG_CHUNK
        assert (t1.n, t1.ngroups, t1.numel) == (2, 1, TOTAL) and t1.rows.view(-1).tolist() == [0, 0, 4096, 0, 4096, 0, TOTAL - 4096, 0]
    assert total.dim() == 0 and float(total) == 4.0
    coef = sgd._vbg_clip
    assert coef is adam._vbg_clip and coef.numel() == 1 and float(coef) == 0.5
    with pytest.raises(RuntimeError, match="pending"):                               # a second call before step()
        clip_in_step([adam], 2.0)
    del rec[:]
    sgd.grad_scale = 0.25
    sgd.step()
    adam.step()
    assert names(rec) == ["sgd_step_seg_clip", "adam_step_seg_clip"]
    (name, a, k), (_, b, kb) = rec
    assert a[0] is sgd.group.pflat and a[1] is sgd.group.gflat and a[2] is sgd.mom and a[3] is t1
    assert a[5:] == (None, None, coef, 0.25) and k == {"keep_mom": True}
    assert all(h[2] == 0.0 and h[4] == ops.SGD_FIRST for h in a[4]) and len(a[4]) == (2 if segmented else 1)
    assert b[5] is t2 and b[4] is None and b[7:] == (None, None, coef, 1.0)
    assert all(h[5] == 1 and h[6] == 0 for h in b[6])
    assert sgd._vbg_clip is None and adam._vbg_clip is None
    del rec[:]
    sgd.step()
    adam.step()
    assert names(rec) == (["sgd_step_seg", "adamw_step_seg"] if segmented else ["sgd_step", "adamw_step"])          # the plain wrappers again
    # zero_grad() drops a pending coefficient
    del rec[:]
    clip_in_step([sgd, adam], 2.0)
    sgd.zero_grad()
    assert sgd._vbg_clip is None and adam._vbg_clip is not None
    sgd.step()
    adam.step()
    assert names(rec)[3:] == [("sgd_step_seg" if segmented else "sgd_step"), "adam_step_seg_clip"]
    assert all(h[5] == 3 for h in rec[-1][1][6])                                     # Adam's third step


def _stock(cls=torch.optim.SGD, amp=False, **kw):
    from vbg.optim import fuse
    named, letters, group = homed()
    opt = fuse(cls(two_groups(named, letters), **kw), seg_chunk=CHUNK, amp_scaling=amp)
    return named, group, opt


def test_stock_optimizer_norm_table_skips_grad_none_and_the_step_takes_the_coefficient(rec):
    from vbg.optim import clip_in_step
    named, group, opt = _stock(torch.optim.AdamW, lr=1e-3)
    by = dict(named)
    by["head.bias"].grad = None                                                      # slot [8, 24)
    by["mid.weight"].grad = None                                                     # slot [216, 408)
    clip_in_step([opt], 1.0)
    assert names(rec) == ["grad_sumsq_seg", "clip_coef"]
    g, table, part = rec[0][1]
    assert g is group.gflat and part.numel() == table.n == rec[1][1][1]
    covered = np.zeros(TOTAL, dtype=bool)
    for s, n, _ in table.chunk_rows:
        assert not covered[s:s + n].any()
        covered[s:s + n] = True
    assert not covered[8:24].any() and not covered[216:408].any() and not covered[4712:].any()
    assert covered[0:8].all() and covered[24:216].all() and covered[408:4712].all()
    coef = opt._vbg_clip
    with pytest.raises(RuntimeError, match="pending"):
        clip_in_step([opt], 1.0)
    del rec[:]
    opt.step()
    assert names(rec) == ["adam_step_seg_clip"] and opt._vbg_clip is None
    a = rec[0][1]
    assert a[1] is group.gflat and a[7:] == (None, None, coef)
    assert a[5].ngroups == 2 and int(a[5].chunk_rows[:, 1].sum()) == int(table.chunk_rows[:, 1].sum())          # the step's table: the same elements, two kernel groups
    opt.step()
    assert names(rec) == ["adam_step_seg_clip", "adam_step_seg_opt"]
    assert (opt._vbg_fused.launches, opt._vbg_fused.fallbacks) == (2, 0)
    # everything present: the rows of the full layout
    del rec[:]
    group.zero_grad()
    clip_in_step([opt], 1.0)
    want = np.array([(s, min(CHUNK, 4712 - s), 0) for s in range(0, 4712, CHUNK)], dtype=np.int64)
    assert np.array_equal(rec[0][1][1].chunk_rows, want)
    assert int(expected_chunks()[:, 1].sum()) == 4712
    opt.zero_grad()                                                                  # torch's zero_grad on the fused object drops it too
    assert opt._vbg_clip is None


def test_a_closure_step_multiplies_the_gradients_first(rec):
    from vbg.optim import clip_in_step
    named, group, opt = _stock(torch.optim.SGD, lr=0.1)
    dict(named)["head.bias"].grad = None
    g0 = group.gflat.clone()
    p0 = group.pflat.clone()
    clip_in_step([opt], 1.0)
    del rec[:]
    opt.step(lambda: torch.tensor(1.0))
    assert rec == [] and opt._vbg_fused.last_fallback == "closure" and opt._vbg_clip is None
    half = g0 * 0.5                                                                  # the recorder's coefficient, on the present gradients
    half[8:24] = g0[8:24]                                                            # (head.bias, grad None: not a gradient, not multiplied)
    assert torch.equal(group.gflat, half)
    want = torch.add(p0, half, alpha=-0.1)
    want[8:24] = p0[8:24]                                                            # ... and torch's step skips it
    assert torch.equal(group.pflat, want)
    # any other fallback reason does the same: a foreign .grad
    q = named[0][1]
    q.grad = q.grad.clone()
    with pytest.raises(RuntimeError, match="flat"):                                  # ... which clip_in_step itself cannot take the norm of
        clip_in_step([opt], 1.0)
    assert opt._vbg_clip is None


def test_a_fallback_after_the_norm_applies_the_coefficient(rec):
    """the gradients are the flat views when clip_in_step runs; step() then falls back (33 param groups: more combinations than a launch
    carries) -- torch's own step runs on the clipped gradients"""
    from vbg.optim import FlatGroup, clip_in_step, fuse
    named = [(f"p{i}", torch.nn.Parameter(torch.ones(3))) for i in range(33)]
    FlatGroup(named, "cpu").gflat.fill_(1.0)
    opt = fuse(torch.optim.SGD([{"params": [p]} for _, p in named], lr=0.1))
    clip_in_step([opt], 1.0)
    opt.step()
    assert "33 combinations" in opt._vbg_fused.last_fallback and names(rec) == ["grad_sumsq_seg", "clip_coef"]
    assert all(torch.equal(p.grad, torch.full((3,), 0.5)) and torch.equal(p.detach(), torch.full((3,), 0.95)) for _, p in named)


def test_amp_protocol_hands_scale_flag_and_coefficient_to_one_call(rec):
    """fuse(amp_scaling=True): with GradScaler's two attributes on the object the clipping step gets all three device scalars, and the
    undo bookkeeping of a skipped step is what it is without a clip"""
    from vbg.optim import clip_in_step
    named, group, opt = _stock(torch.optim.SGD, amp=True, lr=0.1, momentum=0.9)
    clip_in_step([opt], 1.0)
    coef = opt._vbg_clip
    opt.grad_scale, opt.found_inf = torch.full((), 1024.0), torch.full((), 1.0)
    opt.step()
    del opt.grad_scale, opt.found_inf
    assert names(rec)[2:] == ["sgd_step_seg_clip"]
    a = rec[2][1]
    assert float(a[5]) == 1024.0 and float(a[6]) == 1.0 and a[7] is coef
    opt._vbg_fused.reconcile()
    assert opt._vbg_fused.skipped == 1 and all("momentum_buffer" not in opt.state.get(p, {}) for _, p in named)
    assert opt._vbg_clip is None                                                     # the skipped step consumed it
    clip_in_step([opt], 1.0)                                                         # so the next iteration's call does not raise


def test_what_clip_in_step_refuses(rec):
    from vbg.optim import clip_in_step
    named, group, opt = _stock(torch.optim.SGD, lr=0.1)
    with pytest.raises(ValueError):
        clip_in_step([], 1.0)
    with pytest.raises(TypeError):
        clip_in_step([torch.optim.SGD([p for _, p in named], lr=0.1)], 1.0)
    with pytest.raises(TypeError):
        clip_in_step([opt], 1.0, norm_type=1)                                        # other norm types are not offered
    scaler = torch.amp.GradScaler("cpu", init_scale=1024.0)
    with pytest.raises(RuntimeError, match="scaled a loss"):
        clip_in_step([opt], 1.0, scaler=scaler)
    scaler.scale(torch.zeros(()))
    scaler.unscale_(opt)
    with pytest.raises(RuntimeError, match="unscale_"):
        clip_in_step([opt], 1.0, scaler=scaler)
    assert rec == [] and opt._vbg_clip is None
    scaler = torch.amp.GradScaler("cpu", init_scale=1024.0)
    scaler.scale(torch.zeros(()))
    clip_in_step([opt], 1.0, scaler=scaler)
    assert float(rec[1][1][4]) == 1024.0                                             # the finish reads the scaler's own scale tensor
    assert rec[1][1][4] is scaler._scale


# ------------------------------------------------------------------------------------------
# the library without a GPU
# ------------------------------------------------------------------------------------------
def test_argument_errors_of_the_new_entries():
    from vbg import lib as L
    norm, coef, sgd, adam = L.lib.vbg_grad_sumsq_seg, L.lib.vbg_clip_coef, L.lib.vbg_sgd_step_seg_clip, L.lib.vbg_adam_step_seg_clip
    hs, ha = (L.SgdGroupOpt * 2)(), (L.AdamGroupOpt * 2)()
    for h in ha:
        h.step = 1
    buf = (C.c_float * 64)()
    a = C.cast(C.addressof(buf) + (-C.addressof(buf)) % 16, C.c_void_p)
    assert norm(None, None, 0, None, None) == 0                                      # nchunks == 0 is a no-op
    assert norm(a, a, -1, a, None) == -1
    assert norm(a, a, 1, None, None) == -1                                           # no partials
    assert norm(None, a, 1, a, None) == -1 and norm(a, None, 1, a, None) == -1
    assert norm(C.c_void_p(a.value + 4), a, 1, a, None) == -1                        # g: 16-byte alignment
    assert coef(None, 1, 2.0, 1.0, None, a, None) == -1                              # partials missing with n > 0
    assert coef(a, 1, 2.0, 1.0, None, None, None) == -1 and coef(a, -1, 2.0, 1.0, None, a, None) == -1
    for ng in (1, 2):
        assert sgd(None, None, None, None, 0, hs, ng, None, None, a, 1.0, 0, None) == 0          # nchunks == 0 is a no-op
        assert adam(None, None, None, None, None, None, 0, ha, ng, None, None, a, 1.0, None) == 0
    assert sgd(None, None, None, None, 0, hs, 1, None, a, None, 1.0, 0, None) == -1  # clip_coef is required, whatever else is there
    assert adam(None, None, None, None, None, None, 0, ha, 1, a, a, None, 1.0, None) == -1
    assert sgd(a, a, a, a, 1, hs, 1, None, None, None, 1.0, 0, None) == -1
    assert adam(a, a, a, a, None, a, 1, ha, 1, None, None, None, 1.0, None) == -1
    assert sgd(None, None, None, None, 0, hs, 0, None, None, a, 1.0, 0, None) == -1 and sgd(None, None, None, None, 0, hs, 33, None, None, a, 1.0, 0, None) == -1
    assert sgd(None, None, None, None, 1, hs, 1, None, None, a, 1.0, 0, None) == -1  # null operands with work to do
    assert sgd(a, a, None, a, 1, hs, 1, None, None, a, 1.0, 1, None) == -1           # keep_mom without a momentum buffer
    odd = C.c_void_p(a.value + 2)
    assert sgd(None, None, None, None, 0, hs, 1, None, None, odd, 1.0, 0, None) == -1          # the scalars are 4-byte aligned
    assert adam(None, None, None, None, None, None, 0, ha, 1, odd, None, a, 1.0, None) == -1
    # the *_amp entries still require found_inf
    assert L.lib.vbg_sgd_step_seg_amp(None, None, None, None, 0, hs, 1, None, None, None) == -1
    assert L.lib.vbg_sgd_step_seg_amp(None, None, None, None, 0, hs, 1, None, a, None) == 0


def test_ops_wrappers_check_the_scalars_and_buffers():
    from vbg import ops
    ok = ops.chunk_table([(0, 8, 0), (8, 64, 1)], 2, 72, "cpu")
    z = lambda n=72: torch.zeros(n)
    one = torch.ones(1)
    sgd_hp, adam_hp = [(0.1, 0.9, 0.0, 0.0, 0)] * 2, [(1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0)] * 2
    for bad in (None, torch.ones(2), torch.ones(1, dtype=torch.float64), 0.5):       # clip_coef: one fp32 element, required
        with pytest.raises(ValueError, match="clip_coef"):
            ops.sgd_step_seg_clip(z(), z(), z(), ok, sgd_hp, None, None, bad)
        with pytest.raises(ValueError, match="clip_coef"):
            ops.adam_step_seg_clip(z(), z(), z(), z(), None, ok, adam_hp, None, None, bad)
    with pytest.raises(ValueError, match="found_inf"):
        ops.sgd_step_seg_clip(z(), z(), z(), ok, sgd_hp, None, torch.ones(2), one)
    with pytest.raises(ValueError, match="grad_scale"):
        ops.adam_step_seg_clip(z(), z(), z(), z(), None, ok, adam_hp, one.double(), None, one)
    with pytest.raises(ValueError):                                                  # keep_mom needs the buffer
        ops.sgd_step_seg_clip(z(), z(), None, ok, [(0.1, 0.0, 0.0, 0.0, 0)] * 2, None, None, one, keep_mom=True)
    with pytest.raises(ValueError):                                                  # buffers shorter than the table's range
        ops.sgd_step_seg_clip(z(), z(64), z(), ok, sgd_hp, None, None, one)
    with pytest.raises(ValueError):
        ops.grad_sumsq_seg(z(64), ok, z(2))
    with pytest.raises(ValueError):                                                  # one partial per row
        ops.grad_sumsq_seg(z(), ok, z(1))
    with pytest.raises(ValueError):
        ops.grad_sumsq_seg(z().double(), ok, z(2))
    with pytest.raises(ValueError):
        ops.clip_coef(z(4), 5, 1.0)
    with pytest.raises(ValueError):
        ops.clip_coef(z(4), 4, 1.0, out=z(1))
    with pytest.raises(ValueError):
        ops.clip_coef(z(4), 4, 1.0, grad_scale=torch.ones(2))
