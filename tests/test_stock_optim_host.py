"""vbg.optim.fuse, the host side (no GPU, no launch: the two new entries are replaced by recorders): what fuse refuses, the class
switch, the fallbacks to torch's own step, the kernel groups and chunk rows over the six-parameter LAYOUT of
tests/test_optim_groups_host.py with everything present and with two parameters absent, state keys against a torch twin, and the
argument checks / struct layouts of vbg_sgd_step_seg_opt / vbg_adam_step_seg_opt."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from test_optim_groups_host import CHUNK, LAYOUT, OFFSETS, RUNS, TOTAL, expected_chunks, six_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [n for n, _, _ in LAYOUT]


def sgd_opt_ref(p, g, mom, lr, momentum, dampening, wd, flags, gs):
    """vbg_sgd_step_seg_opt's rule for one group (torch 2.10 _single_tensor_sgd, gradient scaled by gs), in the dtype of the operands;
    flags: 1 nesterov, 2 maximize, 4 first.  -> (p, mom); mom comes back untouched when momentum is 0"""
    d = (-g if flags & 2 else g) * gs + wd * p
    if momentum != 0:
        mom = d if flags & 4 else momentum * mom + (1 - dampening) * d
        d = d + momentum * mom if flags & 1 else mom
    return p - lr * d, mom


def adam_opt_ref(p, g, m, v, vmax, lr, b1, b2, eps, wd, step, flags, gs):
    """vbg_adam_step_seg_opt's rule for one group (torch 2.10 _single_tensor_adam); flags: 1 amsgrad, 2 maximize, 4 coupled weight decay.
    -> (p, m, v, vmax); vmax comes back untouched without amsgrad"""
    g = (-g if flags & 2 else g) * gs
    if flags & 4:
        g = g + wd * p
    else:
        p = p * (1 - lr * wd)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    s = v
    if flags & 1:
        s = vmax = torch.maximum(vmax, v)
    denom = s.sqrt() / (1 - b2 ** step) ** 0.5 + eps
    return p - lr / (1 - b1 ** step) * (m / denom), m, v, vmax


SGD_CASES = [dict(momentum=0.9, nesterov=True, weight_decay=0.01), dict(momentum=0.9, dampening=0.3), dict(momentum=0.0, maximize=True, weight_decay=0.1),
             dict(momentum=0.5, dampening=0.2, maximize=True, weight_decay=0.01)]
# (class, constructor arguments, what the param group overrides: torch.optim.AdamW takes decoupled_weight_decay only there)
ADAM_CASES = [(torch.optim.AdamW, dict(amsgrad=True), {}), (torch.optim.Adam, dict(weight_decay=0.01, maximize=True), {}),
              (torch.optim.AdamW, dict(weight_decay=0.1), {}), (torch.optim.AdamW, dict(amsgrad=True, weight_decay=0.05), dict(decoupled_weight_decay=False)),
              (torch.optim.Adam, dict(decoupled_weight_decay=True, weight_decay=0.05), {})]


def test_the_restated_rules_are_torch_optim():
    """the two restatements against torch.optim 2.10 in fp64, four steps whose gradients shrink and grow (amsgrad's maximum matters)"""
    g0 = torch.Generator().manual_seed(9)
    p0 = torch.randn(257, generator=g0, dtype=torch.float64)
    grads = [torch.randn(257, generator=g0, dtype=torch.float64) * s for s in (2.0, 0.1, 0.05, 1.5)]
    for kw in SGD_CASES:
        q = torch.nn.Parameter(p0.clone())
        opt = torch.optim.SGD([q], lr=0.05, **kw)
        p, mom = p0.clone(), torch.zeros_like(p0)
        flags = 1 * bool(kw.get("nesterov")) + 2 * bool(kw.get("maximize"))
        for i, g in enumerate(grads):
            q.grad = g.clone()
            opt.step()
            p, mom = sgd_opt_ref(p, g, mom, 0.05, kw["momentum"], kw.get("dampening", 0), kw.get("weight_decay", 0), flags | (4 if i == 0 else 0), 1.0)
            assert float((p - q.detach()).abs().max()) <= 5e-16 * float(p.abs().max()), kw
        if kw["momentum"]:
            assert float((mom - opt.state[q]["momentum_buffer"]).abs().max()) <= 5e-16 * float(mom.abs().max())
    for cls, kw, over in ADAM_CASES:
        q = torch.nn.Parameter(p0.clone())
        opt = cls([dict(params=[q], **over)], lr=1e-2, betas=(0.9, 0.99), eps=1e-8, **kw)
        pg = opt.param_groups[0]
        flags = 1 * bool(pg["amsgrad"]) + 2 * bool(pg["maximize"]) + 4 * (not pg["decoupled_weight_decay"])
        assert (flags & 4 == 0) == ((cls is torch.optim.AdamW) != ("decoupled_weight_decay" in {**kw, **over}))
        p, m, v, vmax = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0), torch.zeros_like(p0)
        for i, g in enumerate(grads):
            q.grad = g.clone()
            opt.step()
            p, m, v, vmax = adam_opt_ref(p, g, m, v, vmax, 1e-2, 0.9, 0.99, 1e-8, pg["weight_decay"], i + 1, flags, 1.0)
            assert float((p - q.detach()).abs().max()) <= 5e-16 * float(p.abs().max()), (cls, kw, i)
        st = opt.state[q]
        assert float((m - st["exp_avg"]).abs().max()) <= 5e-16 * float(m.abs().max()) and float((v - st["exp_avg_sq"]).abs().max()) <= 5e-16 * float(v.abs().max())
        if flags & 1:
            assert float((vmax - st["max_exp_avg_sq"]).abs().max()) <= 5e-16 * float(vmax.abs().max()) and bool((vmax > v).any())


def homed(seed=0):
    """the six parameters homed in one FlatGroup on the CPU, gradients set: (registration-order list, letters, group)"""
    from vbg.optim import FlatGroup
    named, letters = six_params("cpu", seed=seed)
    group = FlatGroup(named, "cpu")
    assert group.names == NAMES and group.offsets == OFFSETS and group.total == TOTAL
    g = torch.Generator().manual_seed(seed + 50)
    for _, p in named:
        p.grad.copy_(torch.randn(p.shape, generator=g))
    return named, letters, group


def two_groups(named, letters, **b):
    return [{"params": [p for n, p in named if letters[n] == "A"]}, {"params": [p for n, p in named if letters[n] == "B"], **b}]


@pytest.fixture
def recorder(monkeypatch):
    """ops.sgd_step_seg_opt / ops.adam_step_seg_opt record their arguments instead of launching"""
    from vbg import ops
    calls = []
    for name in ("sgd_step_seg_opt", "adam_step_seg_opt"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: calls.append((_n, a)))
    return calls


def test_fuse_refuses_what_it_cannot_keep_exact():
    from vbg.optim import FusedSGD, fuse
    named, letters, _ = homed()
    params = [p for _, p in named]

    class MySGD(torch.optim.SGD):
        pass

    for bad in (MySGD(params, lr=0.1), torch.optim.RMSprop(params, lr=0.1), torch.optim.Adamax(params, lr=0.1), object()):
        with pytest.raises(ValueError, match="exactly"):
            fuse(bad)
    n2, _ = six_params("cpu")
    with pytest.raises(ValueError):
        fuse(FusedSGD(n2, "cpu", lr=0.1))
    for cls, kw in ((torch.optim.Adam, {"capturable": True}), (torch.optim.AdamW, {"differentiable": True}), (torch.optim.SGD, {"differentiable": True})):
        with pytest.raises(ValueError, match="capturable|differentiable"):
            fuse(cls(params, lr=0.1, **kw))
        opt = cls(two_groups(named, letters), lr=0.1)
        opt.param_groups[1][next(iter(kw))] = True                                   # in ANY group
        with pytest.raises(ValueError):
            fuse(opt)
        assert type(opt) is cls                                                      # refused before anything was switched


def test_class_switch_keeps_the_object_and_its_type():
    from vbg.optim import fuse
    named, letters, _ = homed()
    for cls in (torch.optim.SGD, torch.optim.Adam, torch.optim.AdamW):
        opt = cls(two_groups(named, letters, lr=0.5), lr=0.1)
        groups, state = opt.param_groups, opt.state
        got = fuse(opt)
        assert got is opt and isinstance(opt, cls) and type(opt) is not cls and issubclass(type(opt), cls)
        assert opt.param_groups is groups and opt.state is state and opt.param_groups[1]["lr"] == 0.5
        assert isinstance(opt, torch.optim.AdamW) == (cls is torch.optim.AdamW)
        with pytest.raises(ValueError):                                              # a fused object is no longer exactly a torch class
            fuse(opt)
        sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.1)         # schedulers built afterwards are fine
        assert sched.optimizer is opt


def test_a_scheduler_built_first_is_an_error():
    from vbg.optim import fuse
    named, _, _ = homed()
    opt = torch.optim.SGD([p for _, p in named], lr=0.1)
    torch.optim.lr_scheduler.StepLR(opt, step_size=1)
    with pytest.raises(ValueError, match="before building"):
        fuse(opt)
    assert type(opt) is torch.optim.SGD


def _plain_and_fused(cls, named, letters, **kw):
    """a fused optimizer over `named` and a plain torch one over CPU copies with the same gradients"""
    from vbg.optim import fuse
    twin = [(n, torch.nn.Parameter(p.detach().clone())) for n, p in named]
    for (_, p), (_, q) in zip(named, twin):
        q.grad = None if p.grad is None else p.grad.detach().clone()
    return fuse(cls(two_groups(named, letters), **kw), seg_chunk=CHUNK), cls(two_groups(twin, letters), **kw), twin


def test_fallbacks_run_the_parent_step(recorder):
    from vbg.optim import FlatGroup, fuse
    kw = dict(lr=0.1, momentum=0.9)
    # (a) parameters that are not homed: torch's step, same result as a plain object
    named, letters = six_params("cpu")
    for _, p in named:
        p.grad = torch.ones_like(p)
    opt, plain, twin = _plain_and_fused(torch.optim.SGD, named, letters, **kw)
    opt.step()
    plain.step()
    assert recorder == [] and opt._vbg_fused.fallbacks == 1 and "homed" in opt._vbg_fused.last_fallback
    assert all(torch.equal(p, q) for (_, p), (_, q) in zip(named, twin))
    assert all(torch.equal(opt.state[p]["momentum_buffer"], plain.state[q]["momentum_buffer"]) for (_, p), (_, q) in zip(named, twin))
    # ... homed afterwards: the next call is the fused one, and the state torch made is copied into the flat buffer and re-pointed
    group = FlatGroup(named, "cpu")
    bufs = {n: opt.state[p]["momentum_buffer"].clone() for n, p in named}
    opt.step()
    assert [c[0] for c in recorder] == ["sgd_step_seg_opt"] and opt._vbg_fused.launches == 1
    mom = recorder[0][1][2]
    for n, p in named:
        i = group.names.index(n)
        st = opt.state[p]["momentum_buffer"]
        assert st.data_ptr() == mom.data_ptr() + 4 * OFFSETS[i] and torch.equal(st, bufs[n]) and st.shape == p.shape
    assert all(h[4] == 0 for h in recorder[0][1][4])                                 # nobody is on a first step
    # (b) a foreign .grad
    del recorder[:]
    p0 = named[0][1]
    p0.grad = p0.grad.clone()
    opt.step()
    assert recorder == [] and "gradient view" in opt._vbg_fused.last_fallback
    group.zero_grad()
    # (c) a closure (a sparse .grad is case (b): it cannot be the flat view)
    seen = []
    opt.step(lambda: seen.append(1) or torch.tensor(3.0))
    assert recorder == [] and seen == [1] and opt._vbg_fused.last_fallback == "closure"
    # (d) a parameter that moved away from the flat buffer
    opt.step()
    assert len(recorder) == 1
    p0.data = p0.data.clone()
    opt.step()
    assert len(recorder) == 1 and "moved away" in opt._vbg_fused.last_fallback
    # (e) a parameter outside the group with a gradient
    named2, letters2, group2 = homed(seed=2)
    extra = torch.nn.Parameter(torch.zeros(3))
    opt2 = fuse(torch.optim.SGD(two_groups(named2, letters2) + [{"params": [extra]}], **kw), seg_chunk=CHUNK)
    opt2.step()
    assert len(recorder) == 2                                                        # grad None outside the group: fine
    extra.grad = torch.ones(3)
    opt2.step()
    assert len(recorder) == 2 and "not homed" in opt2._vbg_fused.last_fallback
    assert torch.equal(extra.detach(), torch.full((3,), -0.1))                       # torch stepped it


def test_more_than_32_combinations_fall_back(recorder):
    from vbg.optim import FlatGroup, fuse
    named = [(f"p{i}", torch.nn.Parameter(torch.ones(3))) for i in range(33)]
    FlatGroup(named, "cpu").gflat.fill_(1.0)
    for cls in (torch.optim.SGD, torch.optim.AdamW):
        opt = fuse(cls([{"params": [p]} for _, p in named[:32]], lr=0.1))
        opt.step()
        assert len(recorder) == 1 and len(recorder[0][1][-2]) == 32                  # 32 are fine
        del recorder[:]
        opt = fuse(cls([{"params": [p]} for _, p in named], lr=0.1))
        before = [p.detach().clone() for _, p in named]
        opt.step()
        assert recorder == [] and "33 combinations" in opt._vbg_fused.last_fallback
        assert all(not torch.equal(b, p) for b, (_, p) in zip(before, named))        # torch's step ran
    # one param group, 33 step counts
    opt = fuse(torch.optim.Adam([p for _, p in named], lr=0.1))
    for i, (_, p) in enumerate(named):
        opt.state[p].update(step=torch.tensor(float(i)), exp_avg=torch.zeros(3), exp_avg_sq=torch.zeros(3))
    opt.step()
    assert recorder == [] and [int(opt.state[p]["step"]) for _, p in named] == list(range(1, 34))


def test_kernel_groups_and_chunk_rows_everything_present(recorder):
    from vbg import ops
    from vbg.optim import fuse
    named, letters, group = homed()
    opt = fuse(torch.optim.SGD(two_groups(named, letters, lr=0.5, momentum=0.0, maximize=True), lr=0.1, momentum=0.9, nesterov=True, weight_decay=0.01),
               seg_chunk=CHUNK)
    opt.step()
    name, (p, g, mom, table, hp, gs) = recorder[0]
    assert name == "sgd_step_seg_opt" and p is group.pflat and g is group.gflat and gs == 1.0 and mom.shape == p.shape
    F = ops.SGD_FIRST
    # (group B inherits nesterov from the defaults, as in torch, where it means nothing without momentum; momentum 0 is never "first")
    assert hp == [(0.1, 0.9, 0.0, 0.01, ops.SGD_NESTEROV | F), (0.5, 0.0, 0.0, 0.01, ops.SGD_NESTEROV | ops.SGD_MAXIMIZE)]
    assert (table.n, table.ngroups, table.numel) == (77, 2, TOTAL)
    assert np.array_equal(opt._vbg_fused.rows, expected_chunks())                    # group A -> 0, group B -> 1: the rows of RUNS
    opt.param_groups[0]["lr"] = 0.05                                                 # read on every call
    opt.step()
    assert recorder[1][1][3] is table and len(opt._vbg_fused.tables) == 1            # built once
    assert recorder[1][1][4] == [(0.05, 0.9, 0.0, 0.01, ops.SGD_NESTEROV), (0.5, 0.0, 0.0, 0.01, ops.SGD_NESTEROV | ops.SGD_MAXIMIZE)]


def test_absent_parameters_have_no_rows_and_tables_are_cached(recorder):
    from vbg import ops
    from vbg.optim import fuse
    named, letters, group = homed()
    by = dict(named)
    opt = fuse(torch.optim.AdamW(two_groups(named, letters, weight_decay=0.0, amsgrad=True), lr=1e-3), seg_chunk=CHUNK)
    opt.step()
    full = recorder[0][1][5]
    assert recorder[0][0] == "adam_step_seg_opt" and np.array_equal(opt._vbg_fused.rows, expected_chunks())
    assert recorder[0][1][4] is not None and recorder[0][1][4].shape == group.pflat.shape          # vmax: group B has amsgrad
    assert recorder[0][1][6] == [(1e-3, 0.9, 0.999, 1e-8, 0.01, 1, 0), (1e-3, 0.9, 0.999, 1e-8, 0.0, 1, ops.ADAM_AMSGRAD)]
    by["head.bias"].grad = None                                                      # group B, slot [8, 24)
    by["mid.weight"].grad = None                                                     # group A, slot [216, 408): splits the merged A run
    opt.step()
    # present: head.scale (A, step 2), head.weight (A), mid.LayerNorm.weight (B), stem.weight (A) -- param groups are walked in order,
    # A first, so (A, 2) is kernel group 0 and (B, 2) kernel group 1
    runs = [(0, 8, 0), (24, 192, 0), (408, 8, 1), (416, 4296, 0)]
    want = np.array([(s, min(CHUNK, a + n - s), k) for a, n, k in runs for s in range(a, a + n, CHUNK)], dtype=np.int64)
    rows = opt._vbg_fused.rows
    assert np.array_equal(rows, want) and len(rows) == 1 + 3 + 1 + 68
    covered = np.zeros(TOTAL, dtype=bool)
    for s, n, _ in rows:
        covered[s:s + n] = True
    assert not covered[8:24].any() and not covered[216:408].any() and not covered[4712:].any()
    partial = recorder[1][1][5]
    assert partial is not full and partial.n == len(want)
    assert [h[5] for h in recorder[1][1][6]] == [2, 2]
    opt.step()                                                                       # the same present set again: the cached table
    assert recorder[2][1][5] is partial and [h[5] for h in recorder[2][1][6]] == [3, 3] and len(opt._vbg_fused.tables) == 2
    # the two come back: four kernel groups in order of first appearance -- (A, 4), (A, 2), (B, 4), (B, 2) -- over the full layout
    group.zero_grad()
    opt.step()
    hp = recorder[3][1][6]
    assert [(h[5], h[6]) for h in hp] == [(4, 0), (2, 0), (4, ops.ADAM_AMSGRAD), (2, ops.ADAM_AMSGRAD)]
    # (registration order is the reverse of LAYOUT: group A walks stem, mid, head.weight, head.scale; group B mid.LayerNorm, head.bias)
    rows = opt._vbg_fused.rows
    assert {tuple(r) for r in rows if r[0] < 416} == {(0, 8, 0), (8, 16, 3), (408, 8, 2)} | {(s, 64, 0) for s in range(24, 216, 64)} | {(s, 64, 1) for s in range(216, 408, 64)}
    assert [int(opt.state[by[n]]["step"]) for n in NAMES] == [4, 2, 4, 2, 4, 4]
    opt.step()
    assert len(opt._vbg_fused.tables) == 3 and [int(opt.state[by[n]]["step"]) for n in NAMES] == [5, 3, 5, 3, 5, 5]


@pytest.mark.parametrize("case", ["sgd_momentum0", "sgd_momentum", "adam_amsgrad", "adamw_plain", "mixed_amsgrad"])
def test_state_keys_equal_a_torch_twin(recorder, case):
    cls, kw, b = {"sgd_momentum0": (torch.optim.SGD, dict(lr=0.1), {}),
                  "sgd_momentum": (torch.optim.SGD, dict(lr=0.1, momentum=0.9), {"momentum": 0.0}),
                  "adam_amsgrad": (torch.optim.Adam, dict(lr=0.1, amsgrad=True), {}),
                  "adamw_plain": (torch.optim.AdamW, dict(lr=0.1), {}),
                  "mixed_amsgrad": (torch.optim.AdamW, dict(lr=0.1), {"amsgrad": True})}[case]
    named, letters, group = homed()
    opt, plain, twin = _plain_and_fused(cls, named, letters, **kw)
    for o in (opt, plain):
        o.param_groups[1].update(b)
    dict(named)["head.weight"].grad = None                                           # never gets a gradient: torch keeps no state for it
    dict(twin)["head.weight"].grad = None
    for _ in range(2):
        opt.step()
        plain.step()
    assert len(recorder) == 2
    assert len(opt.state) == len(plain.state)
    for (n, p), (_, q) in zip(named, twin):
        assert (p in opt.state) == (q in plain.state), n
        if q not in plain.state:
            continue
        a, t = opt.state[p], plain.state[q]
        assert list(a) == list(t), (n, list(a), list(t))
        for k in t:
            assert (a[k] is None) == (t[k] is None) and a[k].shape == t[k].shape and a[k].dtype == t[k].dtype and a[k].stride() == t[k].stride(), (n, k)
        if "step" in t:
            assert torch.equal(a["step"], t["step"]) and a["step"].device == t["step"].device
    sd, sd_t = opt.state_dict(), plain.state_dict()
    assert sd["param_groups"] == sd_t["param_groups"] and sorted(sd["state"]) == sorted(sd_t["state"])
    flats = {id(f.untyped_storage()) for f in opt._vbg_fused.flat.values()}
    for st in sd["state"].values():                                                  # clones: a checkpoint does not drag the flat storage along
        for v in st.values():
            assert v.untyped_storage().nbytes() <= 4 * 4296 and v._base is None
    plain.load_state_dict(sd)                                                        # and torch takes it
    opt.load_state_dict(sd_t)
    opt.step()                                                                       # loaded tensors are copied in and re-pointed
    for n, p in named:
        for k, v in opt.state.get(p, {}).items():
            if k != "step":
                assert v._base is opt._vbg_fused.flat[k] or v._base is not None and v._base.data_ptr() == opt._vbg_fused.flat[k].data_ptr(), (n, k)
    assert bool(flats) == (case != "sgd_momentum0")                                 # momentum 0: no buffer is ever allocated


def test_argument_errors_of_the_opt_entries():
    from vbg import lib as L
    sgd, adam = L.lib.vbg_sgd_step_seg_opt, L.lib.vbg_adam_step_seg_opt
    hs, ha = (L.SgdGroupOpt * 33)(), (L.AdamGroupOpt * 33)()
    for h in ha:
        h.step = 1
    for ng in (1, 32):
        assert sgd(None, None, None, None, 0, hs, ng, 1.0, None) == 0                # nchunks == 0 is a no-op
        assert adam(None, None, None, None, None, None, 0, ha, ng, 1.0, None) == 0
    for ng in (0, 33, -1):
        assert sgd(None, None, None, None, 0, hs, ng, 1.0, None) == -1
        assert adam(None, None, None, None, None, None, 0, ha, ng, 1.0, None) == -1
    assert sgd(None, None, None, None, -1, hs, 1, 1.0, None) == -1
    assert adam(None, None, None, None, None, None, -1, ha, 1, 1.0, None) == -1
    assert sgd(None, None, None, None, 1, hs, 1, 1.0, None) == -1                    # null operands with work to do
    assert adam(None, None, None, None, None, None, 1, ha, 1, 1.0, None) == -1
    # everything but the optional buffer in place (host memory: these calls must return before any launch)
    buf = (C.c_float * 64)()
    a = C.cast(C.addressof(buf) + (-C.addressof(buf)) % 16, C.c_void_p)
    hs[0].momentum = 0.9
    assert sgd(a, a, None, a, 1, hs, 1, 1.0, None) == -1                             # a group has momentum, no momentum buffer
    ha[1].flags = L.ADAM_AMSGRAD
    assert adam(a, a, a, a, None, a, 1, ha, 2, 1.0, None) == -1                      # amsgrad flag with vmax NULL
    ha[1].flags = 0
    ha[1].step = 0
    assert adam(a, a, a, a, a, a, 1, ha, 2, 1.0, None) == -1                         # every group's step >= 1
    assert adam(a, a, a, a, a, None, 1, ha, 1, 1.0, None) == -1                      # no table
    assert (L.SGD_NESTEROV, L.SGD_MAXIMIZE, L.SGD_FIRST, L.ADAM_AMSGRAD, L.ADAM_MAXIMIZE, L.ADAM_COUPLED) == (1, 2, 4, 1, 2, 4)


def test_ops_wrappers_check_the_buffers():
    from vbg import ops
    ok = ops.chunk_table([(0, 8, 0), (8, 64, 1)], 2, 72, "cpu")
    z = lambda n=72: torch.zeros(n)
    with pytest.raises(ValueError):                                                  # hyper-parameter sets must match the table's groups
        ops.sgd_step_seg_opt(z(), z(), z(), ok, [(0.1, 0.9, 0.0, 0.0, 0)])
    with pytest.raises(ValueError):                                                  # buffers shorter than the table's range
        ops.sgd_step_seg_opt(z(), z(), z(64), ok, [(0.1, 0.9, 0.0, 0.0, 0)] * 2)
    with pytest.raises(ValueError):                                                  # momentum without a buffer
        ops.sgd_step_seg_opt(z(), z(), None, ok, [(0.1, 0.0, 0.0, 0.0, 0), (0.1, 0.9, 0.0, 0.0, 0)])
    with pytest.raises(ValueError):
        ops.adam_step_seg_opt(z(), z(), z(), z(), None, ok, [(1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0)])
    with pytest.raises(ValueError):
        ops.adam_step_seg_opt(z(), z(), z(), z(), z(64), ok, [(1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1)] * 2)
    with pytest.raises(ValueError):                                                  # amsgrad without a buffer
        ops.adam_step_seg_opt(z(), z(), z(), z(), None, ok, [(1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0), (1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1)])
    with pytest.raises(ValueError):
        ops.adam_step_seg_opt(z(), z().double(), z(), z(), None, ok, [(1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0)] * 2)


def test_opt_struct_layouts_against_the_c_compiler(tmp_path):
    from vbg.lib import AdamGroupOpt, SgdGroupOpt
    assert (C.sizeof(SgdGroupOpt), C.sizeof(AdamGroupOpt)) == (20, 28)
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    assert cc is not None, "no C compiler"
    pairs = (("vbg_sgd_group_opt", SgdGroupOpt), ("vbg_adam_group_opt", AdamGroupOpt))
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "vbg.h"', 'int main(void) {']
    for st, cls in pairs:
        src.append(f'printf("{st} sizeof %zu\\n", sizeof({st}));')
        for name, _ in cls._fields_:
            src.append(f'printf("{st} {name} %zu\\n", offsetof({st}, {name}));')
    src += ['return 0; }']
    cfile = tmp_path / "sz.c"
    cfile.write_text("\n".join(src))
    exe = str(tmp_path / "sz")
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(cfile), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {(a, b): int(c) for a, b, c in (ln.split() for ln in out if ln)}
    for st, cls in pairs:
        assert got[(st, "sizeof")] == C.sizeof(cls)
        for name, _ in cls._fields_:
            assert got[(st, name)] == getattr(cls, name).offset, (st, name)
