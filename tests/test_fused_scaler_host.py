"""vbg.optim.fuse_scaler, the host side (no GPU, no launch; the library itself must load): the argument checks of
vbg_grad_unscale_check_seg / vbg_grad_sumsq_seg_inf, which return before any launch, and a real torch.amp.GradScaler("cpu") with the
ops wrappers replaced by recorders (the `recorder` pattern of tests/test_stock_optim_host.py and tests/test_clip_step_host.py) -- the
class switch, one check per `scaler.step` under the amp_scaling protocol and none after `clip_in_step(scaler=...)`, the real inverse
scale on the generic route, the fallbacks to torch's own pass, flags that do not outlive `update()` or their gradients, and a plain
scaler left on the call sequence it had."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

from test_clip_step_host import STEP_WRAPPERS, _flat_pair, _stock, names
from test_optim_groups_host import CHUNK, END, TOTAL, expected_chunks, six_params
from test_stock_optim_host import two_groups

NEW_WRAPPERS = ("grad_unscale_check_seg", "grad_sumsq_seg_inf")


@pytest.fixture
def rec(monkeypatch):
    """every optimizer wrapper of vbg.ops and the two new ones record instead of launching (the new ones with the values their scalars
    held at the call); the finish returns a host tensor (total 4, coefficient 0.5)"""
    from vbg import ops
    calls = []
    for name in STEP_WRAPPERS:
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: calls.append((_n, a, k)))
    monkeypatch.setattr(ops, "grad_unscale_check_seg",
                        lambda g, t, inv, flag: calls.append(("grad_unscale_check_seg", (g, t, inv, flag), {"inv": inv.clone(), "flag": flag.clone()})))
    monkeypatch.setattr(ops, "grad_sumsq_seg_inf",
                        lambda g, t, part, flag: calls.append(("grad_sumsq_seg_inf", (g, t, part, flag), {"flag": flag.clone()})))

    def finish(partials, n, max_norm, norm_scale=1.0, grad_scale=None, out=None):
        calls.append(("clip_coef", (partials, n, max_norm, norm_scale, grad_scale), {}))
        return torch.tensor([4.0, 0.5])

    monkeypatch.setattr(ops, "clip_coef", finish)
    return calls


def _scaler(init_scale=1024.0, fused=True):
    from vbg.optim import fuse_scaler
    s = torch.amp.GradScaler("cpu", init_scale=init_scale)
    s.scale(torch.zeros(()))          # (the scale tensor comes into being at the first scale() call)
    return fuse_scaler(s) if fused else s


def _checks(calls):
    return [c for c in calls if c[0] == "grad_unscale_check_seg"]


def _covered(table):
    m = np.zeros(TOTAL, dtype=bool)
    for s, n, _ in table.chunk_rows:
        assert not m[s:s + n].any()
        m[s:s + n] = True
    return m


# ------------------------------------------------------------------------------------------
# the library without a GPU
# ------------------------------------------------------------------------------------------
def test_argument_errors_of_the_new_entries():
    from vbg import lib as L
    chk, norm = L.lib.vbg_grad_unscale_check_seg, L.lib.vbg_grad_sumsq_seg_inf
    buf = (C.c_float * 64)()
    a = C.cast(C.addressof(buf) + (-C.addressof(buf)) % 16, C.c_void_p)
    odd, off4 = C.c_void_p(a.value + 2), C.c_void_p(a.value + 4)
    # nchunks == 0 is a no-op, with nothing but the scalars in place
    assert chk(None, None, 0, a, a, None) == 0 and norm(None, None, 0, None, a, None) == 0
    assert chk(a, a, 0, off4, off4, None) == 0                                       # (scalars: 4-byte alignment is enough)
    # the scalars are required ...
    assert chk(a, a, 1, None, a, None) == -1 and chk(a, a, 1, a, None, None) == -1 and norm(a, a, 1, a, None, None) == -1
    assert chk(None, None, 0, None, a, None) == -1 and chk(None, None, 0, a, None, None) == -1 and norm(None, None, 0, None, None, None) == -1
    # ... and 4-byte aligned
    assert chk(a, a, 1, odd, a, None) == -1 and chk(a, a, 1, a, odd, None) == -1 and norm(a, a, 1, a, odd, None) == -1
    # g, the table, the partials; 16-byte alignment of g and the table
    assert chk(None, a, 1, a, a, None) == -1 and chk(a, None, 1, a, a, None) == -1
    assert norm(None, a, 1, a, a, None) == -1 and norm(a, None, 1, a, a, None) == -1 and norm(a, a, 1, None, a, None) == -1
    assert chk(off4, a, 1, a, a, None) == -1 and chk(a, off4, 1, a, a, None) == -1
    assert norm(off4, a, 1, a, a, None) == -1 and norm(a, off4, 1, a, a, None) == -1 and norm(a, a, 1, odd, a, None) == -1
    assert chk(a, a, -1, a, a, None) == -1 and norm(a, a, -1, a, a, None) == -1
    # the entry next to them is as it was
    assert L.lib.vbg_grad_sumsq_seg(None, None, 0, None, None) == 0 and L.lib.vbg_grad_sumsq_seg(a, a, 1, None, None) == -1


def test_ops_wrappers_check_the_scalars_and_buffers():
    from vbg import ops
    ok = ops.chunk_table([(0, 8, 0), (8, 64, 0)], 1, 72, "cpu")
    z = lambda n=72: torch.zeros(n)
    one = torch.ones(1)
    for bad in (None, torch.ones(2), torch.ones(1, dtype=torch.float64), 1.0):
        with pytest.raises(ValueError, match="inv_scale"):
            ops.grad_unscale_check_seg(z(), ok, bad, one)
        with pytest.raises(ValueError, match="found_inf"):
            ops.grad_unscale_check_seg(z(), ok, one, bad)
        with pytest.raises(ValueError, match="found_inf"):
            ops.grad_sumsq_seg_inf(z(), ok, z(2), bad)
    for bad in (z(64), z().double(), z(144)[::2]):                                   # shorter than the table's range, fp64, strided
        with pytest.raises(ValueError):
            ops.grad_unscale_check_seg(bad, ok, one, one)
        with pytest.raises(ValueError):
            ops.grad_sumsq_seg_inf(bad, ok, z(2), one)
    with pytest.raises(ValueError):                                                  # one partial per row
        ops.grad_sumsq_seg_inf(z(), ok, z(1), one)


# ------------------------------------------------------------------------------------------
# the class switch
# ------------------------------------------------------------------------------------------
def test_fuse_scaler_keeps_the_object_and_refuses_other_classes():
    from vbg.optim import fuse_scaler
    s = torch.amp.GradScaler("cpu", init_scale=512.0, growth_interval=7)
    before = s.state_dict()
    got = fuse_scaler(s)
    assert got is s and isinstance(s, torch.amp.GradScaler) and type(s) is not torch.amp.GradScaler
    assert s.state_dict() == before and s.get_scale() == 512.0 and s.get_growth_interval() == 7
    fs = s._vbg_fused
    assert (fs.launches, fs.reused, fs.fallbacks, fs.last_fallback) == (0, 0, 0, None)
    for name in ("scale", "step", "unscale_", "update", "state_dict", "load_state_dict"):          # torch's own
        assert getattr(type(s), name) is getattr(torch.amp.GradScaler, name)
    with pytest.raises(ValueError, match="exactly"):                                 # a fused scaler is no longer exactly torch's class
        fuse_scaler(s)

    class MyScaler(torch.amp.GradScaler):
        pass

    for bad in (MyScaler("cpu"), object(), torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1)):
        with pytest.raises(ValueError, match="exactly"):
            fuse_scaler(bad)
    with warnings.catch_warnings():                                                  # the class the reference constructs
        warnings.simplefilter("ignore")
        old = torch.cuda.amp.GradScaler(enabled=False)
    assert fuse_scaler(old) is old and isinstance(old, torch.cuda.amp.GradScaler) and type(old) is not torch.cuda.amp.GradScaler


# ------------------------------------------------------------------------------------------
# the protocol route: fuse(amp_scaling=True)
# ------------------------------------------------------------------------------------------
def test_protocol_route_one_check_per_step_and_none_after_clip_in_step(rec):
    from vbg.optim import clip_in_step
    named, group, opt = _stock(torch.optim.SGD, amp=True, lr=0.1, momentum=0.9)
    scaler = _scaler()
    fs = scaler._vbg_fused
    scaler.step(opt)
    assert names(rec) == ["grad_unscale_check_seg", "sgd_step_seg_amp"]
    _, (g, table, inv, flag), at = rec[0]
    assert g is group.gflat and float(at["inv"]) == 1.0 and float(at["flag"]) == 0.0 and flag.numel() == 1 and flag.dtype == torch.float32
    m = _covered(table)
    want = np.zeros(TOTAL, dtype=bool)
    for s, n, _ in expected_chunks():
        want[s:s + n] = True
    assert np.array_equal(m, want) and m[:END].all() and not m[END:].any()
    assert np.array_equal(table.chunk_rows, np.array([(s, min(CHUNK, END - s), 0) for s in range(0, END, CHUNK)], dtype=np.int64))
    assert table is opt._vbg_norm_table()[1]                                         # the table clip_in_step uses
    assert float(rec[1][1][6]) == 0.0 and float(rec[1][1][5]) == 1024.0              # the step got the flag's value and the scale
    assert (fs.launches, fs.reused, fs.fallbacks) == (1, 0, 0)
    scaler.update()
    # parameters without a gradient are in no row
    by = dict(named)
    by["head.bias"].grad = None                                                      # slot [8, 24)
    by["mid.weight"].grad = None                                                     # slot [216, 408)
    del rec[:]
    first_flag = flag
    scaler.step(opt)
    _, (g, table2, inv, flag), at = rec[0]
    assert flag is not first_flag and float(at["flag"]) == 0.0                       # a fresh flag for every check
    runs = [(0, 8), (24, 192), (408, 8 + 4296)]
    assert np.array_equal(table2.chunk_rows, np.array([(s, min(CHUNK, a + n - s), 0) for a, n in runs for s in range(a, a + n, CHUNK)], dtype=np.int64))
    m = _covered(table2)
    assert not m[8:24].any() and not m[216:408].any() and not m[END:].any() and m[0:8].all() and m[24:216].all() and m[408:END].all()
    scaler.update()
    # after clip_in_step(scaler=...): the norm launch carries the check, scaler.step launches none
    del rec[:]
    clip_in_step([opt], 1.0, scaler=scaler)
    assert names(rec) == ["grad_sumsq_seg_inf", "clip_coef"]
    _, (g, t3, part, cflag), at = rec[0]
    assert g is group.gflat and t3 is table2 and part.numel() == t3.n and cflag.numel() == 1 and float(at["flag"]) == 0.0
    assert rec[1][1][4] is scaler._scale
    scaler.step(opt)
    assert names(rec)[2:] == ["sgd_step_seg_clip"] and _checks(rec) == []
    assert (fs.launches, fs.reused, fs.fallbacks) == (2, 1, 0)
    assert float(rec[2][1][6]) == 0.0 and rec[2][1][7] is not None
    assert scaler._per_optimizer_states[id(opt)]["found_inf_per_device"] == {cflag.device: cflag}
    scaler.update()
    assert scaler.get_scale() == 1024.0


def test_a_flag_set_by_the_norm_pass_reaches_the_step_and_the_scale(rec, monkeypatch):
    """the recorder plays a norm launch that found an inf: the step is handed found_inf 1, update() backs the scale off"""
    from vbg import ops
    from vbg.optim import clip_in_step
    named, group, opt = _stock(torch.optim.SGD, amp=True, lr=0.1, momentum=0.9)
    monkeypatch.setattr(ops, "grad_sumsq_seg_inf", lambda g, t, part, flag: (rec.append(("grad_sumsq_seg_inf", (g, t, part, flag), {})), flag.fill_(1.0)))
    scaler = _scaler()
    clip_in_step([opt], 1.0, scaler=scaler)
    scaler.step(opt)
    assert names(rec) == ["grad_sumsq_seg_inf", "clip_coef", "sgd_step_seg_clip"] and float(rec[2][1][6]) == 1.0
    scaler.update()
    assert scaler.get_scale() == 512.0 and scaler._vbg_fused.reused == 1


def test_flags_are_per_optimizer_and_do_not_outlive_update_or_their_gradients(rec):
    from vbg.optim import _CLIP_FLAG, clip_in_step, fuse
    named, group, a = _stock(torch.optim.SGD, amp=True, lr=0.1, momentum=0.9)
    named_b, group_b, b = _stock(torch.optim.AdamW, amp=True, lr=1e-3)
    scaler = _scaler()
    fs = scaler._vbg_fused
    clip_in_step([a, b], 1.0, scaler=scaler)
    assert names(rec) == ["grad_sumsq_seg_inf", "grad_sumsq_seg_inf", "clip_coef"]
    fa, fb = rec[0][1][3], rec[1][1][3]
    assert rec[0][1][0] is group.gflat and rec[1][1][0] is group_b.gflat
    assert fa.data_ptr() != fb.data_ptr() and fa.untyped_storage().data_ptr() == fb.untyped_storage().data_ptr()          # one torch.zeros
    assert scaler._per_optimizer_states[id(a)][_CLIP_FLAG][0] is fa and scaler._per_optimizer_states[id(b)][_CLIP_FLAG][0] is fb
    scaler.step(a)                                                                   # ... only a steps in this iteration
    assert fs.reused == 1 and _checks(rec) == []
    scaler.update()                                                                  # b's flag goes with GradScaler's own per-optimizer record
    assert _CLIP_FLAG not in scaler._per_optimizer_states[id(b)] and b._vbg_clip is not None
    del rec[:]
    scaler.step(b)
    assert names(rec) == ["grad_unscale_check_seg", "adam_step_seg_clip"] and (fs.launches, fs.reused) == (1, 1)
    scaler.step(a)                                                                   # a second step without a new clip_in_step: a check again
    assert names(rec)[2:] == ["grad_unscale_check_seg", "sgd_step_seg_amp"] and (fs.launches, fs.reused) == (2, 1)
    scaler.update()
    # zero_grad() between clip_in_step and the step: the coefficient is dropped, and the flag speaks for gradients that are gone
    del rec[:]
    clip_in_step([a], 1.0, scaler=scaler)
    a.zero_grad(set_to_none=False)
    assert a._vbg_clip is None
    scaler.step(a)
    assert names(rec) == ["grad_sumsq_seg_inf", "clip_coef", "grad_unscale_check_seg", "sgd_step_seg_amp"] and (fs.launches, fs.reused) == (3, 1)
    assert fs.fallbacks == 0


# ------------------------------------------------------------------------------------------
# the generic route: unscale_ with the real inverse
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1024.0, 1000.0])
def test_generic_route_unscale_with_torchs_inverse(rec, scale):
    named, group, opt = _stock(torch.optim.SGD, lr=0.1, momentum=0.9)                # fused without amp_scaling
    scaler = _scaler(scale)
    g0 = group.gflat.clone()
    scaler.unscale_(opt)
    assert names(rec) == ["grad_unscale_check_seg"]
    _, (g, table, inv, flag), at = rec[0]
    want = scaler._scale.double().reciprocal().float()
    assert g is group.gflat and at["inv"].view(torch.int32).item() == want.view(torch.int32).item() and float(at["flag"]) == 0.0
    assert torch.equal(group.gflat, g0)                                              # (the recorder launched nothing, and torch's pass did not run)
    assert scaler._per_optimizer_states[id(opt)]["found_inf_per_device"] == {flag.device: flag}
    scaler.step(opt)                                                                 # stage UNSCALED: no second pass
    assert names(rec) == ["grad_unscale_check_seg", "sgd_step_seg_opt"]
    scaler.update()
    del rec[:]
    scaler.step(opt)                                                                 # stage READY: step() runs unscale_ itself
    assert names(rec) == ["grad_unscale_check_seg", "sgd_step_seg_opt"] and float(rec[0][2]["inv"]) == float(want)
    assert (scaler._vbg_fused.launches, scaler._vbg_fused.fallbacks) == (2, 0)


def test_fused_sgd_and_adamw_on_the_generic_route(rec):
    sgd, adam = _flat_pair(True)
    plain_sgd, plain_adam = _flat_pair(False)
    scaler = _scaler(1000.0)
    for o in (sgd, adam, plain_sgd, plain_adam):
        scaler.unscale_(o)
    assert names(rec) == ["grad_unscale_check_seg"] * 4
    for (_, (g, table, inv, flag), at), o in zip(rec, (sgd, adam, plain_sgd, plain_adam)):
        assert g is o.group.gflat and table is o._clip_table() and float(at["inv"]) == float(torch.tensor(1000.0).double().reciprocal().float())
    assert rec[0][1][1] is sgd.table and rec[2][1][1].n == 2                         # the param groups' table / one group over the layout
    flags = [c[1][3] for c in rec]
    assert len({f.data_ptr() for f in flags}) == 4                                   # update() adds them into the first: never shared
    for o in (sgd, adam, plain_sgd, plain_adam):
        scaler.step(o)
    assert names(rec)[4:] == ["sgd_step_seg", "adamw_step_seg", "sgd_step", "adamw_step"]
    scaler.update()
    # a parameter whose .grad went to None keeps its zeroed slot: still one launch; a replaced .grad is torch's pass
    sgd.group.params[0].grad = None
    scaler.unscale_(sgd)
    assert scaler._vbg_fused.fallbacks == 0
    p = adam.group.params[1]
    p.grad = p.grad.clone()
    scaler.unscale_(adam)
    assert scaler._vbg_fused.fallbacks == 1 and "gradient view" in scaler._vbg_fused.last_fallback


# ------------------------------------------------------------------------------------------
# fallbacks to torch's own pass
# ------------------------------------------------------------------------------------------
def test_fallbacks_run_torchs_pass_and_are_counted(rec):
    from vbg.optim import FlatGroup, fuse
    scaler = _scaler(1024.0)
    fs = scaler._vbg_fused
    # (a) a fuse()d optimizer whose parameters are not homed
    named, letters = six_params("cpu")
    for _, p in named:
        p.grad = torch.full_like(p, 2048.0)
    opt = fuse(torch.optim.SGD(two_groups(named, letters), lr=0.1), seg_chunk=CHUNK)
    scaler.unscale_(opt)
    assert _checks(rec) == [] and fs.fallbacks == 1 and "homed" in fs.last_fallback
    assert all(torch.equal(p.grad, torch.full_like(p, 2.0)) for _, p in named)       # torch's pass did the unscale
    assert float(next(iter(scaler._per_optimizer_states[id(opt)]["found_inf_per_device"].values()))) == 0.0
    scaler.step(opt)
    scaler.update()
    # (b) homed, one .grad replaced
    group = FlatGroup(named, "cpu")
    group.gflat.fill_(1024.0)
    p0 = named[0][1]
    p0.grad = torch.full_like(p0, float("inf"))
    scaler.unscale_(opt)
    assert _checks(rec) == [] and fs.fallbacks == 2 and "gradient view" in fs.last_fallback
    assert float(next(iter(scaler._per_optimizer_states[id(opt)]["found_inf_per_device"].values()))) == 1.0          # ... and found the inf
    assert torch.equal(named[1][1].grad, torch.ones_like(named[1][1]))
    scaler.step(opt)
    scaler.update()
    assert scaler.get_scale() == 512.0
    # (c) no gradient at all
    for _, p in named:
        p.grad = None
    scaler._unscale_grads_(opt, torch.ones(()), torch.zeros(()), True)
    assert fs.fallbacks == 3 and "no parameter has a gradient" in fs.last_fallback
    # (d) a plain torch optimizer
    q = torch.nn.Parameter(torch.zeros(3))
    q.grad = torch.full((3,), 512.0)
    plain = torch.optim.SGD([q], lr=0.1)
    scaler.unscale_(plain)
    assert fs.fallbacks == 4 and "not a fuse()d" in fs.last_fallback and torch.equal(q.grad, torch.ones(3))
    # (e) scalars that are not one fp32 element on the buffers' device: torch's pass gets them (and refuses them itself)
    group.zero_grad()
    with pytest.raises(Exception):
        scaler._unscale_grads_(opt, torch.ones(()), torch.zeros(2), True)
    assert fs.fallbacks == 5 and "one fp32 element" in fs.last_fallback
    assert _checks(rec) == [] and fs.launches == 0
    scaler._unscale_grads_(opt, torch.ones(()), torch.zeros(()), True)               # ... and with proper ones it is the launch
    assert len(_checks(rec)) == 1 and (fs.launches, fs.fallbacks) == (1, 5)


# ------------------------------------------------------------------------------------------
# nobody called fuse_scaler: the call sequence of before
# ------------------------------------------------------------------------------------------
def test_a_plain_scaler_keeps_the_plain_norm_wrapper(rec):
    from vbg.optim import _CLIP_FLAG, clip_in_step
    named, group, opt = _stock(torch.optim.SGD, amp=True, lr=0.1, momentum=0.9)
    scaler = _scaler(fused=False)
    clip_in_step([opt], 1.0, scaler=scaler)
    assert names(rec) == ["grad_sumsq_seg", "clip_coef"] and len(rec[0][1]) == 3
    assert _CLIP_FLAG not in scaler._per_optimizer_states[id(opt)]
    scaler.step(opt)                                                                 # torch's own check (on the CPU), then the clipping step
    assert names(rec)[2:] == ["sgd_step_seg_clip"]
    scaler.update()
    # a fused scaler that is disabled, and no scaler at all
    from vbg.optim import fuse_scaler
    off = fuse_scaler(torch.amp.GradScaler("cpu", enabled=False))
    for s in (off, None):
        del rec[:]
        clip_in_step([opt], 1.0, scaler=s)
        assert names(rec) == ["grad_sumsq_seg", "clip_coef"]
        opt.step()
