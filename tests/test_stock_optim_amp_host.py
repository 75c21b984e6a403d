"""vbg.optim.fuse(optimizer, amp_scaling=True), the host side (no GPU, no launch: the four stock entries are replaced by recorders, the
two scalars of torch.amp.GradScaler's protocol are CPU tensors): the flag, which entry a step goes to, the deferred reconciliation of
`optimizer.state` after a step the device would have skipped -- against a torch twin whose step was not called --, the fallbacks
under the protocol, and the argument checks of vbg_sgd_step_seg_amp / vbg_adam_step_seg_amp.  Six-parameter LAYOUT and recorder
pattern of tests/test_stock_optim_host.py."""
import ctypes as C
import inspect

import pytest
import torch

from test_optim_groups_host import CHUNK, six_params
from test_stock_optim_host import NAMES, homed, two_groups

ENTRIES = ("sgd_step_seg_opt", "adam_step_seg_opt", "sgd_step_seg_amp", "adam_step_seg_amp")


@pytest.fixture
def recorder(monkeypatch):
    """the four stock entries of vbg.ops record their arguments instead of launching"""
    from vbg import ops
    calls = []
    for name in ENTRIES:
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: calls.append((_n, a)))
    return calls


def scaled_step(opt, found_inf, scale=1024.0):
    """what GradScaler.step does to an optimizer that declares _step_supports_amp_scaling: the two attributes for the length of the call.
    scale None: the caller ran scaler.unscale_ (stage UNSCALED), grad_scale is None"""
    opt.grad_scale = None if scale is None else torch.tensor(float(scale))
    opt.found_inf = torch.tensor(float(found_inf))
    try:
        return opt.step()
    finally:
        del opt.grad_scale
        del opt.found_inf


def amp_pair(cls, seed=0, **kw):
    """_plain_and_fused with the option on: (fused, plain torch twin, named, twin, group)"""
    from vbg.optim import fuse
    named, letters, group = homed(seed)
    twin = [(n, torch.nn.Parameter(p.detach().clone())) for n, p in named]
    for (_, p), (_, q) in zip(named, twin):
        q.grad = p.grad.detach().clone()
    opt = fuse(cls(two_groups(named, letters), **kw), seg_chunk=CHUNK, amp_scaling=True)
    return opt, cls(two_groups(twin, letters), **kw), named, twin, group


def test_the_flag_is_per_instance_and_step_keeps_its_signature():
    from vbg.optim import FusedAdamW, FusedSGD, fuse
    named, letters, _ = homed()
    for cls in (torch.optim.SGD, torch.optim.Adam, torch.optim.AdamW):
        plain = fuse(cls(two_groups(named, letters), lr=0.1))
        assert not hasattr(plain, "_step_supports_amp_scaling") and plain._vbg_fused.amp is False
        opt = fuse(cls(two_groups(named, letters), lr=0.1), amp_scaling=True)
        assert opt._step_supports_amp_scaling is True and opt._vbg_fused.amp is True
        assert not hasattr(type(opt), "_step_supports_amp_scaling") and not hasattr(plain, "_step_supports_amp_scaling")
        for o in (plain, opt):                                                       # torch inspects the signature for a grad_scaler parameter
            assert "grad_scaler" not in inspect.signature(o.step).parameters
        assert (opt._vbg_fused.skipped, opt._vbg_fused.launches) == (0, 0)
    # the native classes keep a host float under the protocol's attribute name: they stay outside it
    for cls in (FusedSGD, FusedAdamW):
        assert not hasattr(cls, "_step_supports_amp_scaling") and "_step_supports_amp_scaling" in cls.__doc__


@pytest.mark.parametrize("cls", [torch.optim.SGD, torch.optim.AdamW])
def test_routing_follows_the_attributes(recorder, cls):
    opt, _, named, _, group = amp_pair(cls, lr=0.1)
    kind = "sgd" if cls is torch.optim.SGD else "adam"
    opt.step()                                                                       # no attributes: the parent's call, host scale 1.0 last
    name, a = recorder[-1]
    assert name == f"{kind}_step_seg_opt" and a[-1] == 1.0 and a[0] is group.pflat and a[1] is group.gflat
    parent_args = len(a)
    opt.grad_scale, opt.found_inf = torch.tensor(1024.0), torch.tensor(0.0)
    sc, fi = opt.grad_scale, opt.found_inf
    opt.step()
    del opt.grad_scale, opt.found_inf
    name, a = recorder[-1]
    assert name == f"{kind}_step_seg_amp" and a[-2] is sc and a[-1] is fi and len(a) == parent_args + 1
    hyper = (lambda hp: hp) if kind == "sgd" else (lambda hp: [h[:5] + h[6:] for h in hp])          # (Adam: without the step count)
    assert a[0] is group.pflat and a[1] is group.gflat and a[-4] is recorder[0][1][-3] and hyper(a[-3]) == hyper(recorder[0][1][-2])
    scaled_step(opt, 0, scale=None)                                                  # scaler.unscale_ ran: NULL scale
    name, a = recorder[-1]
    assert name == f"{kind}_step_seg_amp" and a[-2] is None and float(a[-1]) == 0.0
    opt.step()                                                                       # attributes deleted again: the plain entry
    assert recorder[-1][0] == f"{kind}_step_seg_opt" and recorder[-1][1][-1] == 1.0
    fs = opt._vbg_fused
    assert (fs.launches, fs.skipped, fs.fallbacks) == (4, 0, 0)
    # without the option the attributes mean nothing (GradScaler never sets them then)
    from vbg.optim import fuse
    named2, letters2, _ = homed(seed=3)
    off = fuse(cls(two_groups(named2, letters2), lr=0.1), seg_chunk=CHUNK)
    scaled_step(off, 1)
    assert recorder[-1][0] == f"{kind}_step_seg_opt" and off._vbg_fused.skipped == 0


def test_a_scalar_the_kernel_cannot_read_falls_back(recorder):
    opt, plain, named, twin, _ = amp_pair(torch.optim.SGD, lr=0.1)
    opt.grad_scale, opt.found_inf = torch.tensor(4.0, dtype=torch.float64), torch.tensor(0.0)
    opt.step()
    del opt.grad_scale, opt.found_inf
    for _, q in twin:
        q.grad.mul_(0.25)
    plain.step()
    assert recorder == [] and "grad_scale / found_inf" in opt._vbg_fused.last_fallback
    assert all(torch.equal(p, q) for (_, p), (_, q) in zip(named, twin))             # unscaled by the fallback, stepped by torch


def test_sgd_skip_on_the_very_first_step(recorder):
    from vbg import ops
    opt, plain, named, twin, group = amp_pair(torch.optim.SGD, lr=0.1, momentum=0.9)
    fs = opt._vbg_fused
    scaled_step(opt, 1)
    assert fs._pending is not None and all("momentum_buffer" in opt.state[p] for _, p in named)          # the host has not looked yet
    fs.reconcile()
    assert len(opt.state) == 0 and all("momentum_buffer" not in opt.state.get(p, {}) for _, p in named)
    assert (fs.launches, fs.skipped) == (1, 1) and fs._pending is None
    fs.reconcile()                                                                   # nothing pending: nothing happens
    assert fs.skipped == 1
    scaled_step(opt, 0)
    assert all(h[4] & ops.SGD_FIRST for h in recorder[-1][1][4])                      # first again: nobody's slot was written
    mom = recorder[-1][1][2]
    for n, p in named:
        st = opt.state[p]["momentum_buffer"]
        assert st.data_ptr() == mom.data_ptr() + 4 * p._vbg_flat[1] and st.shape == p.shape
    scaled_step(opt, 0)
    assert all(not h[4] & ops.SGD_FIRST for h in recorder[-1][1][4]) and (fs.launches, fs.skipped) == (3, 1)
    # a buffer key that torch left at None comes back as None
    opt2, _, named2, _, _ = amp_pair(torch.optim.SGD, seed=1, lr=0.1, momentum=0.9)
    p0 = named2[0][1]
    opt2.state[p0]["momentum_buffer"] = None
    scaled_step(opt2, 1)
    opt2._vbg_fused.reconcile()
    assert list(opt2.state) == [p0] and opt2.state[p0] == {"momentum_buffer": None}


def test_adamw_amsgrad_skip_on_the_first_step(recorder):
    opt, plain, named, twin, _ = amp_pair(torch.optim.AdamW, lr=1e-3, amsgrad=True)
    fs = opt._vbg_fused
    scaled_step(opt, 1)
    assert [h[5] for h in recorder[-1][1][6]] == [1, 1] and len(opt.state) == 6
    fs.reconcile()
    assert len(opt.state) == 0 and fs.skipped == 1
    scaled_step(opt, 0)
    assert [h[5] for h in recorder[-1][1][6]] == [1, 1]                               # the next recorded step is 1
    fs.reconcile()
    assert all(float(opt.state[p]["step"]) == 1.0 and list(opt.state[p]) == ["step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"] for _, p in named)


def _recorded_steps(recorder):
    return [sorted({h[5] for h in a[6]}) for name, a in recorder if name.startswith("adam")]


def test_skip_in_the_middle_and_two_in_a_row(recorder):
    opt, _, named, _, _ = amp_pair(torch.optim.AdamW, lr=1e-3)
    fs = opt._vbg_fused
    for inf in (0, 1, 0, 0):                                                         # skip at step 2 of 4
        scaled_step(opt, inf)
    assert _recorded_steps(recorder) == [[1], [2], [2], [3]]
    fs.reconcile()
    assert all(float(opt.state[p]["step"]) == 3.0 for _, p in named) and (fs.launches, fs.skipped) == (4, 1)
    del recorder[:]
    for inf in (1, 1, 0):                                                            # two skips in a row
        scaled_step(opt, inf)
    assert _recorded_steps(recorder) == [[4], [4], [4]]
    fs.reconcile()
    assert all(float(opt.state[p]["step"]) == 4.0 for _, p in named) and (fs.launches, fs.skipped, fs.fallbacks) == (7, 3, 0)


def test_an_absent_parameter_keeps_its_own_count_through_a_skip(recorder):
    opt, _, named, _, group = amp_pair(torch.optim.AdamW, lr=1e-3)
    by = dict(named)
    scaled_step(opt, 0)
    scaled_step(opt, 0)
    by["mid.weight"].grad = None                                                     # absent during the skipped step
    scaled_step(opt, 1)
    opt._vbg_fused.reconcile()
    assert [int(opt.state[by[n]]["step"]) for n in NAMES] == [2] * 6
    scaled_step(opt, 0)                                                              # still absent: its count stays behind
    group.zero_grad()
    scaled_step(opt, 1)                                                              # back, in a step that is skipped
    scaled_step(opt, 0)
    opt._vbg_fused.reconcile()
    assert [int(opt.state[by[n]]["step"]) for n in NAMES] == [4, 4, 4, 3, 4, 4]
    assert _recorded_steps(recorder) == [[1], [2], [3], [3], [3, 4], [3, 4]]
    assert (opt._vbg_fused.launches, opt._vbg_fused.skipped) == (6, 2)


@pytest.mark.parametrize("case", ["sgd_first", "sgd_later", "adam_first", "adam_later"])
def test_checkpoint_right_after_a_skipped_step(recorder, case):
    """state_dict() reconciles by itself: key for key and value for value the checkpoint of a torch twin whose step was not called"""
    cls, kw = (torch.optim.SGD, dict(lr=0.1, momentum=0.9, nesterov=True)) if case.startswith("sgd") else (torch.optim.Adam, dict(lr=1e-3, amsgrad=True))
    opt, plain, named, twin, _ = amp_pair(cls, **kw)
    if case.endswith("later"):
        scaled_step(opt, 0)
        plain.step()
        for (_, p), (_, q) in zip(named, twin):                                      # (the recorder moves nothing: give both sides the same state values)
            for k, v in plain.state[q].items():
                if k != "step":
                    opt.state[p][k].copy_(v)
    scaled_step(opt, 1)
    sd, sd_t = opt.state_dict(), plain.state_dict()
    assert opt._vbg_fused.skipped == 1 and opt._vbg_fused._pending is None
    assert sd["param_groups"] == sd_t["param_groups"] and sorted(sd["state"]) == sorted(sd_t["state"])
    assert bool(sd["state"]) == case.endswith("later")
    for i, st_t in sd_t["state"].items():
        assert list(sd["state"][i]) == list(st_t)
        for k, v in st_t.items():
            assert torch.equal(sd["state"][i][k], v) and sd["state"][i][k].dtype == v.dtype, (i, k)
    scaled_step(opt, 1)                                                              # load_state_dict reconciles first as well
    opt.load_state_dict(sd_t)
    assert opt._vbg_fused.skipped == 2 and opt._vbg_fused._pending is None
    assert sorted(opt.state_dict()["state"]) == sorted(sd_t["state"])


def test_fallback_under_the_protocol(recorder, monkeypatch):
    from vbg.optim import fuse
    seen = []
    real = torch.optim.SGD.step
    real = getattr(real, "__wrapped__", real)

    def spy(self, closure=None):
        seen.append([p.grad.clone() for pg in self.param_groups for p in pg["params"]])
        return real(self, closure)

    spy.hooked = False
    monkeypatch.setattr(torch.optim.SGD, "step", spy)
    named, letters = six_params("cpu")                                               # not homed: every call falls back
    g0 = {n: torch.randn(p.shape, generator=torch.Generator().manual_seed(7)) * 1000.0 for n, p in named}
    for n, p in named:
        p.grad = g0[n].clone()
    opt = fuse(torch.optim.SGD(two_groups(named, letters), lr=0.1, momentum=0.9), amp_scaling=True)
    before = [p.detach().clone() for _, p in named]
    scaled_step(opt, 1, scale=1000.0)
    fs = opt._vbg_fused
    assert seen == [] and recorder == [] and (fs.fallbacks, fs.skipped, fs.launches) == (1, 1, 0) and "homed" in fs.last_fallback
    assert all(torch.equal(b, p) for b, (_, p) in zip(before, named)) and len(opt.state) == 0
    assert all(torch.equal(p.grad, g0[n]) for n, p in named)                         # a skipped step leaves the gradients scaled
    scaled_step(opt, 0, scale=1000.0)
    inv = torch.tensor(1000.0).double().reciprocal().float()
    assert len(seen) == 1 and (fs.fallbacks, fs.skipped) == (2, 1)
    params = [p for pg in opt.param_groups for p in pg["params"]]
    names = {id(p): n for n, p in named}
    assert all(torch.equal(g, g0[names[id(p)]] * inv) for g, p in zip(seen[0], params))          # what the parent step saw: g * inv
    assert all(not torch.equal(b, p) for b, (_, p) in zip(before, named))
    for n, p in named:
        p.grad = g0[n].clone()
    scaled_step(opt, 0, scale=None)                                                  # unscaled by the caller: stepped on as it is
    assert len(seen) == 2 and all(torch.equal(g, g0[names[id(p)]]) for g, p in zip(seen[1], params))


def test_argument_errors_of_the_amp_entries():
    from vbg import lib as L
    sgd, adam = L.lib.vbg_sgd_step_seg_amp, L.lib.vbg_adam_step_seg_amp
    hs, ha = (L.SgdGroupOpt * 33)(), (L.AdamGroupOpt * 33)()
    for h in ha:
        h.step = 1
    buf = (C.c_float * 64)()
    base = C.addressof(buf) + (-C.addressof(buf)) % 16
    a, odd, fi, sc = C.c_void_p(base), C.c_void_p(base + 4), C.c_void_p(base + 32), C.c_void_p(base + 36)
    for ng in (1, 32):
        assert sgd(None, None, None, None, 0, hs, ng, sc, fi, None) == 0             # nchunks == 0 is a no-op ...
        assert adam(None, None, None, None, None, None, 0, ha, ng, None, fi, None) == 0
        assert sgd(None, None, None, None, 0, hs, ng, sc, None, None) == -1          # ... but found_inf is required even then
        assert adam(None, None, None, None, None, None, 0, ha, ng, sc, None, None) == -1
    for ng in (0, 33, -1):
        assert sgd(a, a, a, a, 1, hs, ng, sc, fi, None) == -1
        assert adam(a, a, a, a, a, a, 1, ha, ng, sc, fi, None) == -1
    assert sgd(a, a, a, a, -1, hs, 1, sc, fi, None) == -1
    assert adam(a, a, a, a, a, a, -1, ha, 1, sc, fi, None) == -1
    # everything in place but one thing (host memory: these calls must return before any launch)
    assert sgd(a, a, a, a, 1, hs, 1, sc, None, None) == -1                           # NULL found_inf
    assert adam(a, a, a, a, a, a, 1, ha, 1, None, None, None) == -1
    for k in range(4):                                                               # misaligned p / g / mom / table
        args = [a, a, a, a]
        args[k] = odd
        assert sgd(*args, 1, hs, 1, sc, fi, None) == -1
    for k in range(6):                                                               # misaligned p / g / m / v / vmax / table
        args = [a, a, a, a, a, a]
        args[k] = odd
        assert adam(*args, 1, ha, 1, sc, fi, None) == -1
    assert sgd(None, a, a, a, 1, hs, 1, sc, fi, None) == -1 and sgd(a, None, a, a, 1, hs, 1, sc, fi, None) == -1          # null operands
    assert adam(a, a, None, a, a, a, 1, ha, 1, sc, fi, None) == -1 and adam(a, a, a, a, a, None, 1, ha, 1, sc, fi, None) == -1
    hs[0].momentum = 0.9
    assert sgd(a, a, None, a, 1, hs, 1, sc, fi, None) == -1                          # a group has momentum, no momentum buffer
    ha[1].flags = L.ADAM_AMSGRAD
    assert adam(a, a, a, a, None, a, 1, ha, 2, sc, fi, None) == -1                   # amsgrad flag with vmax NULL
    ha[1].flags = 0
    ha[1].step = 0
    assert adam(a, a, a, a, a, a, 1, ha, 2, sc, fi, None) == -1                      # every group's step >= 1


def test_ops_wrappers_check_the_buffers_and_the_scalars():
    from vbg import ops
    ok = ops.chunk_table([(0, 8, 0), (8, 64, 1)], 2, 72, "cpu")
    z = lambda n=72: torch.zeros(n)
    sc, fi = torch.tensor(2.0), torch.tensor(0.0)
    sgd_hp, adam_hp = [(0.1, 0.9, 0.0, 0.0, 0)] * 2, [(1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0)] * 2
    bad = [((z(), z(), z(), ok, sgd_hp[:1], sc, fi), "sgd"),                          # hyper-parameter sets must match the table's groups
           ((z(), z(), z(64), ok, sgd_hp, sc, fi), "sgd"),                            # buffers shorter than the table's range
           ((z(), z(), None, ok, sgd_hp, sc, fi), "sgd"),                             # momentum without a buffer
           ((z(), z().double(), z(), ok, sgd_hp, sc, fi), "sgd"),
           ((z(), z(), z(), ok, sgd_hp, sc, None), "sgd"),                            # found_inf is required
           ((z(), z(), z(), ok, sgd_hp, sc.double(), fi), "sgd"),                     # fp32 scalars
           ((z(), z(), z(), ok, sgd_hp, sc, torch.zeros(2)), "sgd"),                  # one element each
           ((z(), z(), z(), ok, sgd_hp, 2.0, fi), "sgd"),                             # tensors, not host numbers
           ((z(), z(), z(), z(), None, ok, adam_hp[:1], sc, fi), "adam"),
           ((z(), z(), z(), z(), z(64), ok, adam_hp, sc, fi), "adam"),
           ((z(), z(), z(), z(), None, ok, [adam_hp[0], adam_hp[0][:6] + (1,)], sc, fi), "adam"),          # amsgrad without a buffer
           ((z(), z(), z(), z(), None, ok, adam_hp, sc, fi.to(torch.float16)), "adam"),
           ((z(), z(), z(), z(), None, ok, adam_hp, torch.zeros(1, 2), fi), "adam")]
    for args, which in bad:
        with pytest.raises(ValueError):
            getattr(ops, f"{which}_step_seg_amp")(*args)
    with pytest.raises(ValueError):                                                  # on the buffers' device
        ops.sgd_step_seg_amp(z(), z(), z(), ok, sgd_hp, sc.to("meta"), fi)
