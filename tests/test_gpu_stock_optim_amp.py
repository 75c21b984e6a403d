"""Stock torch.optim objects under torch.amp.GradScaler's protocol for optimizers that consume the scale themselves, on the GPU: the two
AMP entries (csrc/optim.hip vbg_sgd_step_seg_amp / vbg_adam_step_seg_amp -- the AMP instantiation of the kernels behind *_seg_opt) on
canary-filled buffers against the fp64 restatements of tests/test_stock_optim_host.py and, bit for bit, against *_seg_opt on gradients
unscaled beforehand; the early exit of a launch with found_inf set; and `vbg.optim.fuse(optimizer, amp_scaling=True)` under a real
GradScaler against the same loop without the option, bit for bit, and against fp64 torch.optim twins.  Shapes, option sets and the
tolerance `close(..., 1e-6, 1e-7)` are those of tests/test_gpu_stock_optim.py.  Needs a real MI355X."""
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_optim_groups import CHUNK, RUNS, TOTAL, _same, _twin, cut, dev, inside
from test_gpu_small_kernels import _opt_inputs, bits, close, gen, rnd
from test_gpu_stock_optim import ADAM_OPT, AMS_SCALES, AMSGRAD, CONFIGS, COUPLED, FIRST, MAXIMIZE, SGD_OPT, _state_equal, group_mask
from test_optim_groups_host import LAYOUT, six_params
from test_stock_optim_host import adam_opt_ref, sgd_opt_ref, two_groups


@pytest.fixture(scope="module")
def ops():
    from vbg import ops as _ops
    return _ops


def scalars(scale, found_inf=0.0):
    """(grad_scale, found_inf, inv) as GradScaler hands them over; inv: torch's own inverse, `_scale.double().reciprocal().float()`"""
    sc = torch.full((), float(scale), device=dev())
    return sc, torch.full((), float(found_inf), device=dev()), sc.double().reciprocal().float().cpu()


def _sgd_state(grads):
    """the momentum buffer of test_sgd_step_seg_opt: groups 0 and 2 hold a buffer that goes with the gradients, canaries elsewhere"""
    return torch.where(group_mask(RUNS, TOTAL, (0, 2)), grads[0] * (0.5 + torch.rand(TOTAL, generator=gen(113))), rnd(TOTAL, seed=112))


def _adam_state(grads, hp0):
    """the moments of test_gpu_stock_optim._adam_case: zero where a group takes its first step, canaries outside the runs"""
    ins = inside(RUNS, TOTAL)
    fresh = group_mask(RUNS, TOTAL, [k for k, h in enumerate(hp0) if h[5] == 1])
    m0, v0, x0 = rnd(TOTAL, seed=115) * 0.01, 1e-3 * (0.1 + torch.rand(TOTAL, generator=gen(116))), 1e-3 * (0.1 + torch.rand(TOTAL, generator=gen(117)))
    m0 = torch.where(ins, grads[0] * 0.1 * (0.5 + torch.rand(TOTAL, generator=gen(113))), m0)
    return [torch.where(fresh, torch.zeros(()), t) for t in (m0, v0, x0)]


@pytest.mark.parametrize("scale", [1024.0, 1000.0])
def test_sgd_step_seg_amp(ops, scale):
    p0, grads = _opt_inputs(TOTAL, steps=4)
    mom0 = _sgd_state(grads)
    table = ops.chunk_table(cut(RUNS, CHUNK), 3, TOTAL, dev())
    sc, fi, inv = scalars(scale)
    p, mom = p0.to(dev()), mom0.to(dev())
    q, qmom = p0.to(dev()), mom0.to(dev())          # vbg_sgd_step_seg_opt on gradients unscaled beforehand
    pr, mr = p0.double(), mom0.double()
    m, mm = inside(RUNS, TOTAL), group_mask(RUNS, TOTAL, (0, 1))
    same_bits = True
    for i, g in enumerate(grads):
        g0 = g * scale                              # what the scaler's backward leaves in .grad (fp32)
        gd = g0.to(dev())
        hp = [h[:4] + (h[4] | (FIRST if k == 1 and i == 0 else 0),) for k, h in enumerate(SGD_OPT)]
        ops.sgd_step_seg_amp(p, gd, mom, table, hp, sc, fi)
        unscaled = g0 * inv                         # torch, fp32: one rounded product
        assert torch.equal(bits(gd)[m], bits(unscaled)[m])          # g afterwards: the unscaled gradient, bit for bit
        assert torch.equal(bits(gd)[~m], bits(g0)[~m])              # ... and untouched outside the runs
        ops.sgd_step_seg_opt(q, unscaled.to(dev()), qmom, table, hp, 1.0)
        same_bits = same_bits and torch.equal(bits(p), bits(q)) and torch.equal(bits(mom), bits(qmom))
        for s, n, k in RUNS:
            pr[s:s + n], mr[s:s + n] = sgd_opt_ref(pr[s:s + n], g0.double()[s:s + n], mr[s:s + n], *hp[k], float(inv))
    assert close(p.cpu()[m], pr[m], 1e-6, 1e-7) and close(mom.cpu()[mm], mr[mm], 1e-6, 1e-7)
    assert not torch.equal(p.cpu()[m], p0[m]) and not torch.equal(mom.cpu()[mm], mom0[mm])
    assert torch.equal(bits(p)[~m], bits(p0)[~m])
    assert torch.equal(bits(mom)[~mm], bits(mom0)[~mm])          # the momentum buffer of the momentum-0 group included
    print(f"sgd amp, scale {scale}: bit-equal to vbg_sgd_step_seg_opt on g * inv: {same_bits}")
    if scale == 1024.0:                             # g * 2^-10 is exact: the two launches run the same statements on the same numbers
        assert same_bits


@pytest.mark.parametrize("scale", [1024.0, 1000.0])
def test_adam_step_seg_amp(ops, scale):
    p0, grads = _opt_inputs(TOTAL, steps=4)
    grads = [g * s for g, s in zip(grads, AMS_SCALES)]
    st0 = _adam_state(grads, ADAM_OPT)
    table = ops.chunk_table(cut(RUNS, CHUNK), 3, TOTAL, dev())
    sc, fi, inv = scalars(scale)
    a = [t.to(dev()) for t in [p0] + st0]
    b = [t.to(dev()) for t in [p0] + st0]          # vbg_adam_step_seg_opt on gradients unscaled beforehand
    ref = [t.double() for t in [p0] + st0]
    ins, ams = inside(RUNS, TOTAL), group_mask(RUNS, TOTAL, (0,))
    same_bits = True
    for i, g in enumerate(grads):
        g0 = g * scale
        gd = g0.to(dev())
        hp = [h[:5] + (h[5] + i, h[6]) for h in ADAM_OPT]
        ops.adam_step_seg_amp(a[0], gd, a[1], a[2], a[3], table, hp, sc, fi)
        unscaled = g0 * inv
        assert torch.equal(bits(gd)[ins], bits(unscaled)[ins]) and torch.equal(bits(gd)[~ins], bits(g0)[~ins])
        ops.adam_step_seg_opt(b[0], unscaled.to(dev()), b[1], b[2], b[3], table, hp, 1.0)
        same_bits = same_bits and all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))
        for s, n, k in RUNS:
            sl = slice(s, s + n)
            ref[0][sl], ref[1][sl], ref[2][sl], ref[3][sl] = adam_opt_ref(ref[0][sl], g0.double()[sl], ref[1][sl], ref[2][sl], ref[3][sl], *hp[k], float(inv))
    p, m, v, x = a
    assert close(p.cpu()[ins], ref[0][ins], 1e-6, 1e-7) and close(m.cpu()[ins], ref[1][ins], 1e-6, 1e-7) and close(v.cpu()[ins], ref[2][ins], 1e-6, 1e-7)
    assert close(x.cpu()[ams], ref[3][ams], 1e-6, 1e-7) and not torch.equal(p.cpu()[ins], p0[ins])
    for got, was in ((p, p0), (m, st0[0]), (v, st0[1])):
        assert torch.equal(bits(got)[~ins], bits(was)[~ins])
    assert torch.equal(bits(x)[~ams], bits(st0[2])[~ams])          # max_exp_avg_sq outside the amsgrad group: untouched
    print(f"adam amp, scale {scale}: bit-equal to vbg_adam_step_seg_opt on g * inv: {same_bits}")
    if scale == 1024.0:
        assert same_bits


@pytest.mark.parametrize("which", ["sgd", "adam"])
def test_null_scale_is_the_opt_entry_with_scale_one(ops, which):
    """grad_scale NULL (the caller ran scaler.unscale_): the bits of *_seg_opt with grad_scale 1.0, and g is not written"""
    p0, grads = _opt_inputs(TOTAL, steps=3)
    st0 = [_sgd_state(grads)] if which == "sgd" else _adam_state(grads, ADAM_OPT)
    table = ops.chunk_table(cut(RUNS, CHUNK), 3, TOTAL, dev())
    _, fi, _ = scalars(1.0)
    a, b = [t.to(dev()) for t in [p0] + st0], [t.to(dev()) for t in [p0] + st0]
    for i, g in enumerate(grads):
        gd = g.to(dev())
        if which == "sgd":
            hp = [h[:4] + (h[4] | (FIRST if k == 1 and i == 0 else 0),) for k, h in enumerate(SGD_OPT)]
            ops.sgd_step_seg_amp(a[0], gd, a[1], table, hp, None, fi)
            ops.sgd_step_seg_opt(b[0], gd, b[1], table, hp, 1.0)
        else:
            hp = [h[:5] + (h[5] + i, h[6]) for h in ADAM_OPT]
            ops.adam_step_seg_amp(a[0], gd, a[1], a[2], a[3], table, hp, None, fi)
            ops.adam_step_seg_opt(b[0], gd, b[1], b[2], b[3], table, hp, 1.0)
        assert torch.equal(bits(gd), bits(g))
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b)), (which, i)
    assert not torch.equal(a[0].cpu(), p0)


@pytest.mark.parametrize("which,flag", [("sgd", 1.0), ("adam", 2.0)])
def test_found_inf_makes_the_launch_a_no_op(ops, which, flag):
    """200 704 elements in 64-element rows: 3136 rows for a grid capped at 2048 blocks, so blocks on their second row exist -- every block
    leaves before its first.  p, g and every state buffer keep their bits over the whole allocation (an inf sits in g, as it would);
    flag 2.0: GradScaler sums the flags of several devices"""
    n = 200704
    runs = [(0, n, 0), (n, 8, 1)]
    rows = cut(runs, CHUNK)
    assert len(rows) == 3136 + 1
    table = ops.chunk_table(rows, 2, n + 8, dev())
    p0, grads = _opt_inputs(n + 8, steps=1)
    g0 = grads[0] * 1024.0
    g0[77] = float("inf")
    sc, fi, _ = scalars(1024.0, flag)
    host = [p0, g0] + [rnd(n + 8, seed=130 + j).abs() * 1e-3 for j in range(1 if which == "sgd" else 3)]
    d = [t.to(dev()) for t in host]
    if which == "sgd":
        ops.sgd_step_seg_amp(d[0], d[1], d[2], table, [h[:4] + (h[4] | FIRST,) for h in SGD_OPT[:2]], sc, fi)
    else:
        hp = [ADAM_OPT[0][:6] + (AMSGRAD | COUPLED,), ADAM_OPT[1][:5] + (1, MAXIMIZE)]
        ops.adam_step_seg_amp(d[0], d[1], d[2], d[3], d[4], table, hp, sc, fi)
    for got, was in zip(d, host):
        assert torch.equal(bits(got), bits(was))
    # the same launch with the flag at zero does step (the no-op above is the flag's doing)
    if which == "sgd":
        ops.sgd_step_seg_amp(d[0], d[1], d[2], table, [h[:4] + (h[4] | FIRST,) for h in SGD_OPT[:2]], sc, scalars(1.0)[1])
    else:
        ops.adam_step_seg_amp(d[0], d[1], d[2], d[3], d[4], table, hp, sc, scalars(1.0)[1])
    assert not torch.equal(bits(d[0])[:n], bits(p0)[:n]) and float(d[1][78]) == float(g0[78]) / 1024.0


# ------------------------------------------------------------------------------------------
# vbg.optim.fuse(..., amp_scaling=True) under a real GradScaler
# ------------------------------------------------------------------------------------------
def _amp_pair(config, amp, seed=0):
    """_pair of tests/test_gpu_stock_optim.py with fuse()'s amp_scaling argument"""
    from vbg import optim as vo
    cls, kw, b = CONFIGS[config]
    named, letters = six_params(dev(), seed=seed)
    group = vo.FlatGroup(named, dev())
    twin = _twin(named, torch.float64)
    opt = vo.fuse(cls(two_groups(named, letters, **b), **kw), seg_chunk=CHUNK, amp_scaling=True) if amp else vo.fuse(cls(two_groups(named, letters, **b), **kw), seg_chunk=CHUNK)
    assert getattr(opt, "_step_supports_amp_scaling", False) == amp
    return named, twin, opt, cls(two_groups(twin, letters, **b), **kw), group


def _scaler_loop(configs, amp, nsteps, inf_at, clip=None):
    """the loop of test_gradscaler_skips_the_step_with_an_inf (quadratic loss, one shared GradScaler, init_scale 1024, growth_interval 2)
    over one fused optimizer per config, each on its own six parameters; inf_at: {step: index of the optimizer whose gradient gets an
    inf}; clip: scaler.unscale_ + clip_grad_norm_(max_norm=clip) before each scaler.step.  The fp64 torch twins (no scaler) take every
    step their optimizer was not skipped in.  -> (per-step records, the sides)"""
    sides = [_amp_pair(config, amp, seed=j) for j, config in enumerate(configs)]
    w = {n: rnd(*s, seed=400 + i) for i, (n, s, _) in enumerate(LAYOUT)}
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0, growth_interval=2)
    records = []
    for step in range(nsteps):
        for named, twin, opt, topt, group in sides:
            group.zero_grad()
        loss = sum(((p * w[n].to(dev())) ** 2).sum() for named, *_ in sides for n, p in named)
        scaler.scale(loss).backward()
        for named, twin, opt, topt, group in sides:
            assert all(p.grad is gv for p, gv in zip(group.params, group.gviews))
        if step in inf_at:
            sides[inf_at[step]][0][2][1].grad.view(-1)[3] = float("inf")
        scaled = [group.gflat.clone() for *_, group in sides]
        for named, twin, opt, topt, group in sides:
            if clip is not None:
                scaler.unscale_(opt)
                torch.nn.utils.clip_grad_norm_([p for _, p in named], clip)
            scaler.step(opt)
        scaler.update()
        rec = {"scale": scaler.get_scale(), "scaled": scaled}
        for j, (named, twin, opt, topt, group) in enumerate(sides):
            opt._vbg_fused.reconcile()
            rec[j] = {"p": group.pflat.clone(), "g": group.gflat.clone(),
                      "state": {(n, k): (t.clone() if k != "step" else float(t)) for n, p in named for k, t in opt.state.get(p, {}).items()}}
            if inf_at.get(step) != j and clip is None:
                topt.zero_grad()
                sum(((q * w[n].double()) ** 2).sum() for n, q in twin).backward()
                topt.step()
        records.append(rec)
    return records, sides


def _assert_same_records(plain, amp, nopt, inf_at, clip=None):
    for step, (a, b) in enumerate(zip(plain, amp)):
        assert a["scale"] == b["scale"], step
        for j in range(nopt):
            assert torch.equal(bits(a[j]["p"]), bits(b[j]["p"])), (step, j)
            assert list(a[j]["state"]) == list(b[j]["state"]), (step, j)
            for key, t in a[j]["state"].items():
                u = b[j]["state"][key]
                assert (t == u) if key[1] == "step" else torch.equal(bits(t), bits(u)), (step, j, key)
            if inf_at.get(step) == j and clip is None:
                # the skipped step: the generic route has unscaled the gradients before it learnt of the inf; the launch that exits early
                # leaves them as they were (torch's own fused optimizers do the same)
                inv = torch.full((), plain[step - 1]["scale"] if step else 1024.0).double().reciprocal().float()
                assert torch.equal(bits(b[j]["g"]), bits(b["scaled"][j])) and torch.equal(bits(a[j]["g"]), bits(a["scaled"][j].cpu() * inv))
            else:
                assert torch.equal(bits(a[j]["g"]), bits(b[j]["g"])), (step, j)


@pytest.mark.parametrize("config", ["sgd_nesterov", "adamw_amsgrad"])
def test_gradscaler_loop_with_an_inf_in_step_two(config):
    """four steps, an inf planted in the second: parameters, state, step counts, .grad and the scale equal the loop without the option bit
    for bit after every step; both within the tolerance of the fp64 twin"""
    inf_at = {1: 0}
    plain, sides_p = _scaler_loop([config], False, 4, inf_at)
    amp, sides_a = _scaler_loop([config], True, 4, inf_at)
    _assert_same_records(plain, amp, 1, inf_at)
    assert [r["scale"] for r in amp] == [1024.0, 512.0, 512.0, 1024.0]
    assert torch.equal(bits(amp[1][0]["p"]), bits(amp[0][0]["p"]))          # the skipped step moved nothing
    for named, twin, opt, topt, group in (sides_p[0], sides_a[0]):
        assert _same(named, twin, "after three GradScaler steps and a skipped one") and _state_equal(named, twin, opt, topt)
    fs_p, fs_a = sides_p[0][2]._vbg_fused, sides_a[0][2]._vbg_fused
    assert (fs_p.launches, fs_p.fallbacks, fs_p.skipped) == (3, 0, 0), fs_p.last_fallback
    assert (fs_a.launches, fs_a.fallbacks, fs_a.skipped) == (4, 0, 1), fs_a.last_fallback


@pytest.mark.parametrize("config", ["sgd_nesterov", "adamw_amsgrad"])
def test_inf_on_the_first_step(config):
    """the momentum buffers' first step / Adam's fresh state, skipped, then two good steps"""
    inf_at = {0: 0}
    plain, sides_p = _scaler_loop([config], False, 3, inf_at)
    amp, sides_a = _scaler_loop([config], True, 3, inf_at)
    assert amp[0][0]["state"] == {} and plain[0][0]["state"] == {}
    _assert_same_records(plain, amp, 1, inf_at)
    for named, twin, opt, topt, group in (sides_p[0], sides_a[0]):
        assert _same(named, twin, "after a skipped first step and two good ones") and _state_equal(named, twin, opt, topt)
    fs = sides_a[0][2]._vbg_fused
    assert (fs.launches, fs.fallbacks, fs.skipped) == (3, 0, 1), fs.last_fallback


def test_two_optimizers_one_scaler_inf_in_the_second():
    inf_at = {1: 1}
    configs = ["sgd_nesterov", "adamw_amsgrad"]
    plain, sides_p = _scaler_loop(configs, False, 3, inf_at)
    amp, sides_a = _scaler_loop(configs, True, 3, inf_at)
    _assert_same_records(plain, amp, 2, inf_at)
    assert [r["scale"] for r in amp] == [1024.0, 512.0, 512.0]
    assert not torch.equal(bits(amp[1][0]["p"]), bits(amp[0][0]["p"])) and torch.equal(bits(amp[1][1]["p"]), bits(amp[0][1]["p"]))          # the first stepped, the second did not
    for sides in (sides_p, sides_a):
        for named, twin, opt, topt, group in sides:
            assert _same(named, twin) and _state_equal(named, twin, opt, topt)
    assert [(s[2]._vbg_fused.launches, s[2]._vbg_fused.skipped, s[2]._vbg_fused.fallbacks) for s in sides_a] == [(3, 0, 0), (3, 1, 0)]
    assert [(s[2]._vbg_fused.launches, s[2]._vbg_fused.fallbacks) for s in sides_p] == [(3, 0), (2, 0)]


@pytest.mark.parametrize("config", ["sgd_nesterov", "adamw_amsgrad"])
def test_unscale_clip_then_step(config):
    """scaler.unscale_(opt), clip_grad_norm_, scaler.step(opt): the protocol hands over grad_scale None and the flag unscale_ found"""
    inf_at = {1: 0}
    plain, _ = _scaler_loop([config], False, 3, inf_at, clip=1.0)
    amp, sides = _scaler_loop([config], True, 3, inf_at, clip=1.0)
    _assert_same_records(plain, amp, 1, inf_at, clip=1.0)
    assert not torch.equal(bits(amp[2][0]["p"]), bits(amp[1][0]["p"])) and torch.equal(bits(amp[1][0]["p"]), bits(amp[0][0]["p"]))
    g = amp[2][0]["g"]
    assert abs(float(g.double().norm()) - 1.0) < 1e-3          # the clip did bite
    fs = sides[0][2]._vbg_fused
    assert (fs.launches, fs.fallbacks, fs.skipped) == (3, 0, 1), fs.last_fallback


def test_no_host_sync_between_backward_and_update():
    """torch's sync-debug mode around scaler.step(opt); scaler.update(): the generic route's found_inf.item() raises, the protocol's
    route issues nothing that waits for the device (second step: the chunk table's upload belongs to the first)"""
    w = {n: rnd(*s, seed=400 + i) for i, (n, s, _) in enumerate(LAYOUT)}
    raised = {}
    for amp in (False, True):
        named, twin, opt, topt, group = _amp_pair("adamw_amsgrad", amp)
        scaler = torch.amp.GradScaler("cuda", init_scale=1024.0)
        for step in range(2):
            group.zero_grad()
            scaler.scale(sum(((p * w[n].to(dev())) ** 2).sum() for n, p in named)).backward()
            torch.cuda.synchronize()
            if step == 1:
                torch.cuda.set_sync_debug_mode("error")
            try:
                scaler.step(opt)
                scaler.update()
                raised[amp] = None
            except RuntimeError as e:
                raised[amp] = str(e)
            finally:
                torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
    print("sync-debug mode, generic route:", raised[False], "| amp_scaling route:", raised[True])
    assert raised[True] is None
    assert raised[False] is not None and "synchroniz" in raised[False]
    assert opt._vbg_fused.launches == 2 and opt._vbg_fused.fallbacks == 0


def test_stock_loop_step_under_autocast_with_a_shared_scaler(golden, tmp_path):
    """one stock-loop step of the e2e fixture model under fp16 autocast: scaler.step(sgd); scaler.step(adamw); scaler.update() with both
    optimizers fused with the option against the same step without it, on the SAME scaled gradients (one backward: two backward passes
    of this model do not give the same bits), default scale 65536 -- every parameter bit-equal"""
    from test_gpu_model import to_dev
    from test_gpu_train_loop import _net, _torch_opts
    from test_oracle_golden import _e2e_inputs
    from vbg import ops
    from vbg import optim as vo
    dbatch = to_dev(_e2e_inputs(golden("e2e.npz")), dev())
    net = _net(tmp_path, "amp", dev())
    random.seed(100)
    with torch.autocast("cuda", dtype=torch.float16):
        loss = net(*dbatch)
    torch.amp.GradScaler("cuda").scale(loss).backward()
    params = dict(net.named_parameters())
    p0 = {n: p.detach().clone() for n, p in params.items()}
    g0 = {n: p.grad.detach().clone() for n, p in params.items() if p.grad is not None}
    assert max(float(g.abs().max()) for g in g0.values()) > 100.0          # scaled gradients
    after = {}
    for amp in (False, True):
        with torch.no_grad():
            for n, p in params.items():
                p.copy_(p0[n])
                if n in g0:
                    p.grad.copy_(g0[n])
        ops.bump_weight_epoch()
        oc, ob = (vo.fuse(o, amp_scaling=amp) for o in _torch_opts(net))
        scaler = torch.amp.GradScaler("cuda")
        scaler.scale(torch.zeros((), device=dev()))          # (the scale tensor comes into being at the first scale() call)
        scaler.step(oc)
        scaler.step(ob)
        scaler.update()
        for o in (oc, ob):
            o._vbg_fused.reconcile()
            fs = o._vbg_fused
            assert (fs.launches, fs.fallbacks, fs.skipped) == (1, 0, 0), fs.last_fallback
        assert scaler.get_scale() == 65536.0
        after[amp] = ({n: p.detach().clone() for n, p in params.items()}, {n: p.grad.detach().clone() for n, p in params.items() if p.grad is not None})
    moved = 0
    for n in params:
        assert torch.equal(bits(after[True][0][n]), bits(after[False][0][n])), n
        moved += not torch.equal(after[True][0][n], p0[n])
    for n in g0:                                    # and .grad holds the unscaled gradient either way
        assert torch.equal(bits(after[True][1][n]), bits(after[False][1][n])), n
        assert torch.equal(bits(after[True][1][n]), bits(g0[n] * (1.0 / 65536.0))), n
    assert moved > len(g0) // 2, (moved, len(g0))
