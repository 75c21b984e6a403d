"""Stock torch.optim objects on the fused kernels, on the GPU: the two entries with every torch.optim option per group
(csrc/optim.hip vbg_sgd_step_seg_opt / vbg_adam_step_seg_opt) on canary-filled buffers against the fp64 restatements of
tests/test_stock_optim_host.py (which that file holds against torch.optim itself), bit-equality of the default case with
vbg_sgd_step_seg / vbg_adamw_step_seg, the grid-stride, and vbg.optim.fuse against fp64 torch.optim twins: options, skipped
parameters, schedulers, GradScaler with an inf step, checkpoints in both directions, one stock-loop step of the model.  Every
tolerance is `close(..., 1e-6, 1e-7)` of tests/test_gpu_small_kernels.py.  Needs a real MI355X."""
import copy
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_optim_groups import ADAMW_HP, CHUNK, LAMBDAS, RUNS, SGD_HP, TOTAL, _grads, _same, _twin, cut, dev, inside
from test_gpu_small_kernels import _opt_inputs, bits, close, f32, gen, rnd
from test_optim_groups_host import LAYOUT, six_params
from test_stock_optim_host import adam_opt_ref, sgd_opt_ref, two_groups

NESTEROV, MAXIMIZE, FIRST = 1, 2, 4
AMSGRAD, COUPLED = 1, 4
# lr, momentum, dampening, wd, flags: (nesterov), (dampening 0.3), (maximize, momentum 0)
SGD_OPT = [(f32(0.005), f32(0.9), f32(0.0), f32(0.005), NESTEROV), (f32(0.02), f32(0.5), f32(0.3), f32(0.0), 0), (f32(0.001), f32(0.0), f32(0.0), f32(0.05), MAXIMIZE)]
# lr, b1, b2, eps, wd, first step, flags: (amsgrad), (maximize + coupled), (decoupled plain).  beta2 = 0.9 in the amsgrad group: exp_avg_sq
# forgets fast enough to fall below its maximum when the gradients shrink (with 0.999 it keeps growing on most elements)
ADAM_OPT = [(f32(1e-3), f32(0.9), f32(0.9), f32(1e-8), f32(0.01), 1, AMSGRAD), (f32(3e-4), f32(0.8), f32(0.99), f32(1e-6), f32(0.02), 1000, MAXIMIZE | COUPLED),
            (f32(2e-3), f32(0.95), f32(0.9995), f32(1e-7), f32(0.1), 3, 0)]
AMS_SCALES = (2.0, 0.1, 0.05, 1.5)          # the gradients shrink after the first step: exp_avg_sq falls below its maximum


@pytest.fixture(scope="module")
def ops():
    from vbg import ops as _ops
    return _ops


def group_mask(runs, total, groups):
    return inside([r for r in runs if r[2] in groups], total)


@pytest.mark.parametrize("gs", [1.0, 0.125])
def test_sgd_step_seg_opt(ops, gs):
    p0, grads = _opt_inputs(TOTAL, steps=4)
    # groups 0 and 2 start on a buffer that exists and goes with the gradients (same signs: the sums do not cancel, see _opt_inputs);
    # group 1 takes its first step, which overwrites whatever its runs hold; canaries everywhere else
    mom0 = torch.where(group_mask(RUNS, TOTAL, (0, 2)), grads[0] * (0.5 + torch.rand(TOTAL, generator=gen(113))), rnd(TOTAL, seed=112))
    table = ops.chunk_table(cut(RUNS, CHUNK), 3, TOTAL, dev())
    p, mom = p0.to(dev()), mom0.to(dev())
    pr, mr = p0.double(), mom0.double()
    for i, g in enumerate(grads):
        gd = g.to(dev())
        hp = [h[:4] + (h[4] | (FIRST if k == 1 and i == 0 else 0),) for k, h in enumerate(SGD_OPT)]
        ops.sgd_step_seg_opt(p, gd, mom, table, hp, gs)
        assert torch.equal(bits(gd), bits(g))          # g bit-unchanged everywhere
        for s, n, k in RUNS:
            pr[s:s + n], mr[s:s + n] = sgd_opt_ref(pr[s:s + n], g.double()[s:s + n], mr[s:s + n], *hp[k], gs)
    m, mm = inside(RUNS, TOTAL), group_mask(RUNS, TOTAL, (0, 1))
    assert close(p.cpu()[m], pr[m], 1e-6, 1e-7) and close(mom.cpu()[mm], mr[mm], 1e-6, 1e-7)
    assert not torch.equal(p.cpu()[m], p0[m]) and not torch.equal(mom.cpu()[mm], mom0[mm])
    assert torch.equal(bits(p)[~m], bits(p0)[~m])      # outside the runs: untouched
    assert torch.equal(bits(mom)[~mm], bits(mom0)[~mm])          # ... and the momentum buffer in the momentum-0 group as well


def _adam_case(total, runs, hp0, gs, ops, steps=4):
    """`steps` steps of vbg_adam_step_seg_opt over `runs` (group k starts at step hp0[k][5]) and of the fp64 rule with and without
    the amsgrad flag -> everything the assertions need"""
    p0, grads = _opt_inputs(total, steps=steps)
    grads = [g * s for g, s in zip(grads, AMS_SCALES)]
    ins = inside(runs, total)
    fresh = group_mask(runs, total, [k for k, h in enumerate(hp0) if h[5] == 1])
    m0, v0, x0 = rnd(total, seed=115) * 0.01, 1e-3 * (0.1 + torch.rand(total, generator=gen(116))), 1e-3 * (0.1 + torch.rand(total, generator=gen(117)))
    m0 = torch.where(ins, grads[0] * 0.1 * (0.5 + torch.rand(total, generator=gen(113))), m0)          # late steps: moments that go with the gradients
    m0, v0, x0 = (torch.where(fresh, torch.zeros(()), t) for t in (m0, v0, x0))                         # a first step starts from zero
    table = ops.chunk_table(cut(runs, CHUNK), len(hp0), total, dev())
    p, m, v, x = (t.to(dev()) for t in (p0, m0, v0, x0))
    ref = {True: [t.double() for t in (p0, m0, v0, x0)], False: [t.double() for t in (p0, m0, v0, x0)]}
    ams = group_mask(runs, total, [k for k, h in enumerate(hp0) if h[6] & AMSGRAD])
    above = []                                         # per step: elements of the amsgrad groups whose maximum lies above exp_avg_sq
    for i, g in enumerate(grads):
        gd = g.to(dev())
        hp = [h[:5] + (h[5] + i, h[6]) for h in hp0]
        ops.adam_step_seg_opt(p, gd, m, v, x, table, hp, gs)
        assert torch.equal(bits(gd), bits(g))
        for with_flag in (True, False):
            r = ref[with_flag]
            for s, n, k in runs:
                sl = slice(s, s + n)
                h = hp[k] if with_flag else hp[k][:6] + (hp[k][6] & ~AMSGRAD,)
                r[0][sl], r[1][sl], r[2][sl], r[3][sl] = adam_opt_ref(r[0][sl], g.double()[sl], r[1][sl], r[2][sl], r[3][sl], *h, gs)
        above.append(int((ref[True][3][ams] > ref[True][2][ams]).sum()))
    ref["above"] = above
    return (p, m, v, x), (p0, m0, v0, x0), ref


@pytest.mark.parametrize("gs", [1.0, 0.125])
def test_adam_step_seg_opt(ops, gs):
    (p, m, v, x), (p0, m0, v0, x0), ref = _adam_case(TOTAL, RUNS, ADAM_OPT, gs, ops)
    pr, mr, vr, xr = ref[True]
    ins, ams = inside(RUNS, TOTAL), group_mask(RUNS, TOTAL, (0,))
    assert close(p.cpu()[ins], pr[ins], 1e-6, 1e-7) and close(m.cpu()[ins], mr[ins], 1e-6, 1e-7) and close(v.cpu()[ins], vr[ins], 1e-6, 1e-7)
    assert close(x.cpu()[ams], xr[ams], 1e-6, 1e-7)
    assert not torch.equal(p.cpu()[ins], p0[ins])
    for got, was in ((p, p0), (m, m0), (v, v0)):
        assert torch.equal(bits(got)[~ins], bits(was)[~ins])
    assert torch.equal(bits(x)[~ams], bits(x0)[~ams])          # max_exp_avg_sq: read and written only in chunks of the amsgrad group
    # the flag matters on this data: in steps 2 and 3 the maximum lies above exp_avg_sq everywhere, and the rule without it is another rule
    print("amsgrad group:", int(ams.sum()), "elements; with max_exp_avg_sq > exp_avg_sq after each step:", ref["above"])
    assert ref["above"][0] == 0 and min(ref["above"][1:3]) > int(ams.sum()) * 3 // 4
    assert not close(ref[False][0][ams], pr[ams], 1e-6, 1e-7)


@pytest.mark.parametrize("which", ["sgd", "adam"])
def test_default_case_has_the_bits_of_the_segmented_entries(ops, which):
    """flags 0 (beyond `first`), dampening 0: the statements of sgd_update / adamw_update, so vbg_sgd_step_seg / vbg_adamw_step_seg bit for bit"""
    table = ops.chunk_table(cut(RUNS, CHUNK), 3, TOTAL, dev())
    p0, grads = _opt_inputs(TOTAL)
    n_state = 1 if which == "sgd" else 2
    a = [p0.to(dev())] + [rnd(TOTAL, seed=120 + j).abs().to(dev()) * 1e-3 for j in range(n_state)]
    b = [t.clone() for t in a]
    sgd_hp = [SGD_HP[0], SGD_HP[1], (f32(0.001), f32(0.25), f32(0.05))]          # every momentum != 0: the old entry writes the buffer
    ins = inside(RUNS, TOTAL)
    for gs in (1.0, 0.125):
        for i, g in enumerate(grads):
            gd = g.to(dev())
            if which == "sgd":
                ops.sgd_step_seg_opt(a[0], gd, a[1], table, [(lr, mo, 0.0, wd, FIRST if i == 0 else 0) for lr, mo, wd in sgd_hp], gs)
                ops.sgd_step_seg(b[0], gd, b[1], table, sgd_hp, i == 0, gs)
            else:
                ops.adam_step_seg_opt(a[0], gd, a[1], a[2], None, table, [h + (i + 1, 0) for h in ADAMW_HP], gs)
                ops.adamw_step_seg(b[0], gd, b[1], b[2], table, ADAMW_HP, i + 1, gs)
            for x, y in zip(a, b):
                assert torch.equal(bits(x), bits(y)), (which, gs, i)
    assert not torch.equal(a[0].cpu()[ins], p0[ins])


@pytest.mark.parametrize("which", ["sgd", "adam"])
def test_more_chunk_rows_than_blocks_opt(ops, which):
    """200 704 elements in 64-element rows: 3136 rows for a grid capped at 2048 blocks, then a second group on a trailing 8-element run"""
    n = 200704
    runs = [(0, n, 0), (n, 8, 1)]
    rows = cut(runs, CHUNK)
    assert len(rows) == 3136 + 1
    if which == "adam":
        hp0 = [ADAM_OPT[0][:6] + (AMSGRAD | COUPLED,), ADAM_OPT[1][:5] + (1, MAXIMIZE)]
        (p, m, v, x), _, ref = _adam_case(n + 8, runs, hp0, 1.0, ops, steps=3)
        pr, mr, vr, xr = ref[True]
        assert close(p, pr, 1e-6, 1e-7) and close(m, mr, 1e-6, 1e-7) and close(v, vr, 1e-6, 1e-7) and close(x[:n], xr[:n], 1e-6, 1e-7)
        return
    table = ops.chunk_table(rows, 2, n + 8, dev())
    p0, grads = _opt_inputs(n + 8)
    p, mom = p0.to(dev()), torch.zeros(n + 8, device=dev())
    pr, mr = p0.double(), torch.zeros(n + 8, dtype=torch.float64)
    for i, g in enumerate(grads):
        hp = [h[:4] + (h[4] | (FIRST if i == 0 else 0),) for h in SGD_OPT[:2]]
        ops.sgd_step_seg_opt(p, g.to(dev()), mom, table, hp)
        for s, k_n, k in runs:
            sl = slice(s, s + k_n)
            pr[sl], mr[sl] = sgd_opt_ref(pr[sl], g.double()[sl], mr[sl], *hp[k], 1.0)
    assert close(p, pr, 1e-6, 1e-7) and close(mom, mr, 1e-6, 1e-7)


# ------------------------------------------------------------------------------------------
# vbg.optim.fuse: the six parameters of the host test, two param groups (A B A A B A over the flat layout)
# ------------------------------------------------------------------------------------------
SGD_KW = dict(lr=f32(0.005), momentum=f32(0.9), weight_decay=f32(0.005))
ADAM_KW = dict(lr=f32(1e-3), betas=(f32(0.9), f32(0.999)), eps=f32(1e-8), weight_decay=f32(0.01))
# name -> (class, constructor arguments, what param group B overrides)
CONFIGS = {
    "sgd_nesterov": (torch.optim.SGD, dict(SGD_KW, nesterov=True), dict(lr=f32(0.02), momentum=f32(0.5), weight_decay=0.0)),
    "sgd_dampening": (torch.optim.SGD, dict(SGD_KW, dampening=f32(0.3)), dict(momentum=0.0, maximize=True)),
    "adamw_amsgrad": (torch.optim.AdamW, dict(ADAM_KW, amsgrad=True, betas=(f32(0.9), f32(0.9))), dict(weight_decay=0.0, lr=f32(3e-4))),
    "adam_weight_decay": (torch.optim.Adam, dict(ADAM_KW), dict(maximize=True)),
    "adamw_coupled_group": (torch.optim.AdamW, dict(ADAM_KW), dict(decoupled_weight_decay=False, amsgrad=True, betas=(f32(0.8), f32(0.9)))),
}
STATE_KEYS = ("momentum_buffer", "exp_avg", "exp_avg_sq", "max_exp_avg_sq")


def _pair(config, dtype=torch.float64, seed=0):
    """six parameters homed in one FlatGroup on the GPU under a fused torch.optim object, and CPU copies of `dtype` under a plain one"""
    from vbg import optim as vo
    cls, kw, b = CONFIGS[config]
    named, letters = six_params(dev(), seed=seed)
    group = vo.FlatGroup(named, dev())
    twin = _twin(named, dtype)
    opt = vo.fuse(cls(two_groups(named, letters, **b), **kw), seg_chunk=CHUNK)
    topt = cls(two_groups(twin, letters, **b), **kw)
    assert group.names == [n for n, _, _ in LAYOUT] and isinstance(opt, cls) and type(opt) is not cls
    return named, twin, opt, topt, group


def _give(named, twin, group, grads, absent=()):
    """the same gradients on both sides: into the flat views (re-attached first) and as the twin's .grad; `absent`: grad None on both"""
    group.zero_grad()
    for (n, p), (_, q) in zip(named, twin):
        if n in absent:
            p.grad = q.grad = None
        else:
            p.grad.copy_(grads[n].to(dev()))
            q.grad = grads[n].to(q.dtype).clone()


def _state_equal(named, twin, opt, topt):
    ok = len(opt.state) == len(topt.state) or print("state entries", len(opt.state), len(topt.state))
    for (n, p), (_, q) in zip(named, twin):
        if (p in opt.state) != (q in topt.state) or list(opt.state.get(p, {})) != list(topt.state.get(q, {})):
            print("state keys", n, list(opt.state.get(p, {})), list(topt.state.get(q, {})))
            ok = False
            continue
        for k, t in topt.state.get(q, {}).items():
            a = opt.state[p][k]
            if k == "step":
                ok = (float(a) == float(t) and not a.is_cuda) and ok or print("step", n, float(a), float(t))
            else:
                ok = (close(a, t, 1e-6, 1e-7) and ok) or print("state", k, n)
    return bool(ok)


@pytest.mark.parametrize("config", list(CONFIGS))
def test_fuse_equals_a_torch_optim_twin(config):
    """three steps with a LambdaLR per group; gradients scaled 2, 0.1, 1.5 so that amsgrad's maximum is not exp_avg_sq itself"""
    named, twin, opt, topt, group = _pair(config)
    sched, tsched = (torch.optim.lr_scheduler.LambdaLR(o, LAMBDAS) for o in (opt, topt))
    tail = group.pflat[4712:].fill_(5.0).clone()
    for step, (grads, scale) in enumerate(zip(_grads(3, seed=310), (2.0, 0.1, 1.5))):
        _give(named, twin, group, {n: g * scale for n, g in grads.items()})
        opt.step()
        topt.step()
        sched.step()
        tsched.step()
        assert [g["lr"] for g in opt.param_groups] == [g["lr"] for g in topt.param_groups]
        assert _same(named, twin, f"after step {step + 1}")
        assert _state_equal(named, twin, opt, topt)
    fs = opt._vbg_fused
    assert (fs.launches, fs.fallbacks, len(fs.tables)) == (3, 0, 1), fs.last_fallback          # one launch per step, one table
    assert opt.param_groups[0]["lr"] != opt.param_groups[1]["lr"] and torch.equal(group.pflat[4712:], tail)
    for _, p in named:                                 # the state tensors are views of the flat buffers
        for k, t in opt.state.get(p, {}).items():
            if k != "step":
                off = p._vbg_flat[1]
                assert t.data_ptr() == fs.flat[k].data_ptr() + 4 * off


@pytest.mark.parametrize("config", ["sgd_nesterov", "adamw_amsgrad"])
def test_a_parameter_without_a_gradient_is_skipped(config):
    """head.weight (group A, between two A slots) has grad None in step 2 only: nothing of it moves in that step, its step count stays
    behind, and step 3 corrects its bias with step 2 -- all as the twin does"""
    named, twin, opt, topt, group = _pair(config)
    who = "head.weight"
    p = dict(named)[who]
    for step, grads in enumerate(_grads(3, seed=311)):
        _give(named, twin, group, grads, absent=(who,) if step == 1 else ())
        before = [p.detach().clone()] + [t.clone() for k, t in opt.state[p].items()]
        opt.step()
        topt.step()
        after = [p.detach()] + list(opt.state[p].values())
        if step == 1:
            assert all(torch.equal(bits(a), bits(b)) for a, b in zip(after, before)) and p.grad is None
        else:
            assert all(not torch.equal(a.cpu(), b.cpu()) for a, b in zip(after, before))
        assert _same(named, twin, f"after step {step + 1}") and _state_equal(named, twin, opt, topt)
    fs = opt._vbg_fused
    # (tables: everything present; one absent; and, where step counts exist, everything present with one parameter a step behind)
    assert (fs.launches, fs.fallbacks, len(fs.tables)) == (3, 0, 3 if config == "adamw_amsgrad" else 2), fs.last_fallback
    if config == "adamw_amsgrad":
        assert [float(opt.state[q]["step"]) for _, q in named] == [2.0 if n == who else 3.0 for n, _ in named]
        assert fs.rows[:, 2].max() == 2                # step 3: (A, 3), (A, 2), (B, 3)


def test_gradscaler_skips_the_step_with_an_inf():
    """scale(loss).backward(), scaler.step(opt), scaler.update() on a quadratic loss, fp64 torch.optim twin without a scaler; the second
    step's gradient holds an inf: no launch, scale halved, parameters and state untouched"""
    named, twin, opt, topt, group = _pair("adamw_amsgrad")
    w = {n: rnd(*s, seed=400 + i) for i, (n, s, _) in enumerate(LAYOUT)}
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0, growth_interval=2)
    fs = opt._vbg_fused
    for step in range(4):
        group.zero_grad()
        loss = sum(((p * w[n].to(dev())) ** 2).sum() for n, p in named)
        scaler.scale(loss).backward()
        assert all(p.grad is gv for p, gv in zip(group.params, group.gviews))          # the scaled gradients sit in the flat views
        if step == 1:
            named[2][1].grad.view(-1)[3] = float("inf")
            before = [p.detach().clone() for _, p in named] + [t.clone() for _, p in named for t in opt.state[p].values()]
        scaler.step(opt)
        scaler.update()
        if step == 1:
            after = [p.detach() for _, p in named] + [t for _, p in named for t in opt.state[p].values()]
            assert scaler.get_scale() == 512.0 and fs.launches == 1
            assert all(torch.equal(bits(a), bits(b)) for a, b in zip(after, before))
            continue
        topt.zero_grad()
        sum(((q * w[n].double()) ** 2).sum() for n, q in twin).backward()
        topt.step()
    assert (fs.launches, fs.fallbacks) == (3, 0) and scaler.get_scale() == 1024.0
    assert _same(named, twin, "after three GradScaler steps and a skipped one") and _state_equal(named, twin, opt, topt)


@pytest.mark.parametrize("config", ["sgd_nesterov", "adamw_amsgrad"])
@pytest.mark.parametrize("direction", ["fused_to_torch", "torch_to_fused"])
def test_checkpoints_in_both_directions(config, direction):
    """two steps on one side, its state_dict() loaded into the other side's optimizer (fp32 twin, its parameters set to the stepped values),
    then a third step with the same gradient on both"""
    named, twin, opt, topt, group = _pair(config, torch.float32)
    grads = _grads(3, seed=312)
    for g, scale in zip(grads[:2], (2.0, 0.1)):
        _give(named, twin, group, {n: t * scale for n, t in g.items()})
        src = opt if direction == "fused_to_torch" else topt
        src.param_groups[1]["lr"] *= 0.75              # what a scheduler changes travels with the checkpoint
        src.step()
    sd = copy.deepcopy(src.state_dict())               # (as through a file: torch's own state_dict() shares its step tensors with the optimizer)
    assert [g["params"] for g in sd["param_groups"]] == [[0, 1, 2, 3], [4, 5]] and sorted(sd["state"]) == list(range(6))
    if direction == "fused_to_torch":                  # clones: the checkpoint does not hold the flat buffers
        assert all(t._base is None and t.untyped_storage().nbytes() <= 4 * 4296 for st in src.state_dict()["state"].values() for t in st.values())
    with torch.no_grad():
        if direction == "fused_to_torch":
            topt.load_state_dict(sd)
            for (_, p), (_, q) in zip(named, twin):
                q.copy_(p.cpu())
        else:
            opt.load_state_dict(sd)
            for (_, p), (_, q) in zip(named, twin):
                p.copy_(q.to(dev()))
    assert [g["lr"] for g in opt.param_groups] == [g["lr"] for g in topt.param_groups] and opt.param_groups[1]["lr"] != opt.param_groups[0]["lr"]
    before = [p.detach().clone() for _, p in named]
    _give(named, twin, group, {n: t * 1.5 for n, t in grads[2].items()})
    opt.step()
    topt.step()
    fs = opt._vbg_fused
    assert fs.fallbacks == 0 and fs.launches == (3 if direction == "fused_to_torch" else 1)
    assert _same(named, twin, "after the step on the loaded state") and _state_equal(named, twin, opt, topt)
    assert all(not torch.equal(b, p) for b, (_, p) in zip(before, named))


def test_stock_loop_step_with_fused_optimizers(golden, tmp_path):
    """the stock-loop step of tests/test_gpu_train_loop.py (torch.optim.SGD + AdamW around the drop-in model) with fuse() on both
    optimizers and without: one fused launch per optimizer, the parameters agree within that file's bound for two runs of the same
    first step (1e-5 relative per parameter), and the next forward multiplies the stepped weights (its loss within that file's 1e-3)"""
    from test_gpu_model import to_dev
    from test_gpu_train_loop import _net, _torch_opts
    from test_oracle_golden import _e2e_inputs
    from vbg import optim as vo
    dbatch = to_dev(_e2e_inputs(golden("e2e.npz")), dev())
    after, losses = {}, {}
    for mode in ("fused", "stock"):
        net = _net(tmp_path, mode, dev())
        oc, ob = _torch_opts(net)
        if mode == "fused":
            oc, ob = vo.fuse(oc), vo.fuse(ob)
        random.seed(100)
        loss = net(*dbatch)
        oc.zero_grad()
        ob.zero_grad()
        loss.backward()
        oc.step()
        ob.step()
        after[mode] = {k: v.detach().clone() for k, v in net.named_parameters()}
        if mode == "fused":
            for o in (oc, ob):
                fs = o._vbg_fused
                assert (fs.launches, fs.fallbacks) == (1, 0), fs.last_fallback
                assert len(fs.tables) == 1 and fs.group is not None and fs.group.valid()
            assert oc._vbg_fused.group is not ob._vbg_fused.group
            unused = [n for n, p in net.named_parameters() if p.grad is None]
            assert unused and all("pooler" in n or "resnet.fc" in n for n in unused)          # in the optimizers, outside the buffers, skipped
            assert all(len(ob.state[p]) == 0 for n, p in net.named_parameters() if "pooler" in n)
        random.seed(101)
        losses[mode] = (float(loss), float(net(*dbatch)))
    a, b = after["fused"], after["stock"]
    worst = max((float((a[k] - b[k]).norm() / (b[k].norm() + 1e-12)), k) for k in a if "pooler" not in k and "key.bias" not in k)
    print("fused vs stock torch.optim after the first step, worst parameter distance:", worst, "losses (before, after):", losses)
    assert worst[0] < 1e-5, worst
    (f0, f1), (s0, s1) = losses["fused"], losses["stock"]
    assert abs(f1 - f0) > 1e-3 * abs(f0) and abs(f1 - s1) <= 1e-3 * abs(s1), losses
