"""Param groups of the fused optimizers on the GPU: the segmented entries (csrc/optim.hip vbg_sgd_step_seg / vbg_adamw_step_seg) on
canary-filled buffers against the fp64 restatements of tests/test_gpu_small_kernels.py, the grid-stride over more chunk rows than
the grid has blocks, bit-equality with the whole-range entries, and FusedSGD / FusedAdamW with several torch param groups against
torch.optim in fp64 -- schedulers, checkpoints in both directions, clip_grad_norm_, a GradScaler step.  Every tolerance is that
file's `close(..., 1e-6, 1e-7)`.  Needs a real MI355X."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_small_kernels import _opt_inputs, adamw_ref, bits, close, f32, gen, rnd, sgd_ref
from test_optim_groups_host import LAYOUT, split, six_params

CHUNK = 64
# runs (start, length, group): lengths 8, 8, 56, 64, 72, 8, 4104 alternating between three groups; gaps of 8, 16 and 8 elements
# between some of them, 24 untouched elements at the end
RUNS = [(0, 8, 0), (8, 8, 1), (24, 56, 2), (80, 64, 0), (160, 72, 1), (232, 8, 2), (248, 4104, 0)]
TOTAL = 248 + 4104 + 24
SGD_HP = [(f32(0.005), f32(0.9), f32(0.005)), (f32(0.02), f32(0.5), f32(0.0)), (f32(0.001), f32(0.0), f32(0.05))]          # lr, momentum, wd
ADAMW_HP = [(f32(1e-3), f32(0.9), f32(0.999), f32(1e-8), f32(0.01)), (f32(3e-4), f32(0.8), f32(0.99), f32(1e-6), f32(0.0)),
            (f32(2e-3), f32(0.95), f32(0.9995), f32(1e-7), f32(0.1))]                                                       # lr, b1, b2, eps, wd


@pytest.fixture(scope="module")
def ops():
    from vbg import ops as _ops
    return _ops


def dev():
    return torch.device("cuda")


def cut(runs, chunk):
    return [(s, min(chunk, start + n - s), k) for start, n, k in runs for s in range(start, start + n, chunk)]


def inside(runs, total):
    m = torch.zeros(total, dtype=torch.bool)
    for s, n, _ in runs:
        m[s:s + n] = True
    return m


def test_the_long_run_spans_65_chunks():
    rows = cut(RUNS, CHUNK)
    assert len([r for r in rows if r[0] >= 248]) == 65 and rows[-1] == (248 + 64 * 64, 8, 0) and len(rows) == 1 + 1 + 1 + 1 + 2 + 1 + 65


@pytest.mark.parametrize("gs", [1.0, 0.125])
def test_sgd_step_seg(ops, gs):
    p0, grads = _opt_inputs(TOTAL)
    mom0 = rnd(TOTAL, seed=112)                        # (first step: whatever the buffer holds in a run is overwritten)
    table = ops.chunk_table(cut(RUNS, CHUNK), 3, TOTAL, dev())
    p, mom = p0.to(dev()), mom0.to(dev())
    pr, mr = p0.double(), mom0.double()
    for i, g in enumerate(grads):
        gd = g.to(dev())
        ops.sgd_step_seg(p, gd, mom, table, SGD_HP, i == 0, gs)
        assert torch.equal(bits(gd), bits(g))          # g bit-unchanged everywhere
        for s, n, k in RUNS:
            pr[s:s + n], mr[s:s + n] = sgd_ref(pr[s:s + n], g.double()[s:s + n], mr[s:s + n], *SGD_HP[k], i == 0, gs)
    m = inside(RUNS, TOTAL)
    assert close(p.cpu()[m], pr[m], 1e-6, 1e-7) and close(mom.cpu()[m], mr[m], 1e-6, 1e-7)
    assert not torch.equal(p.cpu()[m], p0[m])
    assert torch.equal(bits(p)[~m], bits(p0)[~m]) and torch.equal(bits(mom)[~m], bits(mom0)[~m])          # outside the runs: untouched


@pytest.mark.parametrize("gs,step0", [(1.0, 1), (0.125, 1), (1.0, 1000)])
def test_adamw_step_seg(ops, gs, step0):
    p0, grads = _opt_inputs(TOTAL)
    m0, v0 = rnd(TOTAL, seed=115) * 0.01, 1e-3 * (0.1 + torch.rand(TOTAL, generator=gen(116)))           # canaries outside the runs
    ins = inside(RUNS, TOTAL)
    if step0 > 1:                                      # a late step on given moments: bias corrections far from their first values
        m0 = torch.where(ins, grads[0] * 0.1 * (0.5 + torch.rand(TOTAL, generator=gen(113))), m0)
    else:
        m0, v0 = torch.where(ins, torch.zeros(()), m0), torch.where(ins, torch.zeros(()), v0)
    table = ops.chunk_table(cut(RUNS, CHUNK), 3, TOTAL, dev())
    p, m, v = p0.to(dev()), m0.to(dev()), v0.to(dev())
    pr, mr, vr = p0.double(), m0.double(), v0.double()
    for i, g in enumerate(grads):
        gd = g.to(dev())
        ops.adamw_step_seg(p, gd, m, v, table, ADAMW_HP, step0 + i, gs)
        assert torch.equal(bits(gd), bits(g))
        for s, n, k in RUNS:
            pr[s:s + n], mr[s:s + n], vr[s:s + n] = adamw_ref(pr[s:s + n], g.double()[s:s + n], mr[s:s + n], vr[s:s + n], *ADAMW_HP[k], step0 + i, gs)
    assert close(p.cpu()[ins], pr[ins], 1e-6, 1e-7) and close(m.cpu()[ins], mr[ins], 1e-6, 1e-7) and close(v.cpu()[ins], vr[ins], 1e-6, 1e-7)
    assert not torch.equal(p.cpu()[ins], p0[ins])
    for got, was in ((p, p0), (m, m0), (v, v0)):
        assert torch.equal(bits(got)[~ins], bits(was)[~ins])


@pytest.mark.parametrize("which", ["sgd", "adamw"])
def test_more_chunk_rows_than_blocks(ops, which):
    """200 704 elements in 64-element rows: 3136 rows for a grid capped at 2048 blocks, then a second group on a trailing 8-element run"""
    n = 200704
    runs = [(0, n, 0), (n, 8, 1)]
    rows = cut(runs, CHUNK)
    assert len(rows) == 3136 + 1 and n + 8 < 1 << 20
    table = ops.chunk_table(rows, 2, n + 8, dev())
    p0, grads = _opt_inputs(n + 8)
    pr = p0.double()
    p = p0.to(dev())
    if which == "sgd":
        mom, mr = torch.zeros(n + 8, device=dev()), torch.zeros(n + 8, dtype=torch.float64)
    else:
        m, v = torch.zeros(n + 8, device=dev()), torch.zeros(n + 8, device=dev())
        mr, vr = torch.zeros(n + 8, dtype=torch.float64), torch.zeros(n + 8, dtype=torch.float64)
    for i, g in enumerate(grads):
        gd = g.to(dev())
        for s, k_n, k in runs:
            sl = slice(s, s + k_n)
            if which == "sgd":
                pr[sl], mr[sl] = sgd_ref(pr[sl], g.double()[sl], mr[sl], *SGD_HP[k], i == 0, 1.0)
            else:
                pr[sl], mr[sl], vr[sl] = adamw_ref(pr[sl], g.double()[sl], mr[sl], vr[sl], *ADAMW_HP[k], i + 1, 1.0)
        if which == "sgd":
            ops.sgd_step_seg(p, gd, mom, table, SGD_HP[:2], i == 0)
        else:
            ops.adamw_step_seg(p, gd, m, v, table, ADAMW_HP[:2], i + 1)
    assert close(p, pr, 1e-6, 1e-7)
    if which == "sgd":
        assert close(mom, mr, 1e-6, 1e-7)
    else:
        assert close(m, mr, 1e-6, 1e-7) and close(v, vr, 1e-6, 1e-7)


@pytest.mark.parametrize("which", ["sgd", "adamw", "sgd_momentum0"])
def test_same_bits_as_the_whole_range_launch(ops, which):
    """three groups with identical hyper-parameters over contiguous runs tiling 4096 elements == ops.sgd_step / ops.adamw_step, bit for
    bit: both kernels inline one statement of the update.  sgd_momentum0: a momentum-0 group of ops.sgd_step_seg still goes through
    that statement, in p AND in the momentum buffer it writes"""
    n = 4096
    runs = [(0, 1000, 0), (1000, 72, 1), (1072, n - 1072, 2)]
    table = ops.chunk_table(cut(runs, CHUNK), 3, n, dev())
    p0, grads = _opt_inputs(n)
    sgd_hp = SGD_HP[2] if which == "sgd_momentum0" else SGD_HP[0]
    assert (sgd_hp[1] == 0) == (which == "sgd_momentum0")
    a = [p0.to(dev())] + [torch.zeros(n, device=dev()) for _ in range(2 if which == "adamw" else 1)]
    b = [t.clone() for t in a]
    for gs in (1.0, 0.125):
        for i, g in enumerate(grads):
            gd = g.to(dev())
            if which == "adamw":
                ops.adamw_step_seg(a[0], gd, a[1], a[2], table, [ADAMW_HP[0]] * 3, i + 1, gs)
                ops.adamw_step(b[0], gd, b[1], b[2], *ADAMW_HP[0], i + 1, gs)
            else:
                ops.sgd_step_seg(a[0], gd, a[1], table, [sgd_hp] * 3, i == 0, gs)
                ops.sgd_step(b[0], gd, b[1], *sgd_hp, i == 0, gs)
            for x, y in zip(a, b):
                assert torch.equal(x, y), (which, gs, i)
    assert not torch.equal(a[0].cpu(), p0) and bool(a[1].any())


# ------------------------------------------------------------------------------------------
# optimizer level: the six parameters of the host test (groups A B A A B A over the flat layout)
# ------------------------------------------------------------------------------------------
def _grads(steps, seed=300):
    """per parameter, gradients that keep their sign over the steps (as _opt_inputs: the moment sums do not cancel)"""
    g = gen(seed)
    out = []
    sign = {n: (torch.randint(0, 2, s, generator=g).float() * 2 - 1) * (0.5 + 1.5 * torch.rand(*s, generator=g)) for n, s, _ in LAYOUT}
    for _ in range(steps):
        out.append({n: sign[n] * (0.5 + torch.rand(*s, generator=g)) for n, s, _ in LAYOUT})
    return out


def _twin(named, dtype):
    """CPU copies of a registration-order list, as leaves of `dtype`"""
    return [(n, torch.nn.Parameter(p.detach().cpu().to(dtype).clone())) for n, p in named]


def _set_grads(named, grads):
    for n, p in named:
        if p.grad is None:
            p.grad = torch.zeros_like(p)
        p.grad.copy_(grads[n].to(p.grad.dtype))


def _same(named, twin, what=""):
    return all(close(p, q, 1e-6, 1e-7) or print("parameter", n, what) for (n, p), (_, q) in zip(named, twin))


def _state_same(opt, topt, twin, keys):
    ok = True
    for n, q in twin:
        i = opt.group.names.index(n)
        for k in keys:
            ok = ok and (close(opt.group.view(opt._flat_state()[k], i), topt.state[q][k], 1e-6, 1e-7) or print("state", k, n))
    return bool(ok)


ADAMW_KW = dict(lr=f32(1e-3), betas=(f32(0.9), f32(0.999)), eps=f32(1e-8), weight_decay=f32(0.01))
LAMBDAS = [lambda e: 0.5 ** e, lambda e: 1.0 / (1 + e)]
SGD_KW = dict(lr=f32(0.005), momentum=f32(0.9), weight_decay=f32(0.005))
SGD_B = dict(lr=f32(0.02), momentum=f32(0.5), weight_decay=f32(0.0))


def _adamw_pair(dtype, seed=0):
    from vbg import optim as vo
    named, letters = six_params(dev(), seed=seed)
    twin = _twin(named, dtype)
    opt = vo.FusedAdamW(vo.decay_groups(named), dev(), seg_chunk=CHUNK, **ADAMW_KW)
    groups_t = [{"params": [q for n, q in twin if letters[n] == "A"]}, {"params": [q for n, q in twin if letters[n] == "B"], "weight_decay": 0.0}]
    topt = torch.optim.AdamW(groups_t, **ADAMW_KW)
    assert opt.segmented and len(opt.param_groups) == 2 and opt.group.names == [n for n, _, _ in LAYOUT]
    return named, twin, opt, topt


def _sgd_pair(dtype, seed=0):
    from vbg import optim as vo
    named, letters = six_params(dev(), seed=seed)
    twin = _twin(named, dtype)
    opt = vo.FusedSGD(split(named, letters, **SGD_B), dev(), seg_chunk=CHUNK, layout=named, **SGD_KW)
    topt = torch.optim.SGD([{"params": [q for n, q in twin if letters[n] == "A"]}, {"params": [q for n, q in twin if letters[n] == "B"], **SGD_B}], **SGD_KW)
    assert opt.segmented and opt.group.names == [n for n, _, _ in LAYOUT]
    return named, twin, opt, topt


def test_fused_adamw_decay_groups_and_lambda_lr():
    named, twin, opt, topt = _adamw_pair(torch.float64)
    sched, tsched = (torch.optim.lr_scheduler.LambdaLR(o, LAMBDAS) for o in (opt, topt))
    tail = {"p": (opt.group.pflat, 5.0), "m": (opt.m, 7.0), "v": (opt.v, 3.0)}          # [end of the last slot, total): no chunk covers it
    for buf, canary in tail.values():
        buf[4712:] = canary
    for step, grads in enumerate(_grads(4)):
        opt.zero_grad()
        _set_grads(named, grads)
        _set_grads(twin, grads)
        opt.step()
        topt.step()
        sched.step()
        tsched.step()
        assert [g["lr"] for g in opt.param_groups] == [g["lr"] for g in topt.param_groups]
        assert _same(named, twin, f"after step {step + 1}")
    assert opt.param_groups[0]["lr"] != opt.param_groups[1]["lr"] and opt.steps == 4
    assert _state_same(opt, topt, twin, ("exp_avg", "exp_avg_sq"))
    assert opt.group.total == 4736 and all(bool((buf[4712:] == canary).all()) for buf, canary in tail.values())


def test_fused_sgd_two_groups():
    named, twin, opt, topt = _sgd_pair(torch.float64)
    for step, grads in enumerate(_grads(4, seed=301)):
        opt.zero_grad()
        _set_grads(named, grads)
        _set_grads(twin, grads)
        if step == 2:                                  # a per-step weight-decay schedule, written the way the reference's loop writes it
            for o in (opt, topt):
                o.param_groups[0]["weight_decay"] = f32(0.01)
        opt.step()
        topt.step()
        assert _same(named, twin, f"after step {step + 1}")
    assert _state_same(opt, topt, twin, ("momentum_buffer",))


@pytest.mark.parametrize("which", ["sgd", "adamw"])
@pytest.mark.parametrize("direction", ["fused_to_torch", "torch_to_fused"])
def test_checkpoint_interchange(which, direction):
    """two steps on one side, its state_dict() loaded into the other side's optimizer over the same groups (fp32 twin, its parameters set
    to the stepped values), then one more step with the same gradient on both"""
    pair = _sgd_pair if which == "sgd" else _adamw_pair
    named, twin, opt, topt = pair(torch.float32)
    grads = _grads(3, seed=302)
    src_named, src_opt = (named, opt) if direction == "fused_to_torch" else (twin, topt)
    for g in grads[:2]:
        _set_grads(src_named, g)
        src_opt.param_groups[1]["lr"] *= 0.75          # what a scheduler changes travels with the checkpoint
        src_opt.step()
    sd = src_opt.state_dict()
    assert [g["params"] for g in sd["param_groups"]] == [[0, 1, 2, 3], [4, 5]] and sorted(sd["state"]) == list(range(6))
    if direction == "fused_to_torch":
        topt.load_state_dict(sd)
        with torch.no_grad():
            for (_, p), (_, q) in zip(named, twin):
                q.copy_(p.cpu())
    else:
        opt.load_state_dict(sd)
        with torch.no_grad():
            for (_, p), (_, q) in zip(named, twin):
                p.copy_(q.to(dev()))
    assert [g["lr"] for g in opt.param_groups] == [g["lr"] for g in topt.param_groups] and opt.param_groups[1]["lr"] != opt.param_groups[0]["lr"]
    before = [p.detach().clone() for _, p in named]
    _set_grads(named, grads[2])
    _set_grads(twin, grads[2])
    opt.step()
    topt.step()
    assert _same(named, twin, "after the step on the loaded state")
    assert _state_same(opt, topt, twin, ("momentum_buffer",) if which == "sgd" else ("exp_avg", "exp_avg_sq"))
    assert all(not torch.equal(b, p) for b, (_, p) in zip(before, named))


def test_clip_grad_norm_over_grouped_optimizers():
    from vbg import optim as vo
    named, _, opt, _ = _adamw_pair(torch.float64)
    named2, _, opt2, _ = _sgd_pair(torch.float64, seed=3)
    grads, grads2 = _grads(1, seed=303)[0], _grads(1, seed=304)[0]
    norm = float(torch.cat([g.double().flatten() for g in list(grads.values()) + list(grads2.values())]).norm())
    for max_norm in (0.5 * norm, 2.0 * norm):          # above the threshold (scaled) and below it (untouched)
        copies = []
        for nm, gr in ((named, grads), (named2, grads2)):
            _set_grads(nm, gr)
            for n, p in nm:
                c = torch.nn.Parameter(torch.zeros(p.shape, dtype=torch.float64))
                c.grad = gr[n].double().clone()
                copies.append((p, c))
        ref = float(torch.nn.utils.clip_grad_norm_([c for _, c in copies], max_norm))
        got = vo.clip_grad_norm_([opt, opt2], max_norm)
        assert abs(got - ref) <= 1e-6 * ref
        for p, c in copies:
            assert close(p.grad, c.grad, 1e-6, 1e-7)


def test_gradscaler_step_over_a_grouped_optimizer():
    """scale(loss).backward(), scaler.step(opt), scaler.update() as tests/test_gpu_train_loop.py takes them, on a quadratic loss: unscale_
    walks every param group's gradient views, the step is the segmented launch; the same loop on an fp64 twin with torch.optim"""
    named, twin, opt, topt = _adamw_pair(torch.float64)
    w = {n: rnd(*s, seed=400 + i) for i, (n, s, _) in enumerate(LAYOUT)}
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0, growth_interval=2)
    for step in range(3):
        opt.zero_grad()
        loss = sum(((p * w[n].to(dev())) ** 2).sum() for n, p in named)
        scaler.scale(loss).backward()
        if step == 0:
            assert all(p.grad is gv for p, gv in zip(opt.group.params, opt.group.gviews))          # the scaled gradients sit in the flat views
        scaler.step(opt)
        scaler.update()
        topt.zero_grad()
        sum(((q * w[n].double()) ** 2).sum() for n, q in twin).backward()
        topt.step()
    assert opt.steps == 3 and scaler.get_scale() == 2048.0
    # (1e-6 relative on the parameters as everywhere here: the gradient 2 w^2 p is formed in fp32 on the GPU, one rounding per operation,
    # and a relative gradient error of 2e-7 moves an AdamW update of ~lr = 1e-3 by 1e-10)
    assert _same(named, twin, "after three GradScaler steps")
