"""Gradient-norm clipping on the device, in the step: the norm pass over a chunk table (vbg_grad_sumsq_seg) and its finish (vbg_clip_coef)
against fp64 and the fp32 restatement of tests/test_clip_step_host.py; the two clipping step entries (vbg_sgd_step_seg_clip /
vbg_adam_step_seg_clip) bit for bit against *_seg_opt on gradients that torch unscaled and clipped beforehand, and against the fp64
restatements of tests/test_stock_optim_host.py; and `vbg.optim.clip_in_step` end to end -- FusedSGD / FusedAdamW against the existing
two-pass path bit for bit, fuse()d torch.optim objects against fp64 torch twins, the GradScaler loop without an unscale_ call, and
torch's sync-debug mode around it.  Shapes, option tables and the tolerance `close(..., 1e-6, 1e-7)` are those of the neighbouring
optimizer tests.  Needs a real MI355X."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_clip_step_host import coef_ref
from test_gpu_optim_groups import ADAMW_KW, CHUNK, RUNS, SGD_B, SGD_HP, SGD_KW, TOTAL, _grads, _same, _set_grads, cut, dev, inside
from test_gpu_small_kernels import _opt_inputs, bits, close, rnd
from test_gpu_stock_optim import ADAM_OPT, AMS_SCALES, FIRST, SGD_OPT, _give, _pair, _state_equal, group_mask
from test_gpu_stock_optim_amp import _adam_state, _amp_pair, _sgd_state, scalars
from test_optim_groups_host import LAYOUT, six_params, split
from test_stock_optim_host import adam_opt_ref, sgd_opt_ref

COEF = 0.37


@pytest.fixture(scope="module")
def ops():
    from vbg import ops as _ops
    return _ops


def _norm(ops, g, rows, total, max_norm=1.0, **kw):
    """the two launches on a partials slice with canaries on both sides -> (partials, out, canaries intact)"""
    n = len(rows)
    table = ops.chunk_table(rows, max(r[2] for r in rows) + 1, total, dev())
    buf = torch.full((n + 16,), 777.0, device=dev())
    part = buf[8:8 + n]
    ops.grad_sumsq_seg(g, table, part)
    out = ops.clip_coef(part, n, max_norm, **kw)
    return part.clone(), out, bool((buf[:8] == 777.0).all()) and bool((buf[8 + n:] == 777.0).all())


# ------------------------------------------------------------------------------------------
# the norm pass and its finish
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [CHUNK, 4096])
def test_norm_over_the_runs(ops, chunk):
    """4376 elements, rows of 4 ... 64 elements (chunk 64) or one row of 4096 among short ones; NaN and 1e30 sit everywhere no row covers"""
    m = inside(RUNS, TOTAL)
    g0 = rnd(TOTAL, seed=140)
    canary = torch.where(torch.arange(TOTAL) % 2 == 0, torch.full((), float("nan")), torch.full((), 1e30))
    g0 = torch.where(m, g0, canary)
    rows = cut(RUNS, chunk)
    assert max(r[1] for r in rows) == chunk and min(r[1] for r in rows) == 8
    g = g0.to(dev())
    part, out, intact = _norm(ops, g, rows, TOTAL)
    ref = float(g0.double()[m].norm())
    total = float(out[0])
    print(f"chunk {chunk}: total {total!r} fp64 {ref!r} relative error {abs(total - ref) / ref:.3e}")
    assert np.isfinite(total) and abs(total - ref) <= 1e-6 * ref
    assert intact and torch.equal(bits(g), bits(g0))
    # a row's partial: at most 16 products and 16 + 6 + 4 additions deep, all terms positive -> 27 roundings of 2^-24 at the most
    rows_ref = torch.tensor([float((g0.double()[s:s + n] ** 2).sum()) for s, n, _ in rows], dtype=torch.float64)
    assert close(part, rows_ref, 27 * 2.0 ** -24, 0.0)
    t, c = coef_ref(total, 1.0)
    assert bits(out).tolist() == bits(torch.tensor([float(t), float(c)], dtype=torch.float32)).tolist() and 0 < c < 1
    # the same bits on a second call, and with deterministic mode on (the same code runs)
    part2, out2, _ = _norm(ops, g, rows, TOTAL)
    with ops.deterministic_scope(True):
        part3, out3, _ = _norm(ops, g, rows, TOTAL)
    for p_, o_ in ((part2, out2), (part3, out3)):
        assert torch.equal(bits(p_), bits(part)) and torch.equal(bits(o_), bits(out))


def test_row_walk_past_the_grid_cap(ops):
    """3137 rows: more than the 2048 blocks of the grid (blocks on their second row exist) and more partials than the finish has threads"""
    n = 200704
    rows = cut([(0, n, 0), (n, 8, 1)], CHUNK)
    assert len(rows) == 3137
    g0 = rnd(n + 8, seed=141)
    g = g0.to(dev())
    part, out, intact = _norm(ops, g, rows, n + 8)
    ref = float(g0.double().norm())
    total = float(out[0])
    print(f"3137 rows: total {total!r} fp64 {ref!r} relative error {abs(total - ref) / ref:.3e}")
    assert intact and abs(total - ref) <= 1e-6 * ref
    rows_ref = (g0.double() ** 2)[:n].view(-1, CHUNK).sum(1)
    assert close(part[:-1], rows_ref, 27 * 2.0 ** -24, 0.0) and close(part[-1:], (g0.double()[n:] ** 2).sum().view(1), 27 * 2.0 ** -24, 0.0)
    part2, out2, _ = _norm(ops, g, rows, n + 8)
    assert torch.equal(bits(part2), bits(part)) and torch.equal(bits(out2), bits(out))


def test_finish_on_hand_made_partials(ops):
    d = dev()
    some = torch.ones(5, device=d)
    assert ops.clip_coef(some, 0, 2.0).tolist() == [0.0, 1.0]                          # n == 0: nothing is read
    out = ops.clip_coef(torch.tensor([1.0, float("inf"), 3.0], device=d), 3, 2.0)
    assert out.tolist() == [float("inf"), 0.0]
    out = ops.clip_coef(torch.tensor([1.0, float("nan"), 3.0], device=d), 3, 2.0)
    assert bool(torch.isnan(out).all())
    # 700 integer partials (more than the block has threads; their sum is exact in double in any order) against the restatement
    part = torch.randint(0, 1000, (700,), generator=torch.Generator().manual_seed(7)).float()
    root = np.float32(np.sqrt(float(part.double().sum())))
    for max_norm, norm_scale, scale in ((2.0, 1.0, None), (1e4, 1.0, None), (2.0, 0.5, None), (0.37, 1.0, 1024.0), (0.37, 1.0, 1000.0), (0.13, 0.5, 1000.0)):
        sc = None if scale is None else torch.full((), scale, device=d)
        out = ops.clip_coef(part.to(d), 700, max_norm, norm_scale, sc)
        t, c = coef_ref(root, max_norm, norm_scale, scale)
        assert bits(out).tolist() == bits(torch.tensor([float(t), float(c)], dtype=torch.float32)).tolist(), (max_norm, norm_scale, scale, out.tolist(), float(t), float(c))
        assert (c == 1.0) == (max_norm == 1e4)
    out = torch.full((4,), 5.0, device=d)                                              # a caller's own output: two elements written
    ops.clip_coef(part.to(d)[:300], 300, 2.0, out=out)
    assert out[2:].tolist() == [5.0, 5.0] and float(out[0]) == float(np.float32(np.sqrt(float(part[:300].double().sum()))))


# ------------------------------------------------------------------------------------------
# the step entries
# ------------------------------------------------------------------------------------------
def _coef(value=COEF):
    c = torch.full((1,), value, device=dev())
    return c, c.cpu().reshape(())


@pytest.mark.parametrize("scale", [1024.0, 1000.0])
def test_sgd_step_seg_clip(ops, scale):
    p0, grads = _opt_inputs(TOTAL, steps=4)
    mom0 = _sgd_state(grads)
    table = ops.chunk_table(cut(RUNS, CHUNK), 3, TOTAL, dev())
    sc, fi, inv = scalars(scale)
    cd, ch = _coef()
    p, mom = p0.to(dev()), mom0.to(dev())
    q, qmom = p0.to(dev()), mom0.to(dev())          # vbg_sgd_step_seg_opt on gradients unscaled and clipped beforehand
    pr, mr = p0.double(), mom0.double()
    m, mm = inside(RUNS, TOTAL), group_mask(RUNS, TOTAL, (0, 1))
    for i, g in enumerate(grads):
        g0 = g * scale
        gd = g0.to(dev())
        hp = [h[:4] + (h[4] | (FIRST if k == 1 and i == 0 else 0),) for k, h in enumerate(SGD_OPT)]
        ops.sgd_step_seg_clip(p, gd, mom, table, hp, sc, fi, cd)
        want = (g0 * inv) * ch                      # torch, fp32: two products, each rounded
        assert torch.equal(bits(gd)[m], bits(want)[m]) and torch.equal(bits(gd)[~m], bits(g0)[~m])
        ops.sgd_step_seg_opt(q, want.to(dev()), qmom, table, hp, 1.0)
        assert torch.equal(bits(p), bits(q)) and torch.equal(bits(mom), bits(qmom)), i
        for s, n, k in RUNS:
            pr[s:s + n], mr[s:s + n] = sgd_opt_ref(pr[s:s + n], g0.double()[s:s + n], mr[s:s + n], *hp[k], float(inv) * float(ch))
    assert close(p.cpu()[m], pr[m], 1e-6, 1e-7) and close(mom.cpu()[mm], mr[mm], 1e-6, 1e-7)
    assert not torch.equal(p.cpu()[m], p0[m]) and not torch.equal(mom.cpu()[mm], mom0[mm])
    assert torch.equal(bits(p)[~m], bits(p0)[~m]) and torch.equal(bits(mom)[~mm], bits(mom0)[~mm])


@pytest.mark.parametrize("scale", [1024.0, 1000.0])
def test_adam_step_seg_clip(ops, scale):
    p0, grads = _opt_inputs(TOTAL, steps=4)
    grads = [g * s for g, s in zip(grads, AMS_SCALES)]
    st0 = _adam_state(grads, ADAM_OPT)
    table = ops.chunk_table(cut(RUNS, CHUNK), 3, TOTAL, dev())
    sc, fi, inv = scalars(scale)
    cd, ch = _coef()
    a = [t.to(dev()) for t in [p0] + st0]
    b = [t.to(dev()) for t in [p0] + st0]
    ref = [t.double() for t in [p0] + st0]
    ins, ams = inside(RUNS, TOTAL), group_mask(RUNS, TOTAL, (0,))
    for i, g in enumerate(grads):
        g0 = g * scale
        gd = g0.to(dev())
        hp = [h[:5] + (h[5] + i, h[6]) for h in ADAM_OPT]
        ops.adam_step_seg_clip(a[0], gd, a[1], a[2], a[3], table, hp, sc, fi, cd)
        want = (g0 * inv) * ch
        assert torch.equal(bits(gd)[ins], bits(want)[ins]) and torch.equal(bits(gd)[~ins], bits(g0)[~ins])
        ops.adam_step_seg_opt(b[0], want.to(dev()), b[1], b[2], b[3], table, hp, 1.0)
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b)), i
        for s, n, k in RUNS:
            sl = slice(s, s + n)
            ref[0][sl], ref[1][sl], ref[2][sl], ref[3][sl] = adam_opt_ref(ref[0][sl], g0.double()[sl], ref[1][sl], ref[2][sl], ref[3][sl], *hp[k],
                                                                         float(inv) * float(ch))
    p, m, v, x = a
    assert close(p.cpu()[ins], ref[0][ins], 1e-6, 1e-7) and close(m.cpu()[ins], ref[1][ins], 1e-6, 1e-7) and close(v.cpu()[ins], ref[2][ins], 1e-6, 1e-7)
    assert close(x.cpu()[ams], ref[3][ams], 1e-6, 1e-7) and not torch.equal(p.cpu()[ins], p0[ins])
    for got, was in ((p, p0), (m, st0[0]), (v, st0[1])):
        assert torch.equal(bits(got)[~ins], bits(was)[~ins])
    assert torch.equal(bits(x)[~ams], bits(st0[2])[~ams])


@pytest.mark.parametrize("which", ["sgd", "adam"])
def test_coefficient_one_without_a_scale_is_the_opt_entry(ops, which):
    """coefficient exactly 1, no scale, no scaler (found_inf NULL): the bits of *_seg_opt, with its host scale, and g keeps its bits"""
    p0, grads = _opt_inputs(TOTAL, steps=3)
    st0 = [_sgd_state(grads)] if which == "sgd" else _adam_state(grads, ADAM_OPT)
    table = ops.chunk_table(cut(RUNS, CHUNK), 3, TOTAL, dev())
    one, _ = _coef(1.0)
    a, b = [t.to(dev()) for t in [p0] + st0], [t.to(dev()) for t in [p0] + st0]
    for i, g in enumerate(grads):
        gd = g.to(dev())
        if which == "sgd":
            hp = [h[:4] + (h[4] | (FIRST if k == 1 and i == 0 else 0),) for k, h in enumerate(SGD_OPT)]
            ops.sgd_step_seg_clip(a[0], gd, a[1], table, hp, None, None, one, 0.125)
            ops.sgd_step_seg_opt(b[0], gd, b[1], table, hp, 0.125)
        else:
            hp = [h[:5] + (h[5] + i, h[6]) for h in ADAM_OPT]
            ops.adam_step_seg_clip(a[0], gd, a[1], a[2], a[3], table, hp, None, None, one, 0.125)
            ops.adam_step_seg_opt(b[0], gd, b[1], b[2], b[3], table, hp, 0.125)
        assert torch.equal(bits(gd), bits(g))
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b)), (which, i)
    assert not torch.equal(a[0].cpu(), p0)


def test_keep_mom_is_the_plain_segmented_sgd_step(ops):
    """what FusedSGD's clipping step relies on: with keep_mom the momentum-0 group writes its buffer, and every buffer carries the bits of
    vbg_sgd_step_seg on the gradient clipped beforehand (host scale 0.125 inside the rule on both sides)"""
    p0, grads = _opt_inputs(TOTAL, steps=3)
    table = ops.chunk_table(cut(RUNS, CHUNK), 3, TOTAL, dev())
    assert SGD_HP[2][1] == 0.0
    cd, ch = _coef()
    mom0 = rnd(TOTAL, seed=112)
    a, b = [p0.to(dev()), mom0.to(dev())], [p0.to(dev()), mom0.to(dev())]
    for i, g in enumerate(grads):
        gd = g.to(dev())
        hp = [(lr, mo, 0.0, wd, FIRST if i == 0 else 0) for lr, mo, wd in SGD_HP]
        ops.sgd_step_seg_clip(a[0], gd, a[1], table, hp, None, None, cd, 0.125, keep_mom=True)
        want = g * ch
        assert torch.equal(bits(gd)[inside(RUNS, TOTAL)], bits(want)[inside(RUNS, TOTAL)])
        ops.sgd_step_seg(b[0], want.to(dev()), b[1], table, SGD_HP, i == 0, 0.125)
        assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1])), i
    g2 = group_mask(RUNS, TOTAL, (2,))
    assert not torch.equal(a[1].cpu()[g2], mom0[g2])                                   # the momentum-0 group's buffer was written


@pytest.mark.parametrize("which,flag", [("sgd", 1.0), ("adam", 2.0)])
def test_found_inf_makes_the_clipping_launch_a_no_op(ops, which, flag):
    p0, grads = _opt_inputs(TOTAL, steps=1)
    g0 = grads[0] * 1024.0
    g0[300] = float("inf")
    sc, fi, _ = scalars(1024.0, flag)
    cd, _ = _coef(0.0)                                                                # (what an inf norm makes of the coefficient)
    table = ops.chunk_table(cut(RUNS, CHUNK), 3, TOTAL, dev())
    host = [p0, g0] + ([_sgd_state(grads)] if which == "sgd" else _adam_state(grads, ADAM_OPT))
    d = [t.to(dev()) for t in host]
    if which == "sgd":
        ops.sgd_step_seg_clip(d[0], d[1], d[2], table, SGD_OPT, sc, fi, cd)
    else:
        ops.adam_step_seg_clip(d[0], d[1], d[2], d[3], d[4], table, ADAM_OPT, sc, fi, cd)
    for got, was in zip(d, host):
        assert torch.equal(bits(got), bits(was))
    assert float(cd) == 0.0


# ------------------------------------------------------------------------------------------
# clip_in_step
# ------------------------------------------------------------------------------------------
def _flat_opts(segmented):
    from vbg import optim as vo
    n1, l1 = six_params(dev(), seed=3)
    n2, _ = six_params(dev(), seed=0)
    if segmented:
        return (n1, vo.FusedSGD(split(n1, l1, **SGD_B), dev(), seg_chunk=CHUNK, layout=n1, **SGD_KW)), (n2, vo.FusedAdamW(vo.decay_groups(n2), dev(), seg_chunk=CHUNK, **ADAMW_KW))
    return (n1, vo.FusedSGD(n1, dev(), **SGD_KW)), (n2, vo.FusedAdamW(n2, dev(), **ADAMW_KW))


@pytest.mark.parametrize("segmented", [False, True])
def test_fused_optimizers_against_the_two_pass_path(ops, segmented):
    """FusedSGD + FusedAdamW, one norm over both: clip_in_step + step() against twins that take the coefficient read back from the
    device through ops.scale_ and the plain step() -- parameters, state and .grad bit-equal over three steps, the last one not biting"""
    from vbg import optim as vo
    (na, sgd_a), (nb, adam_a) = _flat_opts(segmented)
    (nc, sgd_b), (nd, adam_b) = _flat_opts(segmented)
    assert sgd_a.segmented == segmented and adam_a.segmented == segmented
    g1, g2 = _grads(3, seed=305), _grads(3, seed=306)
    for step in range(3):
        norm = float(torch.cat([t.double().flatten() for t in list(g1[step].values()) + list(g2[step].values())]).norm())
        max_norm = 2.0 * norm if step == 2 else 0.5 * norm
        for named, grads in ((na, g1), (nb, g2), (nc, g1), (nd, g2)):
            _set_grads(named, grads[step])
        total = vo.clip_in_step([sgd_a, adam_a], max_norm)
        coef = sgd_a._vbg_clip
        sgd_a.step()
        adam_a.step()
        assert sgd_a._vbg_clip is None and adam_a._vbg_clip is None
        ref = vo.clip_grad_norm_([sgd_b, adam_b], 1e30)                              # (never bites: the existing path's norm)
        assert abs(float(total) - ref) <= 1e-6 * ref and abs(float(total) - norm) <= 1e-6 * norm
        c = float(coef)
        assert (c == 1.0) == (step == 2) and _c_is(total, max_norm, c)
        if c != 1.0:
            ops.scale_(sgd_b.group.gflat, c)
            ops.scale_(adam_b.group.gflat, c)
        sgd_b.step()
        adam_b.step()
        pairs = [(sgd_a.group.pflat, sgd_b.group.pflat), (sgd_a.group.gflat, sgd_b.group.gflat), (sgd_a.mom, sgd_b.mom),
                 (adam_a.group.pflat, adam_b.group.pflat), (adam_a.group.gflat, adam_b.group.gflat), (adam_a.m, adam_b.m), (adam_a.v, adam_b.v)]
        for k, (x, y) in enumerate(pairs):
            assert torch.equal(bits(x), bits(y)), (step, k)
    assert sgd_a.steps == 3 and adam_a.steps == 3 and bool(sgd_a.mom.any()) and bool(adam_a.v.any())


def _c_is(total, max_norm, c):
    """the coefficient the device left is the restatement's for the total it returned"""
    return bits(torch.tensor(c)).item() == bits(torch.tensor(float(coef_ref(float(total), max_norm)[1]))).item()


@pytest.mark.parametrize("config", ["sgd_nesterov", "adamw_amsgrad"])
def test_fused_stock_optimizers_against_fp64_twins(config):
    """fuse()d torch.optim objects, head.weight's .grad None in every step: the fp64 twin multiplies its gradients by the coefficient the
    device computed (torch's clip with that factor substituted) and steps"""
    from vbg import optim as vo
    named, twin, opt, topt, group = _pair(config)
    who = "head.weight"
    p_who = dict(named)[who]
    before = p_who.detach().clone()
    for step, grads in enumerate(_grads(3, seed=312)):
        _give(named, twin, group, grads, absent=(who,))
        norm = float(torch.cat([t.double().flatten() for n, t in grads.items() if n != who]).norm())
        max_norm = 0.5 * norm
        total = vo.clip_in_step([opt], max_norm)
        coef = opt._vbg_clip
        opt.step()
        c = float(coef)
        assert abs(float(total) - norm) <= 1e-6 * norm and 0.49 < c < 0.51 and _c_is(total, max_norm, c)
        for n, q in twin:
            if q.grad is not None:
                q.grad.mul_(c)
        topt.step()
        assert _same(named, twin, f"after step {step + 1}") and _state_equal(named, twin, opt, topt)
        for (n, p), (_, q) in zip(named, twin):                                      # .grad holds the clipped gradient, as torch leaves it
            assert (p.grad is None) == (n == who) and (n == who or close(p.grad, q.grad, 1e-6, 1e-7))
    fs = opt._vbg_fused
    assert (fs.launches, fs.fallbacks) == (3, 0), fs.last_fallback
    assert torch.equal(bits(p_who), bits(before)) and p_who not in opt.state


@pytest.mark.parametrize("config", ["sgd_nesterov", "adamw_amsgrad"])
def test_gradscaler_loop_without_unscale(config):
    """scale(loss).backward(); clip_in_step(scaler=...); scaler.step(opt); scaler.update() -- no unscale_ -- with an inf planted in step two"""
    from vbg import optim as vo
    named, twin, opt, topt, group = _amp_pair(config, True)
    w = {n: rnd(*s, seed=400 + i) for i, (n, s, _) in enumerate(LAYOUT)}
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0, growth_interval=2)
    scales = []
    for step in range(3):
        group.zero_grad()
        scaler.scale(sum(((p * w[n].to(dev())) ** 2).sum() for n, p in named)).backward()
        assert all(p.grad is gv for p, gv in zip(group.params, group.gviews))
        if step == 1:
            named[2][1].grad.view(-1)[3] = float("inf")
        scale = scaler.get_scale()
        scaled, p_before = group.gflat.clone(), group.pflat.clone()
        total = vo.clip_in_step([opt], 1.0, scaler=scaler)
        scaler.step(opt)
        scaler.update()
        opt._vbg_fused.reconcile()
        scales.append(scaler.get_scale())
        if step == 1:                                                               # skipped: nothing moved, .grad as backward wrote it
            assert torch.equal(bits(group.pflat), bits(p_before)) and torch.equal(bits(group.gflat), bits(scaled))
            assert float(total) == float("inf")
        else:
            unscaled = float((scaled.double() / scale).norm())
            assert unscaled > 1.0 and abs(float(total) - unscaled) <= 1e-6 * unscaled
            assert abs(float(group.gflat.double().norm()) - 1.0) < 1e-3             # the clip did bite
            assert not torch.equal(bits(group.pflat), bits(p_before))
    assert scales == [1024.0, 512.0, 512.0]
    fs = opt._vbg_fused
    assert (fs.launches, fs.fallbacks, fs.skipped) == (3, 0, 1), fs.last_fallback
    assert opt._vbg_clip is None


def test_no_host_sync_from_backward_to_update():
    """torch's sync-debug mode around clip_in_step(...); scaler.step(opt); scaler.update() on a second step (tables and buffers belong to
    the first): nothing waits for the device.  clip_grad_norm_ in the same place does (its acc.item())"""
    from vbg import optim as vo
    w = {n: rnd(*s, seed=400 + i) for i, (n, s, _) in enumerate(LAYOUT)}
    named, twin, opt, topt, group = _amp_pair("adamw_amsgrad", True)
    (nf, fused), _ = _flat_opts(False)
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0)
    raised = None
    for step in range(2):
        group.zero_grad()
        scaler.scale(sum(((p * w[n].to(dev())) ** 2).sum() for n, p in named)).backward()
        _set_grads(nf, _grads(1, seed=307)[0])
        torch.cuda.synchronize()
        if step == 1:
            torch.cuda.set_sync_debug_mode("error")
        try:
            total = vo.clip_in_step([opt], 1.0, scaler=scaler)
            scaler.step(opt)
            scaler.update()
            vo.clip_in_step([fused], 1.0)                                            # (unscaled gradients of its own: a norm of its own)
            fused.step()
        except RuntimeError as e:
            raised = str(e)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert raised is None, raised
    assert total.is_cuda and total.dim() == 0 and float(total) > 0
    assert (opt._vbg_fused.launches, opt._vbg_fused.fallbacks) == (2, 0) and fused.steps == 2
    _set_grads(nf, _grads(1, seed=307)[0])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError, match="synchroniz"):
            vo.clip_grad_norm_([fused], 1.0)
    finally:
        torch.cuda.set_sync_debug_mode("default")
