"""clip_in_step's loss gate and norm types 1 and inf on the device: the row pass (vbg_grad_norm_seg) against vbg_grad_sumsq_seg bit for
bit (kind 2), fp64 sums (kind 1) and exact maxima (kind 0), past the grid cap and with non-finite values planted at every place of the
walk; the finish (vbg_clip_coef_gate) against the fp32 restatement of tests/test_clip_gate_host.py; the gate with fp64 and fp32 losses --
open: the ungated bits, closed: (0, 1, 0) with the partials' canaries untouched; and `vbg.optim.clip_in_step(norm_type=..., when=...)`
end to end against twins driven by a host `if`, twins that never clip, fp64 torch twins, through a closure step and under torch's
sync-debug mode.  Shapes and the tolerance `close(..., 1e-6, 1e-7)` are those of tests/test_gpu_clip_step.py.  Needs a real MI355X."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

from test_clip_gate_host import INF, KINDS, finish_ref, gate_ref
from test_gpu_clip_step import _flat_opts
from test_gpu_optim_groups import CHUNK, RUNS, TOTAL, _grads, _same, _set_grads, cut, dev, inside
from test_gpu_small_kernels import bits, close, rnd
from test_gpu_stock_optim import _give, _pair, _state_equal

NAN = float("nan")
U = 2.0 ** -24
CANARY = 777.0


@pytest.fixture(scope="module")
def ops():
    from vbg import ops as _ops
    return _ops


def _canaried():
    """(g0, mask of the covered elements): random values in the runs, NaN and 1e30 everywhere no row covers"""
    m = inside(RUNS, TOTAL)
    canary = torch.where(torch.arange(TOTAL) % 2 == 0, torch.full((), NAN), torch.full((), 1e30))
    return torch.where(m, rnd(TOTAL, seed=140), canary), m


def _rows(ops, g, rows, total, kind, found_inf=None, gate=None):
    """the row launch on a partials slice with canaries on both sides -> (the slice's buffer, the slice, the table)"""
    n = len(rows)
    table = ops.chunk_table(rows, max(r[2] for r in rows) + 1, total, dev())
    buf = torch.full((n + 16,), CANARY, device=dev())
    part = buf[8:8 + n]
    ops.grad_norm_seg(g, table, part, kind, found_inf, gate)
    return buf, part, table


def _finish(ops, part, n, kind, max_norm=1.0, gate=None, **kw):
    """the finish into the middle of a canaried buffer -> (the three floats, canaries intact)"""
    buf = torch.full((9,), 5.0, device=dev())
    ops.clip_coef_gate(part, n, max_norm, kind=kind, gate=gate, out=buf[3:6], **kw)
    return buf[3:6].clone(), buf[:3].tolist() == [5.0] * 3 and buf[6:].tolist() == [5.0] * 3


def _norm(ops, g, rows, total, kind, found_inf=None, gate=None, max_norm=1.0):
    buf, part, _ = _rows(ops, g, rows, total, kind, found_inf, gate)
    n = len(rows)
    out, ok = _finish(ops, part, n, kind, max_norm, gate)
    return part.clone(), out, ok and bool((buf[:8] == CANARY).all()) and bool((buf[8 + n:] == CANARY).all())


def _row_refs(g0, rows, kind):
    """per row, in fp64 (kind 1) or exactly (kind 0)"""
    if kind == 1:
        return torch.tensor([float(g0.double()[s:s + n].abs().sum()) for s, n, _ in rows], dtype=torch.float64)
    return torch.stack([g0[s:s + n].abs().max() for s, n, _ in rows])


def _f3(*v):
    return bits(torch.tensor([float(x) for x in v], dtype=torch.float32)).tolist()


# ------------------------------------------------------------------------------------------
# the row pass and its finish
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [2, 1, 0])
@pytest.mark.parametrize("chunk", [CHUNK, 4096])
def test_rows_over_the_runs(ops, chunk, kind):
    """4376 elements, rows of 8 ... 64 elements (chunk 64) or one row of 4096 among short ones; NaN and 1e30 sit everywhere no row covers"""
    g0, m = _canaried()
    rows = cut(RUNS, chunk)
    assert max(r[1] for r in rows) == chunk and min(r[1] for r in rows) == 8
    g = g0.to(dev())
    part, out, intact = _norm(ops, g, rows, TOTAL, kind)
    assert intact and torch.equal(bits(g), bits(g0)) and float(out[2]) == 1.0
    total = float(out[0])
    if kind == 2:                                          # the bits of the existing pair
        table = ops.chunk_table(rows, 3, TOTAL, dev())
        old = ops.grad_sumsq_seg(g, table, torch.empty(len(rows), device=dev()))
        assert torch.equal(bits(part), bits(old))
        assert torch.equal(bits(out[:2]), bits(ops.clip_coef(old, len(rows), 1.0)))
    elif kind == 1:
        # a row's partial: at most 16 + 6 + 4 additions of positive terms (the absolute values add no rounding) -> 27 * 2^-24 at the most;
        # the total: that bound, the exact sum over rows in double, one rounding to fp32
        ref = _row_refs(g0, rows, 1)
        assert close(part, ref, 27 * U, 0.0)
        whole = float(g0.double()[m].abs().sum())
        print(f"chunk {chunk}: L1 total {total!r} fp64 {whole!r} relative error {abs(total - whole) / whole:.3e}")
        assert abs(total - whole) <= 28 * U * whole
    else:
        assert torch.equal(bits(part), bits(_row_refs(g0, rows, 0)))
        assert bits(out[:1]).item() == bits(g0[m].abs().max().view(1)).item()
    t, c, gate = finish_ref(part.cpu().numpy(), kind, 1.0)
    assert bits(out).tolist() == _f3(t, c, gate) and 0 < c < 1
    # the same bits on a second call, and with deterministic mode on (the same code runs)
    part2, out2, _ = _norm(ops, g, rows, TOTAL, kind)
    with ops.deterministic_scope(True):
        part3, out3, _ = _norm(ops, g, rows, TOTAL, kind)
    for p_, o_ in ((part2, out2), (part3, out3)):
        assert torch.equal(bits(p_), bits(part)) and torch.equal(bits(o_), bits(out))
    assert torch.equal(bits(g), bits(g0))


def test_row_walk_past_the_grid_cap(ops):
    """3137 rows: more than the 2048 blocks of the grid, so blocks on their second row exist -- the largest magnitude sits in such a row,
    in the last float4 a thread of that row reads, negative"""
    n = 200704
    rows = cut([(0, n, 0), (n, 8, 1)], CHUNK)
    assert len(rows) == 3137
    g0 = rnd(n + 8, seed=141)
    row = 2500
    at = rows[row][0] + rows[row][1] - 1
    assert row >= 2048 and at == 2500 * 64 + 63 and float(g0.abs().max()) < 50.0
    g0[at] = -123.4375
    g = g0.to(dev())
    part, out, intact = _norm(ops, g, rows, n + 8, 0)
    assert intact and float(out[0]) == 123.4375 and float(part[row]) == 123.4375
    assert torch.equal(bits(part[:-1]), bits(g0[:n].abs().view(-1, CHUNK).max(1).values)) and float(part[-1]) == float(g0[n:].abs().max())
    part, out, intact = _norm(ops, g, rows, n + 8, 1)
    whole = float(g0.double().abs().sum())
    total = float(out[0])
    print(f"3137 rows: L1 total {total!r} fp64 {whole!r} relative error {abs(total - whole) / whole:.3e}")
    assert intact and abs(total - whole) <= 28 * U * whole
    assert close(part[:-1], g0.double()[:n].abs().view(-1, CHUNK).sum(1), 27 * U, 0.0) and close(part[-1:], g0.double()[n:].abs().sum().view(1), 27 * U, 0.0)
    part2, out2, _ = _norm(ops, g, rows, n + 8, 1)
    assert torch.equal(bits(part2), bits(part)) and torch.equal(bits(out2), bits(out))
    part, out, intact = _norm(ops, g, rows, n + 8, 2)
    table = ops.chunk_table(rows, 2, n + 8, dev())
    assert intact and torch.equal(bits(part), bits(ops.grad_sumsq_seg(g, table, torch.empty(3137, device=dev()))))


@pytest.mark.parametrize("table", ["runs", "cap"])
def test_bits_of_the_recorded_calls(ops, golden, table):
    """every array of tests/golden/optim_bits.npz bit for bit: the calls of tests/golden/make_golden_optim_bits.py (both row-pass entries for
    squares, grad_norm_seg of every kind with and without the flag, clip_coef and clip_coef_gate over them), recorded by the commit before
    grad_sumsq_seg and clip_coef lost their own kernels; "cap" walks past the grid's 2048 blocks.  Canaries and g intact"""
    import make_golden_optim_bits as M
    fix = golden("optim_bits.npz")
    g0 = torch.from_numpy(fix[f"g_{table}"].view(np.float32).copy())
    cuts = sorted(k[len(f"rows_{table}_"):] for k in fix.files if k.startswith(f"rows_{table}_"))
    assert cuts == {"runs": ["4096", "64"], "cap": ["8"]}[table]
    for c in cuts:
        rows = [tuple(int(v) for v in r) for r in fix[f"rows_{table}_{c}"]]
        assert len(rows) == {"64": 72, "4096": 8, "8": 2051}[c] and (table != "cap" or len(rows) > 2048)
        got, intact = M.record(ops, dev(), g0, rows)
        assert intact, (table, c)
        want = {k[len(f"{table}_{c}_"):]: fix[k] for k in fix.files if k.startswith(f"{table}_{c}_")}
        assert sorted(want) == sorted(got) and len(want) == 10
        for k in sorted(want):
            assert torch.equal(torch.from_numpy(got[k].view(np.int32)), torch.from_numpy(want[k].view(np.int32))), (table, c, k)


PLACES = {"first": 0, "last": 248 + 4104 - 1, "middle": 2300, "gap": 20}


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_non_finite_values(ops, kind):
    """each of +inf, -inf and NaN at the first, the last and a middle covered element and in a gap no row covers (rows of 64 and the
    4096-element row): the total, the coefficient and GradScaler's flag"""
    base, m = _canaried()
    assert m[PLACES["first"]] and m[PLACES["last"]] and m[PLACES["middle"]] and not m[PLACES["gap"]] and not m[PLACES["last"] + 1]
    clean = {}
    for chunk in (CHUNK, 4096):
        rows = cut(RUNS, chunk)
        for value in (INF, -INF, NAN):
            for place, at in PLACES.items():
                g0 = base.clone()
                g0[at] = value
                flag = torch.zeros(1, device=dev())
                part, out, intact = _norm(ops, g0.to(dev()), rows, TOTAL, kind, found_inf=flag, max_norm=2.0)
                total, coef, gate = out.tolist()
                what = (kind, chunk, value, place, out.tolist())
                assert intact and gate == 1.0, what
                if place == "gap":                         # nothing: what no row covers is not read
                    assert np.isfinite(total) and 0 < coef <= 1 and float(flag) == 0.0, what
                    assert bits(out).tolist() == clean.setdefault(chunk, bits(out).tolist()), what
                elif value != value:
                    assert np.isnan(total) and np.isnan(coef) and float(flag) == 1.0, what
                else:
                    assert total == INF and coef == 0.0 and float(flag) == 1.0, what
                    if kind == 0:
                        assert int(torch.isinf(part).sum()) == 1 and float(part.max()) == INF, what          # -inf gives +inf
    # finite values whose squares overflow: an inf partial for kind 2 only, and no flag for any kind
    g0 = base.clone()
    g0[2300] = -3e30
    flag = torch.zeros(1, device=dev())
    part, out, _ = _norm(ops, g0.to(dev()), cut(RUNS, CHUNK), TOTAL, kind, found_inf=flag)
    assert float(flag) == 0.0 and (float(out[0]) == INF) == (kind == 2)
    if kind == 0:
        assert bits(out[:1]).item() == bits(torch.tensor([3e30])).item()


@pytest.mark.parametrize("kind", [2, 1, 0])
def test_finish_on_hand_made_partials(ops, kind):
    d = dev()
    some = torch.ones(5, device=d)
    out, ok = _finish(ops, some, 0, kind, 2.0)
    assert ok and out.tolist() == [0.0, 1.0, 1.0]                                      # n == 0: nothing is read; only three floats written
    out, ok = _finish(ops, torch.tensor([1.0, INF, 3.0], device=d), 3, kind, 2.0)
    assert ok and out.tolist() == [INF, 0.0, 1.0]
    out, ok = _finish(ops, torch.tensor([1.0, NAN, 3.0], device=d), 3, kind, 2.0)
    assert ok and bool(torch.isnan(out[:2]).all()) and float(out[2]) == 1.0
    out, ok = _finish(ops, torch.tensor([NAN] + [1.0] * 299 + [INF], device=d), 301, kind, 2.0)          # a NaN beats an inf, wherever it sits
    assert ok and bool(torch.isnan(out[:2]).all())
    # 700 integer partials (more than the block has threads; their sum is exact in double in any order) against the restatement
    part = torch.randint(0, 1000, (700,), generator=torch.Generator().manual_seed(7)).float()
    part[699 if kind == 0 else 5] = 1000.0                                             # (kind 0: the maximum where thread 187 reads last)
    for max_norm, norm_scale, scale in ((2.0, 1.0, None), (1e7, 1.0, None), (2.0, 0.5, None), (0.37, 1.0, 1024.0), (0.37, 1.0, 1000.0), (0.13, 0.5, 1000.0)):
        sc = None if scale is None else torch.full((), scale, device=d)
        out, ok = _finish(ops, part.to(d), 700, kind, max_norm, norm_scale=norm_scale, grad_scale=sc)
        t, c, gate = finish_ref(part.numpy(), kind, max_norm, norm_scale, scale)
        assert ok and bits(out).tolist() == _f3(t, c, gate), (kind, max_norm, norm_scale, scale, out.tolist(), float(t), float(c))
        assert (c == 1.0) == (max_norm == 1e7)
    out, ok = _finish(ops, part.to(d)[:300], 300, kind, 2.0)
    want = {2: np.sqrt(float(part[:300].double().sum())), 1: float(part[:300].double().sum()), 0: float(part[:300].max())}[kind]
    assert ok and float(out[0]) == float(np.float32(want))
    fresh = ops.clip_coef_gate(part.to(d), 700, 2.0, kind=kind)                        # the wrapper's own output: three floats
    assert fresh.shape == (3,) and float(fresh[2]) == 1.0


# ------------------------------------------------------------------------------------------
# the gate
# ------------------------------------------------------------------------------------------
def _loss(value, dtype):
    return torch.tensor([float(value)], dtype=torch.float64).to(dtype)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("kind", [2, 1, 0])
def test_gate_open_is_the_ungated_call_and_closed_touches_nothing(ops, dtype, kind):
    g0, m = _canaried()
    g = g0.to(dev())
    rows = cut(RUNS, CHUNK)
    n = len(rows)
    part0, out0, _ = _norm(ops, g, rows, TOTAL, kind)
    opened = (_loss(12.5, dtype).to(dev()), 10)
    part, out, intact = _norm(ops, g, rows, TOTAL, kind, gate=opened)
    assert intact and torch.equal(bits(part), bits(part0)) and torch.equal(bits(out), bits(out0)) and float(out[2]) == 1.0
    closed = (_loss(3.0, dtype).to(dev()), 10)
    part, out, intact = _norm(ops, g, rows, TOTAL, kind, gate=closed)
    assert intact and out.tolist() == [0.0, 1.0, 0.0]
    assert bool((part == CANARY).all())                                                # the early exit: no row wrote its partial
    # the finish reads no partial when the gate is closed: NaNs where they would be
    out, ok = _finish(ops, torch.full((n,), NAN, device=dev()), n, kind, gate=closed)
    assert ok and out.tolist() == [0.0, 1.0, 0.0]
    out, ok = _finish(ops, torch.full((n,), NAN, device=dev()), 0, kind, gate=closed)      # n == 0: (0, 1, gate)
    assert ok and out.tolist() == [0.0, 1.0, 0.0]
    # with GradScaler's flag the rows are walked whatever the gate says: the partials and the flag of the ungated call
    for plant in (None, -INF):
        gp = g0.clone()
        if plant is not None:
            gp[2300] = plant
        flag = torch.zeros(1, device=dev())
        part, out, intact = _norm(ops, gp.to(dev()), rows, TOTAL, kind, found_inf=flag, gate=closed)
        assert intact and out.tolist() == [0.0, 1.0, 0.0] and float(flag) == (0.0 if plant is None else 1.0)
        if plant is None:
            assert torch.equal(bits(part), bits(part0))
        else:
            assert not bool((part == CANARY).any())
    assert torch.equal(bits(g), bits(g0))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("threshold", [10, 0.1, float(np.float32(0.1))])
def test_gate_decision_on_the_device_is_torchs(ops, dtype, threshold):
    """the loss at the threshold, one ulp above and below it, NaN and +-inf: the third float of the finish and the rows' early exit
    against torch's own `loss > threshold` on the CPU (and against the restatement the host test pins to it)"""
    npdt = np.float64 if dtype == torch.float64 else np.float32
    at = npdt(threshold)
    g = rnd(64, seed=142).to(dev())
    rows = [(0, 64, 0)]
    values = [at, np.nextafter(at, npdt(np.inf)), np.nextafter(at, npdt(-np.inf)), npdt(NAN), npdt(INF), npdt(-INF), npdt(0.0), npdt(float(threshold) * 2)]
    got = []
    for v in values:
        loss = _loss(v, dtype)
        want = bool((loss > threshold).item())
        assert gate_ref(loss, threshold) == want
        part, out, intact = _norm(ops, g, rows, 64, 2, gate=(loss.to(dev()), threshold))
        assert intact and float(out[2]) == float(want), (dtype, threshold, float(v), out.tolist())
        assert bool((part == CANARY).all()) == (not want)
        got.append(want)
    assert got[1:6] == [True, False, False, True, False] and got[6:] == [False, True]
    assert got[0] is False or float(at) > float(threshold)


# ------------------------------------------------------------------------------------------
# clip_in_step
# ------------------------------------------------------------------------------------------
LOSSES = (3.0, 12.5, 10.0)          # against the threshold 10: above it on the second step only (the third sits at it: strictly greater)


def _flat_buffers(sgd, adam):
    return [sgd.group.pflat, sgd.group.gflat, sgd.mom, adam.group.pflat, adam.group.gflat, adam.m, adam.v]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("segmented", [False, True])
def test_fused_optimizers_gate_against_a_host_if(segmented, dtype):
    """FusedSGD + FusedAdamW, three steps: `a` takes when=(loss, 10) on the device, `b` a host `if` around the ungated call, `c` never
    clips and starts every step from a's buffers -- parameters, state and .grad bit-equal to b after each step, to c on the closed ones"""
    from vbg import optim as vo
    sets = [_flat_opts(segmented) for _ in range(3)]
    (na, sgd_a), (nb, adam_a) = sets[0]
    g1, g2 = _grads(3, seed=305), _grads(3, seed=306)
    for step, value in enumerate(LOSSES):
        norm = float(torch.cat([t.double().flatten() for t in list(g1[step].values()) + list(g2[step].values())]).norm())
        for x, y in zip(_flat_buffers(sets[2][0][1], sets[2][1][1]), _flat_buffers(sgd_a, adam_a)):
            x.copy_(y)
        for (n1, _), (n2, _) in sets:
            _set_grads(n1, g1[step])
            _set_grads(n2, g2[step])
        given = [sgd_a.group.gflat.clone(), adam_a.group.gflat.clone()]
        loss = _loss(value, dtype).to(dev())
        total = vo.clip_in_step([sgd_a, adam_a], 0.5 * norm, when=(loss.view(()), 10))
        coef = sgd_a._vbg_clip
        assert coef is adam_a._vbg_clip and coef.numel() == 1
        sgd_a.step()
        adam_a.step()
        (_, sgd_b), (_, adam_b) = sets[1]
        if value > 10:
            total_b = vo.clip_in_step([sgd_b, adam_b], 0.5 * norm)
            assert bits(total.view(1)).item() == bits(total_b.view(1)).item() and abs(float(total) - norm) <= 1e-6 * norm
            assert bits(coef).item() == bits(sgd_b._vbg_clip).item() and 0.49 < float(coef) < 0.51
        else:
            assert float(total) == 0.0 and float(coef) == 1.0
            assert torch.equal(bits(sgd_a.group.gflat), bits(given[0])) and torch.equal(bits(adam_a.group.gflat), bits(given[1]))          # .grad unwritten
        for o in sets[1][0][1], sets[1][1][1], sets[2][0][1], sets[2][1][1]:
            o.step()
        for other in (1,) if value > 10 else (1, 2):
            for k, (x, y) in enumerate(zip(_flat_buffers(sgd_a, adam_a), _flat_buffers(sets[other][0][1], sets[other][1][1]))):
                assert torch.equal(bits(x), bits(y)), (step, other, k)
        if value > 10:
            assert not torch.equal(bits(sgd_a.group.pflat), bits(sets[2][0][1].group.pflat))          # the clip did bite
    assert sgd_a.steps == 3 and adam_a.steps == 3 and sgd_a._vbg_clip is None


def _copy_stock(dst_named, dst_opt, src_named, src_opt):
    """parameters and optimizer state of one fuse()d optimizer onto another over the same layout"""
    with torch.no_grad():
        for (_, q), (_, p) in zip(dst_named, src_named):
            q.copy_(p)
            for k, t in src_opt.state.get(p, {}).items():
                if k in dst_opt.state.get(q, {}) and isinstance(t, torch.Tensor):
                    dst_opt.state[q][k].copy_(t)


def _stock_equal(a, b):
    (named_a, opt_a), (named_b, opt_b) = a, b
    ok = True
    for (n, p), (_, q) in zip(named_a, named_b):
        ok = ok and (torch.equal(bits(p), bits(q)) or print("parameter", n))
        ok = ok and (torch.equal(bits(p.grad), bits(q.grad)) or print("grad", n))
        ok = ok and (list(opt_a.state.get(p, {})) == list(opt_b.state.get(q, {})) or print("state keys", n))
        for k, t in opt_a.state.get(p, {}).items():
            u = opt_b.state[q][k]
            ok = ok and ((torch.equal(bits(t), bits(u)) if t.is_cuda else float(t) == float(u)) or print("state", k, n))
    return bool(ok)


@pytest.mark.parametrize("config", ["sgd_nesterov", "adamw_amsgrad"])
def test_fused_stock_optimizers_gate_against_a_host_if(config):
    """the same three twins with fuse()d torch.optim objects, an fp64 loss as ViBERTgridNet.forward returns it"""
    from vbg import optim as vo
    a, b, c = [_pair(config) for _ in range(3)]
    for step, (value, grads) in enumerate(zip(LOSSES, _grads(3, seed=312))):
        norm = float(torch.cat([t.double().flatten() for t in grads.values()]).norm())
        if step:
            _copy_stock(c[0], c[2], a[0], a[2])
        for named, twin, _, _, group in (a, b, c):
            _give(named, twin, group, grads)
        given = a[4].gflat.clone()
        loss = torch.tensor(value, dtype=torch.float64, device=dev())
        total = vo.clip_in_step([a[2]], 0.5 * norm, when=(loss, 10.0))
        coef = a[2]._vbg_clip
        a[2].step()
        if value > 10:
            total_b = vo.clip_in_step([b[2]], 0.5 * norm)
            assert bits(total.view(1)).item() == bits(total_b.view(1)).item() and bits(coef).item() == bits(b[2]._vbg_clip).item()
            assert 0.49 < float(coef) < 0.51
        else:
            assert float(total) == 0.0 and float(coef) == 1.0 and torch.equal(bits(a[4].gflat), bits(given))
        b[2].step()
        c[2].step()
        assert _stock_equal((a[0], a[2]), (b[0], b[2])), step
        if value > 10:
            assert not torch.equal(bits(a[4].pflat), bits(c[4].pflat))
        else:
            assert _stock_equal((a[0], a[2]), (c[0], c[2])), step
    fs = a[2]._vbg_fused
    assert (fs.launches, fs.fallbacks) == (3, 0), fs.last_fallback


@pytest.mark.parametrize("norm_type", [1.0, INF])
@pytest.mark.parametrize("config", ["sgd_nesterov", "adamw_amsgrad"])
def test_other_norm_types_against_fp64_torch_twins(config, norm_type):
    """fuse()d torch.optim objects, head.weight's .grad None in every step, the gate open: the fp64 twin runs
    torch.nn.utils.clip_grad_norm_(..., norm_type=...) and steps"""
    from vbg import optim as vo
    named, twin, opt, topt, group = _pair(config)
    who = "head.weight"
    loss = torch.tensor([12.5], device=dev())
    for step, grads in enumerate(_grads(3, seed=312)):
        _give(named, twin, group, grads, absent=(who,))
        present = torch.cat([t.double().flatten() for n, t in grads.items() if n != who]).abs()
        norm = float(present.sum() if norm_type == 1.0 else present.max())
        max_norm = 1e3 * norm if step == 2 else 0.5 * norm
        total = vo.clip_in_step([opt], max_norm, norm_type=norm_type, when=(loss, 10))
        coef = opt._vbg_clip
        opt.step()
        want = torch.nn.utils.clip_grad_norm_([q for _, q in twin], max_norm, norm_type=norm_type)
        topt.step()
        assert abs(float(want) - norm) <= 1e-12 * norm
        assert abs(float(total) - norm) <= (28 * U if norm_type == 1.0 else U) * norm, (float(total), norm)
        assert (float(coef) == 1.0) == (step == 2) and (step == 2 or 0.49 < float(coef) < 0.51)
        assert _same(named, twin, f"after step {step + 1}") and _state_equal(named, twin, opt, topt)
        for (n, p), (_, q) in zip(named, twin):                                      # .grad holds the clipped gradient, as torch leaves it
            assert (p.grad is None) == (n == who) and (n == who or close(p.grad, q.grad, 1e-6, 1e-7))
    fs = opt._vbg_fused
    assert (fs.launches, fs.fallbacks) == (3, 0), fs.last_fallback


@pytest.mark.parametrize("norm_type", [1, INF])
def test_other_norm_types_on_fused_sgd_and_adamw(norm_type):
    """FusedSGD + FusedAdamW, one norm over both: the total against fp64, and the step against twins that take the coefficient read back
    from the device through ops.scale_ and the plain step() -- bit-equal"""
    from vbg import ops
    a, b = _flat_opts(True), _flat_opts(True)
    from vbg import optim as vo
    g1, g2 = _grads(1, seed=305)[0], _grads(1, seed=306)[0]
    for (n1, _), (n2, _) in (a, b):
        _set_grads(n1, g1)
        _set_grads(n2, g2)
    every = torch.cat([t.double().flatten() for t in list(g1.values()) + list(g2.values())]).abs()
    norm = float(every.sum() if norm_type == 1 else every.max())
    total = vo.clip_in_step([a[0][1], a[1][1]], 0.5 * norm, norm_type=norm_type)
    c = float(a[0][1]._vbg_clip)
    assert abs(float(total) - norm) <= (28 * U if norm_type == 1 else 0.0) * norm and 0.49 < c < 0.51
    t, cr, _ = finish_ref([float(total)], 0, 0.5 * norm)
    assert bits(torch.tensor(c)).item() == bits(torch.tensor(float(cr))).item()
    for (_, o), (_, o2) in zip(a, b):
        o.step()
        ops.scale_(o2.group.gflat, c)
        o2.step()
    for k, (x, y) in enumerate(zip(_flat_buffers(a[0][1], a[1][1]), _flat_buffers(b[0][1], b[1][1]))):
        assert torch.equal(bits(x), bits(y)), k


@pytest.mark.parametrize("value", [3.0, 12.5])
def test_a_closure_step_under_the_gate(value):
    """a step that falls back to torch's own multiplies the present gradients by the pending coefficient first: exactly 1 under a closed
    gate (the bits of .grad stay), the clip's factor under an open one"""
    from vbg import optim as vo
    a, b = _pair("sgd_nesterov"), _pair("sgd_nesterov")
    grads = _grads(1, seed=313)[0]
    for named, twin, _, _, group in (a, b):
        _give(named, twin, group, grads)
    start = a[4].pflat.clone()
    norm = float(torch.cat([t.double().flatten() for t in grads.values()]).norm())
    loss = torch.tensor(value, dtype=torch.float64, device=dev())
    total = vo.clip_in_step([a[2]], 0.5 * norm, when=(loss, 10))
    coef = a[2]._vbg_clip.clone()
    a[2].step(lambda: None)
    assert a[2]._vbg_fused.last_fallback == "closure" and a[2]._vbg_clip is None
    if value > 10:
        assert 0.49 < float(coef) < 0.51 and abs(float(total) - norm) <= 1e-6 * norm
        for _, q in b[0]:
            q.grad.mul_(coef.reshape(()))
    else:
        assert float(coef) == 1.0 and float(total) == 0.0
    b[2].step(lambda: None)
    # (torch's own foreach step may write .grad itself -- nesterov without weight decay adds the momentum in place -- so the gradients
    # are held against the twin's, which never saw a coefficient under the closed gate)
    assert _stock_equal((a[0], a[2]), (b[0], b[2]))
    assert not torch.equal(bits(a[4].pflat), bits(start))


def test_what_the_device_call_refuses():
    from vbg import optim as vo
    (named, sgd), _ = _flat_opts(False)
    with pytest.raises(ValueError, match="lives on cpu"):                            # a loss on the CPU
        vo.clip_in_step([sgd], 1.0, when=(torch.tensor(3.0, dtype=torch.float64), 10))
    with pytest.raises(TypeError):
        vo.clip_in_step([sgd], 1.0, when=(torch.tensor(3, device=dev()), 10))         # an integer loss
    with pytest.raises(ValueError):
        vo.clip_in_step([sgd], 1.0, when=(torch.zeros(2, device=dev()), 10))
    with pytest.raises(ValueError):
        vo.clip_in_step([sgd], 1.0, norm_type=3)
    assert sgd._vbg_clip is None


def test_no_host_sync_from_backward_to_step():
    """torch's sync-debug mode around clip_in_step(..., when=(loss, 10)) and both step() calls on a second step (tables and buffers belong
    to the first), with the loss a device tensor nobody reads on the host: nothing waits for the device"""
    from vbg import optim as vo
    (n1, sgd), (n2, adam) = _flat_opts(False)
    w = {n: rnd(*p.shape, seed=500 + i).to(dev()) for i, (n, p) in enumerate(n1 + n2)}
    raised = None
    totals = []
    for step in range(3):
        sgd.zero_grad()
        adam.zero_grad()
        loss = sum(((p * w[n]) ** 2).sum() for n, p in n1 + n2).double() * (1e-4 if step == 2 else 1.0)
        loss.backward()
        torch.cuda.synchronize()
        if step >= 1:
            torch.cuda.set_sync_debug_mode("error")
        try:
            totals.append(vo.clip_in_step([sgd, adam], 1.0, when=(loss.detach(), 10), norm_type=INF if step == 1 else 2))
            sgd.step()
            adam.step()
        except RuntimeError as e:
            raised = str(e)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert raised is None, raised
    assert all(t.is_cuda and t.dim() == 0 for t in totals) and float(totals[0]) > 0 and float(totals[1]) > 0
    assert float(totals[2]) == 0.0                                                   # the small loss of the third step closed the gate
    assert sgd.steps == 3 and adam.steps == 3
