"""GradScaler's pass over the gradients in one launch, on the GPU: vbg_grad_unscale_check_seg against torch's own op
(torch._amp_foreach_non_finite_check_and_unscale_ on the covered slices, same device) on the canary-filled TOTAL / RUNS / CHUNK layout of
tests/test_gpu_optim_groups.py; one planted inf / NaN at every place of the row walk where a test could be lost; the set-only flag;
vbg_grad_sumsq_seg_inf against vbg_grad_sumsq_seg bit for bit; and `vbg.optim.fuse_scaler` in real loops -- the `_amp_pair` twins of
tests/test_gpu_stock_optim_amp.py and FusedSGD / FusedAdamW under a fused scaler against the same loop under a plain one, bit for bit
after every step, with torch's op patched to raise -- and torch's sync-debug mode around two scaler.step calls and update().  Every
comparison here is exact (bits, or the class of a non-finite value): the kernels state one rounded product and torch's op does the same.
Needs a real MI355X."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_clip_step import _flat_opts
from test_gpu_optim_groups import CHUNK, RUNS, TOTAL, _grads, _set_grads, cut, dev, inside
from test_gpu_small_kernels import bits, rnd
from test_gpu_stock_optim_amp import _amp_pair
from test_optim_groups_host import LAYOUT

FLT_MAX = float(np.finfo(np.float32).max)
INVS = {"one": 1.0, "2^-10": 2.0 ** -10, "1/1000": float(torch.tensor(1000.0).double().reciprocal().float())}
PLANTS = {"+inf": float("inf"), "-inf": float("-inf"), "nan": float("nan")}
SEG_THREADS = 256          # csrc/optim.hip: a row of fewer than 4 * SEG_THREADS elements leaves threads of the block without a float4


@pytest.fixture(scope="module")
def ops():
    from vbg import ops as _ops
    return _ops


def _scalar(v):
    return torch.full((), float(v), device=dev())


def _table(ops, rows, total):
    return ops.chunk_table(rows, max(r[2] for r in rows) + 1, total, dev())


def _input(seed=150, scale=1024.0):
    """TOTAL elements: scaled gradients inside the runs with FLT_MAX, a denormal and -0.0 among them, NaN / 1e30 canaries outside"""
    m = inside(RUNS, TOTAL)
    g0 = rnd(TOTAL, seed=seed) * scale
    for i, v in ((0, FLT_MAX), (7, -FLT_MAX), (30, 1e-41), (31, -1e-45), (100, -0.0), (248 + 4103, FLT_MAX), (2000, 1.1754942e-38)):
        assert m[i]
        g0[i] = v
    canary = torch.where(torch.arange(TOTAL) % 2 == 0, torch.full((), float("nan")), torch.full((), 1e30))
    return torch.where(m, g0, canary), m


def _torch_op(g0, runs, inv):
    """torch's op on the covered slices of a device copy -> (g afterwards on the host, flag)"""
    g = g0.to(dev())
    flag = _scalar(0.0)
    torch._amp_foreach_non_finite_check_and_unscale_([g[s:s + n] for s, n, _ in runs], flag, _scalar(inv))
    return g.cpu(), float(flag)


def _same_class(a, b):
    """bit-equal where b is finite; elsewhere the same class: +inf, -inf or NaN"""
    fin = torch.isfinite(b)
    return (torch.equal(bits(a)[fin], bits(b)[fin]) and torch.equal(torch.isnan(a), torch.isnan(b))
            and torch.equal(torch.isposinf(a), torch.isposinf(b)) and torch.equal(torch.isneginf(a), torch.isneginf(b)))


# ------------------------------------------------------------------------------------------
# the kernel against torch's op
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [CHUNK, 4096])
@pytest.mark.parametrize("inv", list(INVS))
def test_unscale_check_against_torchs_op(ops, inv, chunk):
    inv = INVS[inv]
    g0, m = _input()
    rows = cut(RUNS, chunk)
    table = _table(ops, rows, TOTAL)
    # finite input (FLT_MAX, denormals and -0.0 included): flag 0, g what torch's op leaves
    g, flag = g0.to(dev()), _scalar(0.0)
    ops.grad_unscale_check_seg(g, table, _scalar(inv), flag)
    want, wflag = _torch_op(g0, RUNS, inv)
    assert float(flag) == 0.0 == wflag
    assert torch.equal(bits(g)[m], bits(want)[m]) and torch.equal(bits(g)[~m], bits(g0)[~m])
    assert torch.equal(bits(want)[~m], bits(g0)[~m])
    if inv == 1.0:
        assert torch.equal(bits(g), bits(g0))
    else:
        assert not torch.equal(bits(g)[m], bits(g0)[m])
    # the three non-finite values among them: flag 1, the finite elements torch's bits, the others torch's class
    g1 = g0.clone()
    for i, v in ((5, float("inf")), (170, float("-inf")), (3000, float("nan")), (248 + 4100, float("inf"))):
        g1[i] = v
    g, flag = g1.to(dev()), _scalar(0.0)
    ops.grad_unscale_check_seg(g, table, _scalar(inv), flag)
    want, wflag = _torch_op(g1, RUNS, inv)
    assert float(flag) == 1.0 == wflag
    assert _same_class(g.cpu()[m], want[m]) and torch.equal(bits(g)[~m], bits(g1)[~m])
    if inv == 1.0:
        assert torch.equal(bits(g), bits(g1))


# (place, chunk length of the table over RUNS, index): every one inside a run
PLACES = [(f"float4 component {c}", CHUNK, 248 + 64 * 7 + 4 * 5 + c) for c in range(4)] + [
    ("first element of a run", CHUNK, 160), ("last element of a run", CHUNK, 160 + 72 - 1),
    ("first element of the first run", CHUNK, 0), ("last element of the last run", CHUNK, 248 + 4104 - 1),
    ("last float4 of a 56-element row", CHUNK, 24 + 52), ("last float4 of an 8-element row", 4096, 232 + 4),
    ("fourth trip of a 4096-element row", 4096, 248 + 3 * 4 * SEG_THREADS + 4 * 77 + 2), ("last float4 of a 4096-element row", 4096, 248 + 4095)]


@pytest.mark.parametrize("value", list(PLANTS))
@pytest.mark.parametrize("place", range(len(PLACES)), ids=[p[0].replace(" ", "_") for p in PLACES])
def test_one_planted_value_sets_the_flag(ops, place, value):
    _, chunk, idx = PLACES[place]
    g0, m = _input()
    assert m[idx]
    g0[idx] = PLANTS[value]
    table = _table(ops, cut(RUNS, chunk), TOTAL)
    g, flag = g0.to(dev()), _scalar(0.0)
    ops.grad_unscale_check_seg(g, table, _scalar(1.0), flag)
    assert float(flag) == 1.0 and _torch_op(g0, RUNS, 1.0)[1] == 1.0
    assert torch.equal(bits(g), bits(g0))
    flag = _scalar(0.0)
    ops.grad_unscale_check_seg(g, table, _scalar(INVS["1/1000"]), flag)              # the storing loop tests before it multiplies
    assert float(flag) == 1.0
    flag, part = _scalar(0.0), torch.empty(table.n, device=dev())
    ops.grad_sumsq_seg_inf(g0.to(dev()), table, part, flag)                          # the norm pass's loop
    assert float(flag) == 1.0


def _short_rows():
    """2 100 rows of 4 and 8 elements, 8 apart: past the 2 048-block grid cap, so 52 blocks walk a second row"""
    return [(8 * i, 4 if i % 2 else 8, 0) for i in range(2100)], 8 * 2100


@pytest.mark.parametrize("value", list(PLANTS))
def test_a_row_reached_on_the_second_stride(ops, value):
    rows, total = _short_rows()
    table = _table(ops, rows, total)
    g0 = rnd(total, seed=151) * 1024.0
    clean, flag = g0.to(dev()), _scalar(0.0)
    ops.grad_unscale_check_seg(clean, table, _scalar(1.0), flag)
    assert float(flag) == 0.0
    for row, at in ((2048, 0), (2075, 3), (2099, 2), (2098, 7)):
        g1 = g0.clone()
        g1[8 * row + at] = PLANTS[value]
        assert at < rows[row][1]
        for inv in (1.0, INVS["2^-10"]):
            g, flag = g1.to(dev()), _scalar(0.0)
            ops.grad_unscale_check_seg(g, table, _scalar(inv), flag)
            assert float(flag) == 1.0, (row, at, inv)
        flag, part = _scalar(0.0), torch.empty(table.n, device=dev())
        ops.grad_sumsq_seg_inf(g1.to(dev()), table, part, flag)
        assert float(flag) == 1.0, (row, at)
    # the four elements a 4-element row leaves uncovered, on the second stride as well
    g1 = g0.clone()
    g1[8 * 2075 + 5] = PLANTS[value]
    g1[8 * 1 + 4] = PLANTS[value]
    g, flag = g1.to(dev()), _scalar(0.0)
    ops.grad_unscale_check_seg(g, table, _scalar(INVS["2^-10"]), flag)
    assert float(flag) == 0.0
    covered = inside(rows, total)
    assert torch.equal(bits(g)[~covered], bits(g1)[~covered]) and torch.equal(bits(g)[covered], bits(g1 * INVS["2^-10"])[covered])


@pytest.mark.parametrize("value", list(PLANTS))
def test_what_no_row_covers_does_not_set_the_flag(ops, value):
    g0 = rnd(TOTAL, seed=152) * 1024.0
    m = inside(RUNS, TOTAL)
    for i in (16, 23, 144, 159, 240, 247, 248 + 4104, TOTAL - 1):                    # the three gaps between runs and the tail
        assert not m[i]
        g0[i] = PLANTS[value]
    for chunk in (CHUNK, 4096):
        table = _table(ops, cut(RUNS, chunk), TOTAL)
        for inv in (1.0, INVS["1/1000"]):
            g, flag = g0.to(dev()), _scalar(0.0)
            ops.grad_unscale_check_seg(g, table, _scalar(inv), flag)
            assert float(flag) == 0.0 and torch.equal(bits(g)[~m], bits(g0)[~m])
        flag, part = _scalar(0.0), torch.empty(table.n, device=dev())
        ops.grad_sumsq_seg_inf(g0.to(dev()), table, part, flag)
        assert float(flag) == 0.0 and bool(torch.isfinite(part).all())


def test_the_flag_is_only_ever_set(ops):
    g0, m = _input()
    table = _table(ops, cut(RUNS, CHUNK), TOTAL)
    clean = g0.to(dev())
    dirty = g0.clone()
    dirty[300] = float("nan")
    dirty = dirty.to(dev())
    part = torch.empty(table.n, device=dev())
    for check in (lambda g, f: ops.grad_unscale_check_seg(g, table, _scalar(1.0), f), lambda g, f: ops.grad_sumsq_seg_inf(g, table, part, f)):
        flag = _scalar(1.0)
        check(clean, flag)
        assert float(flag) == 1.0                                                    # handed in as 1: stays 1 on clean input
        flag = _scalar(0.0)
        check(dirty, flag)
        assert float(flag) == 1.0
        fresh = _scalar(0.0)
        check(clean, fresh)
        assert float(fresh) == 0.0 and float(flag) == 1.0                            # a fresh zero after a dirty call stays 0
        two = _scalar(2.0)                                                           # (GradScaler sums flags: any non-zero value is kept or becomes 1)
        check(clean, two)
        assert float(two) == 2.0


# ------------------------------------------------------------------------------------------
# vbg_grad_sumsq_seg_inf
# ------------------------------------------------------------------------------------------
def _both_norms(ops, g, table):
    """(partials of vbg_grad_sumsq_seg, partials of vbg_grad_sumsq_seg_inf, flag, canaries around the latter intact)"""
    a = torch.empty(table.n, device=dev())
    buf = torch.full((table.n + 16,), 777.0, device=dev())
    b, flag = buf[8:8 + table.n], _scalar(0.0)
    ops.grad_sumsq_seg(g, table, a)
    ops.grad_sumsq_seg_inf(g, table, b, flag)
    return a.cpu(), b.cpu(), float(flag), bool((buf[:8] == 777.0).all()) and bool((buf[8 + table.n:] == 777.0).all())


@pytest.mark.parametrize("layout", ["chunk64", "chunk4096", "short_rows"])
def test_sumsq_inf_partials_are_the_norm_passes_bits(ops, layout):
    if layout == "short_rows":
        rows, total = _short_rows()
        g0 = rnd(total, seed=153)
    else:
        rows, total = cut(RUNS, CHUNK if layout == "chunk64" else 4096), TOTAL
        g0, _ = _input(scale=1.0)
        g0 = torch.where(torch.isfinite(g0) & (g0.abs() < 1e18), g0, torch.full((), 3.0))          # (finite squares inside the runs)
    table = _table(ops, rows, total)
    g = g0.to(dev())
    a, b, flag, intact = _both_norms(ops, g, table)
    assert intact and flag == 0.0 and torch.equal(bits(a), bits(b)) and bool(torch.isfinite(a).all()) and bool((a > 0).all())
    assert torch.equal(bits(g), bits(g0))
    # rows with a planted inf / NaN: the same class in both, the other rows the same bits, the flag set
    g1 = g0.clone()
    at = [rows[1][0], rows[len(rows) // 2][0] + 2, rows[-1][0] + rows[-1][1] - 1]
    for i, v in zip(at, PLANTS.values()):
        g1[i] = v
    a, b, flag, intact = _both_norms(ops, g1.to(dev()), table)
    assert intact and flag == 1.0 and _same_class(b, a) and int((~torch.isfinite(a)).sum()) == 3
    assert bool(torch.isposinf(a[1])) and bool(torch.isposinf(a[len(rows) // 2])) and bool(torch.isnan(a[-1]))          # (+inf)^2, (-inf)^2, NaN


def test_squares_that_overflow_are_not_an_inf_gradient(ops):
    """a row of 1e30: finite gradients, a partial of inf -- the flag comes from the elements"""
    g0, m = _input(scale=1.0)
    g0 = torch.where(m, g0.clamp(-10, 10), g0)
    g0[80:144] = 1e30
    table = _table(ops, cut(RUNS, CHUNK), TOTAL)
    a, b, flag, intact = _both_norms(ops, g0.to(dev()), table)
    row = [r[0] for r in cut(RUNS, CHUNK)].index(80)
    assert intact and flag == 0.0 and torch.equal(bits(a), bits(b))
    assert bool(torch.isposinf(b[row])) and int((~torch.isfinite(b)).sum()) == 1
    flag = _scalar(0.0)
    ops.grad_unscale_check_seg(g0.to(dev()), table, _scalar(1.0), flag)
    assert float(flag) == 0.0


# ------------------------------------------------------------------------------------------
# vbg.optim.fuse_scaler in real loops
# ------------------------------------------------------------------------------------------
CONFIGS = ["sgd_nesterov", "adamw_amsgrad"]


def _refuse_torchs_pass(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("torch._amp_foreach_non_finite_check_and_unscale_ ran under a fused scaler")
    monkeypatch.setattr(torch, "_amp_foreach_non_finite_check_and_unscale_", refuse)


def _count_wrappers(monkeypatch, ops):
    """pass-through shims around the two wrappers -> the counters they bump"""
    n = {"check": 0, "norm_inf": 0}
    check, norm = ops.grad_unscale_check_seg, ops.grad_sumsq_seg_inf
    monkeypatch.setattr(ops, "grad_unscale_check_seg", lambda *a: (n.__setitem__("check", n["check"] + 1), check(*a))[1])
    monkeypatch.setattr(ops, "grad_sumsq_seg_inf", lambda *a: (n.__setitem__("norm_inf", n["norm_inf"] + 1), norm(*a))[1])
    return n


def _stock_loop(variant, fused):
    """three steps of the quadratic loss of tests/test_gpu_stock_optim_amp.py over the two `_amp_pair` twins on ONE GradScaler
    (init_scale 1024, growth_interval 2), an inf planted in the AdamW side's gradients in step two.  variant: "step" (scaler.step alone,
    amp_scaling=True), "clip" (clip_in_step(scaler=) + step, amp_scaling=True), "unscale_clip" (unscale_ + torch's clip_grad_norm_ + step,
    fused without amp_scaling).  -> (per-step records, scaler, sides)"""
    from vbg import optim as vo
    sides = [_amp_pair(config, variant != "unscale_clip", seed=j) for j, config in enumerate(CONFIGS)]
    w = {n: rnd(*s, seed=400 + i) for i, (n, s, _) in enumerate(LAYOUT)}
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0, growth_interval=2)
    if fused:
        assert vo.fuse_scaler(scaler) is scaler
    records = []
    for step in range(3):
        for *_, group in sides:
            group.zero_grad()
        scaler.scale(sum(((p * w[n].to(dev())) ** 2).sum() for named, *_ in sides for n, p in named)).backward()
        if step == 1:
            sides[1][0][2][1].grad.view(-1)[3] = float("inf")
        scaled = [group.gflat.clone() for *_, group in sides]
        if variant == "clip":
            vo.clip_in_step([s[2] for s in sides], 1.0, scaler=scaler)
        for named, _, opt, _, _ in sides:
            if variant == "unscale_clip":
                scaler.unscale_(opt)
                torch.nn.utils.clip_grad_norm_([p for _, p in named], 1.0)
            scaler.step(opt)
        scaler.update()
        rec = {"scale": scaler.get_scale(), "tracker": scaler._get_growth_tracker(), "scaled": scaled}
        for j, (named, _, opt, _, group) in enumerate(sides):
            opt._vbg_fused.reconcile()
            rec[j] = {"p": group.pflat.clone(), "g": group.gflat.clone(),
                      "state": {(n, k): (t.clone() if k != "step" else float(t)) for n, p in named for k, t in opt.state.get(p, {}).items()}}
        records.append(rec)
    return records, scaler, sides


@pytest.mark.parametrize("variant", ["step", "clip", "unscale_clip"])
def test_stock_optimizers_under_a_fused_scaler_equal_a_plain_one(ops, monkeypatch, variant):
    plain, _, sides_p = _stock_loop(variant, False)
    with monkeypatch.context() as mp:
        _refuse_torchs_pass(mp)
        n = _count_wrappers(mp, ops)
        fused, scaler, sides_f = _stock_loop(variant, True)
    for step, (a, b) in enumerate(zip(plain, fused)):
        assert a["scale"] == b["scale"] and a["tracker"] == b["tracker"], step
        for j in range(2):
            assert torch.equal(bits(a["scaled"][j]), bits(b["scaled"][j])), (step, j)          # identical gradients went in
            assert torch.equal(bits(a[j]["p"]), bits(b[j]["p"])) and torch.equal(bits(a[j]["g"]), bits(b[j]["g"])), (step, j)
            assert list(a[j]["state"]) == list(b[j]["state"]), (step, j)
            for key, t in a[j]["state"].items():
                u = b[j]["state"][key]
                assert (t == u) if key[1] == "step" else torch.equal(bits(t), bits(u)), (step, j, key)
    assert [r["scale"] for r in fused] == [1024.0, 512.0, 512.0] and [r["tracker"] for r in fused] == [1, 0, 1]
    # the inf skipped the AdamW side only, and everything else moved
    assert torch.equal(bits(fused[1][1]["p"]), bits(fused[0][1]["p"])) and not torch.equal(bits(fused[1][0]["p"]), bits(fused[0][0]["p"]))
    assert not torch.equal(bits(fused[2][1]["p"]), bits(fused[1][1]["p"]))
    fs = scaler._vbg_fused
    want = {"step": (6, 0, 6, 0), "clip": (0, 6, 0, 6), "unscale_clip": (6, 0, 6, 0)}[variant]
    assert (n["check"], n["norm_inf"], fs.launches, fs.reused) == want and fs.fallbacks == 0, (n, fs.launches, fs.reused, fs.last_fallback)
    for sides in (sides_p, sides_f):
        assert all(s[2]._vbg_fused.fallbacks == 0 for s in sides)


@pytest.mark.parametrize("segmented", [False, True])
def test_fused_sgd_and_adamw_under_a_fused_scaler_equal_a_plain_one(ops, monkeypatch, segmented):
    """the generic route (these classes stay outside the amp_scaling protocol): scaler.step runs unscale_ -- one launch with the real
    inverse under the fused scaler -- reads the flag and steps; scale 1000 (an inverse that rounds), an inf in AdamW's gradients in step two"""
    from vbg import optim as vo

    def loop(fused):
        (n1, sgd), (n2, adam) = _flat_opts(segmented)
        scaler = torch.amp.GradScaler("cuda", init_scale=1000.0, growth_interval=2)
        scaler.scale(torch.zeros((), device=dev()))
        if fused:
            vo.fuse_scaler(scaler)
        g1, g2 = _grads(3, seed=320), _grads(3, seed=321)
        out = []
        for step in range(3):
            s = scaler.get_scale()
            _set_grads(n1, {k: v * s for k, v in g1[step].items()})
            _set_grads(n2, {k: v * s for k, v in g2[step].items()})
            if step == 1:
                n2[2][1].grad.view(-1)[3] = float("inf")
            scaler.step(sgd)
            scaler.step(adam)
            scaler.update()
            out.append([scaler.get_scale(), scaler._get_growth_tracker(), sgd.steps, adam.steps] +
                       [t.clone() for t in (sgd.group.pflat, sgd.group.gflat, sgd.mom, adam.group.pflat, adam.group.gflat, adam.m, adam.v)])
        return out, scaler

    plain, _ = loop(False)
    with monkeypatch.context() as mp:
        _refuse_torchs_pass(mp)
        n = _count_wrappers(mp, ops)
        fused, scaler = loop(True)
    for step, (a, b) in enumerate(zip(plain, fused)):
        assert a[:4] == b[:4], (step, a[:4], b[:4])
        for k, (x, y) in enumerate(zip(a[4:], b[4:])):
            assert torch.equal(bits(x), bits(y)), (step, k)
    assert [r[:4] for r in fused] == [[1000.0, 1, 1, 1], [500.0, 0, 2, 1], [500.0, 1, 3, 2]]
    fs = scaler._vbg_fused
    assert (n["check"], n["norm_inf"], fs.launches, fs.reused, fs.fallbacks) == (6, 0, 6, 0, 0), fs.last_fallback


def test_no_host_sync_from_the_first_step_call_to_update():
    """torch's sync-debug mode around scaler.step(opt_cnn); scaler.step(opt_bert); scaler.update() on a second step (the chunk tables
    belong to the first): both optimizers fused with amp_scaling, the scaler fused, no clip -- nothing waits for the device"""
    from vbg import optim as vo
    w = {n: rnd(*s, seed=400 + i) for i, (n, s, _) in enumerate(LAYOUT)}
    sides = [_amp_pair(config, True, seed=j) for j, config in enumerate(CONFIGS)]
    opt_cnn, opt_bert = sides[0][2], sides[1][2]
    scaler = vo.fuse_scaler(torch.amp.GradScaler("cuda", init_scale=1024.0))
    raised = None
    for step in range(2):
        for *_, group in sides:
            group.zero_grad()
        scaler.scale(sum(((p * w[n].to(dev())) ** 2).sum() for named, *_ in sides for n, p in named)).backward()
        torch.cuda.synchronize()
        if step == 1:
            torch.cuda.set_sync_debug_mode("error")
        try:
            scaler.step(opt_cnn)
            scaler.step(opt_bert)
            scaler.update()
        except RuntimeError as e:
            raised = str(e)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert raised is None, raised
    fs = scaler._vbg_fused
    assert (fs.launches, fs.reused, fs.fallbacks) == (4, 0, 0), fs.last_fallback
    for o in (opt_cnn, opt_bert):
        o._vbg_fused.reconcile()
        assert (o._vbg_fused.launches, o._vbg_fused.fallbacks, o._vbg_fused.skipped) == (2, 0, 0)
    assert scaler.get_scale() == 1024.0
