"""Per-parameter statistics on the device (csrc/stats.hip; vbg/stats.py): vbg_param_stats_rows / vbg_param_stats_finish on raw,
canary-framed buffers against the numpy restatement of tests/param_stats_restate.py -- integer fields and amax exactly, the sum of
squares against math.fsum of the exact double squares within the bound derived from the table -- and vbg.stats.ParamStats on the
small model: against the gradients themselves, against vbg.optim.clip_grad_norm_, with a planted inf, with a GradScaler, without a
host sync.  Needs a real MI355X."""
import math
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import param_stats_restate as R
from test_gpu_model import to_dev
from test_gpu_small_kernels import bits
from test_gpu_train_loop import _fused_opts, _net
from test_optim_groups_host import LAYOUT
from test_oracle_golden import _e2e_inputs
from weight_average_restate import homed_six

NUMELS = [1, 3, 4, 5, 7, 8, 9, 4095, 4096, 4097, 2 * 4096 + 1]
LONG = [4096 * 257 + 5]                                    # 258 rows of 4096: the finish walks more rows than a block has lanes
SHORT = [1 + i % 13 for i in range(100)]                   # 100 consecutive parameters of 1 .. 13 elements
LONGER = [4096 * 1030 + 3]                                 # ... and more rows of 4096 than the finish's block of 1024 lanes has
LAYOUTS = {"edges": NUMELS, "long": LONG, "longer": LONGER, "short": SHORT}
CHUNKS = (64, 4096)
PAD = 8
INT_FIELDS = ("amax_bits", "nonfinite", "zeros", "over_f16", "hist")


def dev():
    return torch.device("cuda")


def fill(numels, seed):
    """the buffer of a layout on the host: every parameter's elements from R.mixed_values, every element of padding NaN or inf"""
    offsets, total = R.layout(numels)
    buf = np.empty(total, dtype=np.float32)
    buf[0::2] = np.nan
    buf[1::2] = np.inf
    for i, (off, n) in enumerate(zip(offsets, numels)):
        buf[off:off + n] = R.mixed_values(n, seed=seed + i)
    return offsets, total, buf


def framed(buf):
    """`buf` inside a device buffer with NaN / inf canaries on both sides -> (whole buffer, the range as a 16-byte aligned view)"""
    whole = torch.empty(PAD + len(buf) + PAD)
    whole[0::2] = float("nan")
    whole[1::2] = float("inf")
    whole[PAD:PAD + len(buf)] = torch.from_numpy(buf)
    whole = whole.to(dev())
    view = whole[PAD:PAD + len(buf)]
    assert view.data_ptr() % 16 == 0
    return whole, view


def launch(x, table, scale=None, total=None, recs=None):
    """one row pass and one finish -> (last as numpy records, the running table's device buffer, the row records' device buffer)"""
    from vbg import ops, stats
    if recs is None:
        recs = torch.empty(max(1, table.n) * ops.STATS_REC_BYTES, dtype=torch.uint8, device=dev())
    last = torch.empty(table.nparams * ops.STATS_REC_BYTES, dtype=torch.uint8, device=dev())
    sc = None if scale is None else torch.tensor([scale], dtype=torch.float32, device=dev())
    ops.param_stats_rows(x, table, recs, sc)
    ops.param_stats_finish(recs, table, last, total)
    torch.cuda.synchronize()
    return last.cpu().numpy().view(stats.REC_DTYPE), total, recs


def want_records(buf, offsets, numels, scale=None):
    return [R.record(buf[off:off + n], scale) for off, n in zip(offsets, numels)]


def bound(chunk, nrows):
    """relative bound on a parameter's sum of squares against the exact sum: every summand is non-negative and every product exact,
    so each of the at most chunk + nrows additions on any path through the row pass and the finish costs at most 2^-53"""
    return (chunk + nrows) * 2.0 ** -53


def compare(got, want, chunk, row_ptr, what):
    for i, w in enumerate(want):
        for k in INT_FIELDS:
            assert np.array_equal(got[k][i], w[k]), (what, i, k, got[k][i], w[k])
        nrows = int(row_ptr[i + 1] - row_ptr[i])
        err, lim = abs(float(got["sumsq"][i]) - w["sumsq"]), bound(chunk, nrows) * w["sumsq"]
        assert err <= lim, (what, i, float(got["sumsq"][i]), w["sumsq"], err, lim)


@pytest.fixture(scope="module")
def raw_runs():
    """every (layout, chunk) once without a scale: the host buffer, the table, the records, and whether x and the canaries kept their bits"""
    from vbg import ops, stats
    runs = {}
    for name, numels in LAYOUTS.items():
        offsets, total, buf = fill(numels, seed=17 * len(numels))
        want = want_records(buf, offsets, numels)
        for chunk in CHUNKS:
            rows, row_ptr = stats.stats_rows(offsets, numels, chunk)
            table = ops.stats_table(rows, row_ptr, total, dev())
            whole, view = framed(buf)
            before = bits(whole)
            got, _, _ = launch(view, table)
            runs[(name, chunk)] = (got, want, row_ptr, torch.equal(bits(whole), before))
    return runs


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_records_against_the_restatement(raw_runs, name, chunk):
    got, want, row_ptr, intact = raw_runs[(name, chunk)]
    assert intact, "x or a canary changed"
    numels = LAYOUTS[name]
    if name == "long":
        assert row_ptr[1] - row_ptr[0] > 256
    if name == "longer":                                                           # (the finish's block has 1024 lanes)
        assert row_ptr[1] - row_ptr[0] > 1024
    compare(got, want, chunk, row_ptr, (name, chunk))
    # nothing of the padding (all NaN / inf) was counted: every element of a parameter is in exactly one class
    for i, n in enumerate(numels):
        assert int(got["nonfinite"][i]) + int(got["zeros"][i]) + int(got["hist"][i].sum()) == n, (name, i)
    assert sum(int(w["nonfinite"]) for w in want) > 0 and sum(int(w["over_f16"]) for w in want) > 0          # (the planted values are there)


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_integer_fields_do_not_depend_on_the_chunk(raw_runs, name):
    a, b = raw_runs[(name, 64)][0], raw_runs[(name, 4096)][0]
    for k in INT_FIELDS:
        assert np.array_equal(a[k], b[k]), (name, k)


@pytest.mark.parametrize("scale", [65536.0, 1000.0, None])
def test_scale_is_torchs_inverse_and_one_rounded_product(scale):
    from vbg import ops, stats
    offsets, total, buf = fill(NUMELS, seed=901)
    want = want_records(buf, offsets, NUMELS, scale)
    plain = want_records(buf, offsets, NUMELS, None)
    if scale is not None:                                                          # (the scale shows: the classes move)
        assert any(not np.array_equal(w["hist"], p["hist"]) for w, p in zip(want, plain))
    for chunk in CHUNKS:
        rows, row_ptr = stats.stats_rows(offsets, NUMELS, chunk)
        table = ops.stats_table(rows, row_ptr, total, dev())
        whole, view = framed(buf)
        before = bits(whole)
        got, _, _ = launch(view, table, scale)
        assert torch.equal(bits(whole), before), "x is only ever read"
        compare(got, want, chunk, row_ptr, (scale, chunk))


def test_running_table_two_updates_then_reset():
    from vbg import ops, stats
    offsets, total, buf_a = fill(NUMELS, seed=31)
    _, _, buf_b = fill(NUMELS, seed=77)
    # the second update is finite everywhere except in parameters 3 and 9
    for i, (off, n) in enumerate(zip(offsets, NUMELS)):
        part = buf_b[off:off + n]
        part[~np.isfinite(part)] = 1.5
        if i in (3, 9):
            part[n // 2] = np.inf
    rows, row_ptr = stats.stats_rows(offsets, NUMELS, 64)
    table = ops.stats_table(rows, row_ptr, total, dev())
    tot = torch.zeros(table.nparams * ops.STATS_TOTAL_BYTES, dtype=torch.uint8, device=dev())
    want = [None] * len(NUMELS)
    for step, buf in enumerate((buf_a, buf_b)):
        last, _, _ = launch(framed(buf)[1], table, None, tot)
        recs = want_records(buf, offsets, NUMELS)
        want = [R.fold(t, r) for t, r in zip(want, recs)]
        compare(last, recs, 64, row_ptr, ("update", step))
        got = tot.cpu().numpy().view(stats.TOTAL_DTYPE)
        for i, w in enumerate(want):
            for k in ("amax_bits", "nonfinite", "zeros", "over_f16", "updates", "steps_nonfinite", "hist"):
                assert np.array_equal(got[k][i], w[k]), (step, i, k)
            assert got["sumsq"][i] == last["sumsq"][i]                             # the last value only
    had_a = [int(r["nonfinite"] > 0) for r in want_records(buf_a, offsets, NUMELS)]
    assert got["steps_nonfinite"].tolist() == [a + (1 if i in (3, 9) else 0) for i, a in enumerate(had_a)] and 0 in had_a
    assert got["updates"].tolist() == [2] * len(NUMELS)
    tot.zero_()                                                                    # what ParamStats.reset() does
    last, _, _ = launch(framed(buf_b)[1], table, None, tot)
    got = tot.cpu().numpy().view(stats.TOTAL_DTYPE)
    assert got["updates"].tolist() == [1] * len(NUMELS) and np.array_equal(got["hist"], last["hist"])
    assert np.array_equal(got["amax_bits"], last["amax_bits"]) and np.array_equal(got["nonfinite"], last["nonfinite"])


def test_two_calls_leave_the_same_bits_and_empty_launches_are_no_ops():
    from vbg import ops, stats
    offsets, total, buf = fill(LONG + NUMELS, seed=5)
    rows, row_ptr = stats.stats_rows(offsets, LONG + NUMELS, 4096)
    table = ops.stats_table(rows, row_ptr, total, dev())
    _, view = framed(buf)
    a, _, recs_a = launch(view, table)
    b, _, recs_b = launch(view, table)
    assert a.tobytes() == b.tobytes() and torch.equal(recs_a, recs_b)
    # nrows == 0 / nparams == 0: no pointer is looked at, nothing is written
    before = recs_a.clone()
    ops.check(ops.lib.vbg_param_stats_rows(None, None, 0, None, None, ops._stream()), "rows")
    ops.check(ops.lib.vbg_param_stats_finish(None, None, 0, None, None, ops._stream()), "finish")
    empty = ops.stats_table(np.zeros((0, 3), dtype=np.int64), [0], total, dev())
    assert (empty.n, empty.nparams) == (0, 0)
    ops.param_stats_rows(view, empty, recs_a)
    ops.param_stats_finish(recs_a, empty, torch.empty(0, dtype=torch.uint8, device=dev()))
    torch.cuda.synchronize()
    assert torch.equal(recs_a, before)


# ---- ParamStats ------------------------------------------------------------------------------------------------------------------
def test_no_host_sync_in_update_and_one_copy_in_read(monkeypatch):
    from vbg.stats import ParamStats
    model, g = homed_six(LAYOUT, dev())
    g.gflat.copy_(torch.from_numpy(R.mixed_values(g.total, seed=2)).to(dev()))
    ps = ParamStats(model, what=("grad", "param"), seg_chunk=64)
    ps.update()                                                        # (binds, uploads the tables, allocates)
    torch.cuda.synchronize()
    copies = []
    real = torch.Tensor.copy_

    def counting(self, src, *a, **k):
        if src.is_cuda and not self.is_cuda:
            copies.append(src.numel())
        return real(self, src, *a, **k)

    monkeypatch.setattr(torch.Tensor, "copy_", counting)
    raised = None
    torch.cuda.set_sync_debug_mode("error")
    try:
        ps.update()
        ps.reset()
        ps.update()
        n0 = len(copies)
        snap = ps.read()                                               # a non-blocking copy and an event: nothing torch calls a sync
    except RuntimeError as e:
        raised = str(e)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert raised is None, raised
    assert n0 == 0 and len(copies) == 1 and ps.copies == 1
    for what, flat in (("grad", g.gflat), ("param", g.pflat)):
        s = snap[what]
        host = flat.cpu().numpy()
        assert s.names == [n for n, _ in sorted(model.named_parameters(), key=lambda np_: g.offsets[g._index[id(np_[1])]])]
        assert s.numel.tolist() == [p.numel() for p in g.params] and s.updates.tolist() == [1] * len(g.params)
        for i, (off, p) in enumerate(zip(g.offsets, g.params)):
            w = R.record(host[off:off + p.numel()])
            assert (int(s.amax_bits[i]), int(s.nonfinite[i]), int(s.zeros[i]), int(s.over_f16[i])) == \
                (w["amax_bits"], w["nonfinite"], w["zeros"], w["over_f16"]), (what, i)
            assert np.array_equal(s.hist[i], w["hist"]) and np.array_equal(s.hist_total[i], w["hist"])
            assert abs(s.sumsq[i] - w["sumsq"]) <= bound(64, -(-p.numel() // 64)) * w["sumsq"]


@pytest.fixture(scope="module")
def trained(golden, tmp_path_factory):
    """the small model after one training forward and backward, its fused optimizers, and ParamStats' tables of that state"""
    from vbg.optim import clip_grad_norm_
    from vbg.stats import ParamStats
    net = _net(tmp_path_factory.mktemp("param_stats"), "a", dev())
    opts = _fused_opts(net, dev())
    dbatch = to_dev(_e2e_inputs(golden("e2e.npz")), dev())
    random.seed(100)
    loss = net(*dbatch)
    loss.backward()
    ps = ParamStats(net, what=("grad", "param"))
    ps.update()
    snap = ps.read()
    total = clip_grad_norm_(list(opts), 1e30)                          # (a huge max_norm: nothing is scaled)
    return net, opts, ps, snap, total


def test_model_norms_names_and_total_norm(trained):
    from vbg.optim import SEG_CHUNK
    net, opts, ps, snap, total = trained
    homed = {n: p for n, p in net.named_parameters() if p.requires_grad and getattr(p, "_vbg_flat", None) is not None}
    for what in ("grad", "param"):
        s = snap[what]
        assert dict(zip(s.names, s.numel.tolist())) == {n: p.numel() for n, p in homed.items()} and len(s.names) == len(homed)
        assert s.nonfinite.sum() == 0 and s.offenders() == [] and s.updates.tolist() == [1] * len(s)
        exact, worst = [], 0.0
        for i, n in enumerate(s.names):
            t = (homed[n].grad if what == "grad" else homed[n].data).detach().cpu().contiguous().reshape(-1).numpy()
            ref = R.exact_sumsq(t)                                                 # (math.fsum's value: the exact sum rounded once)
            lim = bound(SEG_CHUNK, -(-t.size // SEG_CHUNK)) * ref
            assert abs(s.sumsq[i] - ref) <= lim, (what, n, s.sumsq[i], ref)
            assert s.norm[i] == math.sqrt(s.sumsq[i]) and float(s.amax[i]) == float(np.abs(t).max()) and int(s.zeros[i]) == int((t == 0).sum())
            exact.append(ref)
            worst = max(worst, bound(SEG_CHUNK, -(-t.size // SEG_CHUNK)))
        # total_norm(): the root of the parameters' sums added in double -- one more 2^-53 per parameter, half of it all on the root,
        # and the root's own rounding
        want = math.sqrt(math.fsum(exact))
        assert abs(s.total_norm() - want) <= ((worst + (len(s) + 2) * 2.0 ** -53) / 2 + 2 * 2.0 ** -53) * want, (what, s.total_norm(), want)
    # clip_grad_norm_ (vbg_sumsq: csrc/loss.hip sumsq_kernel on ew_grid(n, 1024) blocks of 256 threads): fp32 squares summed per thread
    # (a chain of L terms), over the block (10 additions), then one atomic addition per block into one fp32 word, for both buffers: at
    # most L + 10 + blocks roundings of 2^-24 on the sum, half of that on its root, and one more for the root's own rounding.  A
    # worst case over every order the atomics can arrive in, so far above what that kernel loses; the tight statement about
    # total_norm() is the one above, against the exact sum
    terms = 0
    for o in opts:
        n = o.group.total
        blocks = min(2048, -(-n // 1024))
        terms += -(-n // (blocks * 256)) + 10 + blocks
    got = snap["grad"].total_norm()
    assert got > 0 and abs(got - total) <= (terms / 2 + 1) * 2.0 ** -24 * got, (got, total)


def test_model_one_inf_names_one_offender_and_changes_no_other_row(trained):
    net, opts, ps, snap, _ = trained
    name = "late_fusion_net.fuse_embedding_net.linear.weight"
    p = dict(net.named_parameters())[name]
    flat, off = p._vbg_flat
    i = snap["grad"].names.index(name)
    keep = flat.gflat[off + 3].clone()
    flat.gflat[off + 3] = float("inf")
    ps.update()
    now = ps.read()
    flat.gflat[off + 3] = keep
    g0, g1 = snap["grad"], now["grad"]
    assert g1.offenders() == [name] and int(g1.nonfinite[i]) == 1 and g1.nonfinite.sum() == 1
    others = np.arange(len(g0)) != i
    for k in ("sumsq", "amax_bits", "nonfinite", "zeros", "over_f16", "hist"):
        assert np.array_equal(getattr(g0, k)[others], getattr(g1, k)[others]), k
    assert g1.steps_nonfinite.tolist() == [int(j == i) for j in range(len(g1))] and g1.updates.tolist() == [2] * len(g1)
    assert int(g1.hist[i].sum()) + int(g1.zeros[i]) == g0.numel[i] - 1 and g1.sumsq[i] <= g0.sumsq[i]
    for k in ("sumsq", "amax_bits", "hist"):                                       # the weights did not move
        assert np.array_equal(getattr(snap["param"], k), getattr(now["param"], k)), k


def test_model_scaler_reports_the_unscaled_norms(trained):
    from vbg.stats import ParamStats
    net, opts, ps, snap, _ = trained
    scaler = torch.amp.GradScaler("cuda", init_scale=65536.0)
    with pytest.raises(RuntimeError):                                              # no loss scaled yet: there is no device scale
        ParamStats(net, what=("grad",), scaler=scaler).update()
    scaler.scale(torch.ones(1, device=dev()))
    scaled = ParamStats(net, what=("grad",), scaler=scaler)
    plain = ParamStats(net, what=("grad",))
    groups = [o.group for o in opts]
    try:
        for g in groups:
            g.gflat.mul_(65536.0)                                                  # what scaler.scale(loss).backward() leaves: exact products
        scaled.update()
        plain.update()
    finally:
        for g in groups:
            g.gflat.mul_(1.0 / 65536.0)
    a, b, g0 = scaled.read()["grad"], plain.read()["grad"], snap["grad"]
    # a power of two, no gradient near either end of the range: unscaling gives the gradients back, bit for bit
    assert np.array_equal(a.sumsq, g0.sumsq) and np.array_equal(a.amax_bits, g0.amax_bits) and np.array_equal(a.hist, g0.hist)
    assert abs(a.total_norm() - g0.total_norm()) == 0.0
    nz = g0.sumsq > 0
    # without scaler= the same buffer reads 2^16 times larger: every sum of squares 2^32 times (exactly: powers of two), every binade
    # that is not clamped at either end 16 bins up
    assert nz.any() and np.array_equal(b.sumsq[nz], g0.sumsq[nz] * 65536.0 ** 2) and np.array_equal(b.hist[:, 17:63], g0.hist[:, 1:47])
