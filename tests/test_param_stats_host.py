"""Per-parameter statistics, the host side (no GPU, no launch; the library itself must load): the numpy restatement pinned on
hand-written values, the row-table builder against brute force, the snapshot's helpers on synthetic tables, the ABI of the two new
structs and entries, and every argument error before a launch."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import param_stats_restate as R
from test_optim_groups_host import LAYOUT, OFFSETS, TOTAL
from vbg import stats as S
from weight_average_restate import homed_six

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUMELS = [1, 3, 4, 5, 7, 8, 9, 4095, 4096, 4097, 2 * 4096 + 1]
FAKE = 0x10000          # a non-NULL, aligned address that is never dereferenced: every case below fails its argument check first


# ---- the restatement on hand-written values ------------------------------------------------------------------------------------
def one(v, scale=None):
    return R.record(np.array([v], dtype=np.float32), scale)


def test_library_constants_are_the_restatements():
    """what vbg.stats reads the bins with is what the restatement fills them with"""
    assert S.HIST_BINS == R.BINS == 64 and S.HIST_E0 == -46 and S.F16_OVER == 65520.0
    assert int(np.float32(S.F16_OVER).view(np.uint32)) == R.F16_OVER_BITS
    # bin k holds [2^(k + HIST_E0), 2^(k + HIST_E0 + 1)): the first bin at or above 2^-14 / 2^-25 is where the two shares end
    assert int(R.bin_of(np.float32(2.0 ** -14))) == S.SUB_F16_BINS == -14 - S.HIST_E0
    assert int(R.bin_of(np.float32(2.0 ** -25))) == S.LOST_F16_BINS == -25 - S.HIST_E0
    for k in (1, 20, 21, 31, 32, 46, 62):
        assert int(R.bin_of(np.float32(2.0 ** (k + S.HIST_E0)))) == k == int(R.bin_of(R.below(2.0 ** (k + S.HIST_E0 + 1))))


def test_bin_rule_on_every_power_of_two_and_its_predecessor():
    for e in range(-149, 128):
        want = min(max(e + 46, 0), 63) if e >= -126 else 0          # fp32 subnormals (e < -126) count as exponent -127: bin 0
        for sign in (1.0, -1.0):
            r = one(sign * 2.0 ** e)
            assert r["hist"][want] == 1 and r["hist"].sum() == 1, e
            assert r["nonfinite"] == 0 and r["zeros"] == 0
            assert r["sumsq"] == (2.0 ** e) ** 2 and r["amax_bits"] == int(np.float32(2.0 ** e).view(np.uint32))
        if e > -149:
            low = min(max(e - 1 + 46, 0), 63) if e - 1 >= -126 else 0          # the largest fp32 below 2^e sits in the binade below
            r = one(R.below(2.0 ** e))
            assert r["hist"][low] == 1 and r["hist"].sum() == 1, e
    # bin k in 1..62 holds [2^(k-46), 2^(k-45)); bin 0 everything below 2^-45; bin 63 everything from 2^17 up
    assert one(2.0 ** -45)["hist"][1] == 1 and one(R.below(2.0 ** -45))["hist"][0] == 1
    assert one(2.0 ** 17)["hist"][63] == 1 and one(R.below(2.0 ** 17))["hist"][62] == 1 and one(3e38)["hist"][63] == 1


def test_fp16_edges():
    for v, over in ((65504.0, 0), (float(R.below(65520.0)), 0), (65520.0, 1), (65536.0, 1), (-65520.0, 1), (1e30, 1)):
        r = one(v)
        assert r["over_f16"] == over and r["nonfinite"] == 0, v
    assert one(65520.0)["hist"][61] == 1 and one(65536.0)["hist"][62] == 1
    sub = lambda r: int(r["hist"][:32].sum())            # noqa: E731  |v| < 2^-14: bins 0 .. 31
    lost = lambda r: int(r["hist"][:21].sum())           # noqa: E731  |v| < 2^-25: bins 0 .. 20
    assert sub(one(2.0 ** -14)) == 0 and sub(one(R.below(2.0 ** -14))) == 1
    assert lost(one(2.0 ** -25)) == 0 and lost(one(R.below(2.0 ** -25))) == 1
    assert lost(one(np.nextafter(np.float32(2.0 ** -25), np.float32(1)))) == 0 and sub(one(2.0 ** -25)) == 1


def test_zeros_nonfinite_and_subnormals_are_classified_not_summed():
    x = np.array([0.0, -0.0, np.inf, -np.inf, 3.0], dtype=np.float32)
    x = np.concatenate([x, np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0x00000001, 0x807FFFFF], dtype=np.uint32).view(np.float32)])
    r = R.record(x)
    assert r["zeros"] == 2 and r["nonfinite"] == 5 and r["over_f16"] == 0
    assert r["hist"].sum() == 3 and r["hist"][0] == 2 and r["hist"][47] == 1          # two subnormals, and 3.0 in [2, 4)
    assert r["amax_bits"] == int(np.float32(3.0).view(np.uint32))                      # finite elements only: no inf, no NaN pattern
    sub = np.array([0x00000001, 0x807FFFFF], dtype=np.uint32).view(np.float32).astype(np.float64)
    assert r["sumsq"] == math.fsum([9.0] + (sub * sub).tolist())
    assert R.record(sub.astype(np.float32))["sumsq"] == math.fsum((sub * sub).tolist()) > 0.0          # subnormals are summed, not flushed
    empty = R.record(np.array([np.nan, np.inf], dtype=np.float32))
    assert empty["sumsq"] == 0.0 and empty["amax_bits"] == 0 and empty["nonfinite"] == 2 and empty["hist"].sum() == 0


def test_unscale_is_one_fp32_product_with_the_inverse_formed_in_double():
    x = np.array([3.0, 1e-3, 65520.0 * 1000.0, 7e4, 2.0 ** -120, np.inf], dtype=np.float32)
    inv = np.float32(1.0 / 1000.0)
    v = R.unscaled(x, 1000.0)
    assert v.dtype == np.float32 and np.array_equal(v[:5], (x * inv)[:5])
    assert float(inv) == float(np.float32(1.0 / 1000.0)) and float(v[0]) == float(np.float32(np.float32(3.0) * inv))
    r = R.record(x, 1000.0)
    assert r["nonfinite"] == 1 and r["over_f16"] == int((np.abs(v[:5]) >= 65520.0).sum())
    assert r["sumsq"] == math.fsum((v[:5].astype(np.float64) ** 2).tolist())
    # a power-of-two scale moves binades exactly: 16 bins down for 65536
    a, b = R.record(np.array([1.0], dtype=np.float32)), R.record(np.array([1.0], dtype=np.float32), 65536.0)
    assert a["hist"][46] == 1 and b["hist"][30] == 1
    assert np.array_equal(R.unscaled(x, None), x)


def test_finish_and_running_table():
    x = R.mixed_values(1000, seed=3)
    whole = R.record(x)
    parts = R.finish([R.record(x[:64]), R.record(x[64:900]), R.record(x[900:])])
    assert all(np.array_equal(whole[k], parts[k]) for k in ("amax_bits", "nonfinite", "zeros", "over_f16", "hist"))
    assert abs(parts["sumsq"] - whole["sumsq"]) <= 4 * 2.0 ** -53 * whole["sumsq"]
    clean = R.record(np.ones(7, dtype=np.float32))
    t = R.fold(R.fold(R.fold(None, whole), clean), whole)
    assert t["updates"] == 3 and t["steps_nonfinite"] == 2 and t["nonfinite"] == 2 * whole["nonfinite"] and t["sumsq"] == whole["sumsq"]
    assert np.array_equal(t["hist"], 2 * whole["hist"] + clean["hist"]) and t["amax_bits"] == max(whole["amax_bits"], clean["amax_bits"])
    hv = R.record(R.hand_values())
    assert hv["nonfinite"] == 6 and hv["zeros"] == 2 and hv["hist"].sum() == len(R.hand_values()) - 8


def test_exact_sumsq_is_fsum_of_the_exact_squares():
    """the fast exact sum the model test uses for vectors of millions gives math.fsum's double, bit for bit"""
    rng = np.random.default_rng(11)
    cases = [R.hand_values(), R.mixed_values(5000, seed=4), R.mixed_values(1, seed=5), np.zeros(3, dtype=np.float32),
             (rng.standard_normal(200_000) * 1e-3).astype(np.float32), np.array([2.0 ** -149, -2.0 ** 127, 3.0], dtype=np.float32),
             np.full(70_000, np.float32(1.0) + np.float32(2.0 ** -23))]
    for x in cases:
        assert R.exact_sumsq(x) == R.record(x)["sumsq"], len(x)


# ---- the row table ------------------------------------------------------------------------------------------------------------
def check_rows(offsets, numels, total, chunk):
    from vbg import stats
    rows, row_ptr = stats.stats_rows(offsets, numels, chunk)
    want_rows, want_ptr = R.brute_rows(offsets, numels, chunk)
    assert rows.tolist() == [list(r) for r in want_rows] and row_ptr.tolist() == want_ptr
    covered = np.zeros(total, dtype=np.int64)
    for s, n, _ in rows:
        covered[s:s + n] += 1
    own = np.zeros(total, dtype=np.int64)
    for off, n in zip(offsets, numels):
        own[off:off + n] = 1
    assert np.array_equal(covered, own)                                            # each element once, the padding never
    assert (rows[:, 0] % 4 == 0).all() and (rows[:, 1] >= 1).all() and (rows[:, 1] <= chunk).all()
    assert np.array_equal(rows[:, 2], np.repeat(np.arange(len(numels)), np.diff(row_ptr)))          # consecutive per parameter
    assert (np.diff(rows[:, 0]) > 0).all() and row_ptr[0] == 0 and row_ptr[-1] == len(rows)
    return rows, row_ptr


@pytest.mark.parametrize("chunk", [64, 4096])
def test_row_table_against_brute_force(chunk):
    model, g = homed_six(LAYOUT, torch.device("cpu"))
    assert g.offsets == OFFSETS and g.total == TOTAL
    check_rows(g.offsets, [p.numel() for p in g.params], g.total, chunk)
    offsets, total = R.layout(NUMELS)
    rows, row_ptr = check_rows(offsets, NUMELS, total, chunk)
    assert len(rows) == sum((n + chunk - 1) // chunk for n in NUMELS)


def test_row_table_is_the_same_partition_for_both_chunks_and_is_checked():
    from vbg import ops, stats
    offsets, total = R.layout(NUMELS)
    tables = {}
    for chunk in (64, 4096):
        rows, row_ptr = stats.stats_rows(offsets, NUMELS, chunk)
        per = [rows[row_ptr[i]:row_ptr[i + 1]] for i in range(len(NUMELS))]
        tables[chunk] = [(int(r[0, 0]), int(r[:, 1].sum())) for r in per]          # (first element, element count) per parameter
        t = ops.stats_table(rows, row_ptr, total, torch.device("cpu"))
        assert (t.n, t.nparams, t.numel) == (len(rows), len(NUMELS), total) and t.rows.shape == (len(rows), 4) and t.row_ptr.dtype == torch.int32
    assert tables[64] == tables[4096] == list(zip(offsets, NUMELS))
    rows, row_ptr = stats.stats_rows(offsets, NUMELS, 64)
    cpu = torch.device("cpu")
    for bad_rows, bad_ptr in ((rows, row_ptr[:-1]), (rows[:-1], row_ptr), (rows[::-1], row_ptr), (rows + [[2, 0, 0]], row_ptr),
                              (rows + [[0, 0, 1]], row_ptr), (rows * [[1, 0, 1]], row_ptr)):
        with pytest.raises(ValueError):
            ops.stats_table(bad_rows, bad_ptr, total, cpu)
    with pytest.raises(ValueError):
        ops.stats_table(rows, row_ptr, total - 32, cpu)                            # the last float4 of a row outside the buffer
    # a row as long as the kernel's 32-bit element index allows, and one element more
    ops.stats_table([[0, (1 << 31) - 4, 0]], [0, 1], 1 << 31, cpu)
    with pytest.raises(ValueError):
        ops.stats_table([[0, (1 << 31) - 3, 0]], [0, 1], 1 << 32, cpu)
    for chunk in (0, 6, -4):
        with pytest.raises(ValueError):
            stats.stats_rows(offsets, NUMELS, chunk)
    with pytest.raises(ValueError):
        stats.stats_rows([0, 2], [1, 1], 64)
    with pytest.raises(ValueError):
        stats.stats_rows([0, 8], [1, 0], 64)


# ---- the snapshot's helpers -----------------------------------------------------------------------------------------------------
class Recorder:
    def __init__(self):
        self.calls = []

    def update(self, head="scalar", step=None, **kwargs):
        assert all(isinstance(v, (float, int)) for v in kwargs.values())          # (what TensorboardLogger.update asserts)
        self.calls.append((head, step, dict(kwargs)))


def synthetic():
    from vbg import stats
    names = ["enc.layer.0.q.weight", "enc.layer.0.q.bias", "enc.layer.1.q.weight", "head.weight", "head.bias"]
    numel = [100, 10, 100, 50, 5]
    data = [np.full(100, 3.0), np.r_[np.full(8, 1e-6), np.inf, np.nan], np.r_[np.full(99, 2.0 ** -26), 70000.0], np.r_[np.zeros(49), np.nan],
            np.full(5, -4.0)]
    last = np.zeros(5, dtype=stats.REC_DTYPE)
    total = np.zeros(5, dtype=stats.TOTAL_DTYPE)
    for i, d in enumerate(data):
        r = R.record(d.astype(np.float32))
        t = R.fold(R.fold(None, r), r)
        for k in ("sumsq", "amax_bits", "nonfinite", "zeros", "over_f16", "hist"):
            last[k][i] = r[k]
        for k in ("sumsq", "amax_bits", "nonfinite", "zeros", "over_f16", "hist", "updates", "steps_nonfinite"):
            total[k][i] = t[k]
    return stats.Snapshot.from_records(names, numel, last, total), data


def test_snapshot_helpers_on_a_synthetic_table():
    s, data = synthetic()
    assert s.norm[0] == 30.0 and s.amax[0] == 3.0 and s.amax[4] == 4.0 and s.amax.dtype == np.float32
    fin = np.concatenate([d[np.isfinite(d)] for d in data]).astype(np.float32).astype(np.float64)
    assert abs(s.total_norm() - math.sqrt(math.fsum(fin * fin))) <= 1e-15 * s.total_norm()
    assert s.offenders() == ["enc.layer.0.q.bias", "head.weight"]                  # 2 non-finite elements before 1
    assert s.nonfinite.tolist() == [0, 2, 0, 1, 0] and s.zeros.tolist() == [0, 0, 0, 49, 0]
    assert s.over_f16.tolist() == [0, 0, 1, 0, 0] and s.sub_f16.tolist() == [0, 8, 99, 0, 0] and s.lost_f16.tolist() == [0, 0, 99, 0, 0]
    assert s.updates.tolist() == [2] * 5 and s.steps_nonfinite.tolist() == [0, 2, 0, 2, 0] and np.array_equal(s.hist_total, 2 * s.hist)
    assert np.array_equal(s.amax_total, s.amax)
    fr = s.fp16_range()
    assert fr["names"] == s.names and fr["over"].tolist() == [0, 0, 0.01, 0, 0] and fr["sub"].tolist() == [0, 0.8, 0.99, 0, 0]
    assert fr["lost"].tolist() == [0, 0, 0.99, 0, 0]
    m = s.by_module(3)
    assert m.names == ["enc.layer.0", "enc.layer.1", "head.weight", "head.bias"] and m.numel.tolist() == [110, 100, 50, 5]
    assert m.sumsq[0] == s.sumsq[0] + s.sumsq[1] and m.nonfinite.tolist() == [2, 0, 1, 0] and m.amax[0] == 3.0
    assert np.array_equal(m.hist[0], s.hist[0] + s.hist[1]) and m.steps_nonfinite.tolist() == [2, 0, 2, 0]
    top = s.by_module(1)
    assert top.names == ["enc", "head"] and top.numel.tolist() == [210, 55] and top.amax.tolist() == [70000.0, 4.0]
    assert abs(top.total_norm() - s.total_norm()) <= 1e-15 * s.total_norm() and top.offenders() == ["enc", "head"]
    kinds = s.grouped(lambda n: n.rsplit(".", 1)[1])
    assert kinds.names == ["weight", "bias"] and kinds.numel.tolist() == [250, 15] and kinds.over_f16.tolist() == [1, 0]
    with pytest.raises(ValueError):
        s.by_module(0)


def test_log_calls_the_reference_loggers_signature():
    from vbg import stats
    s, _ = synthetic()
    ps = stats.ParamStats(torch.nn.Linear(2, 2), what=("grad",))
    rec = Recorder()
    out = ps.log(rec, "grad", depth=None, step=7, snap={"grad": s})
    assert out is s and [c[0] for c in rec.calls] == ["grad_norm", "grad_amax", "grad_nonfinite"] and all(c[1] == 7 for c in rec.calls)
    assert rec.calls[0][2] == {n: float(v) for n, v in zip(s.names, s.norm)} and rec.calls[2][2]["head.weight"] == 1.0
    rec = Recorder()
    ps.log(rec, "grad", depth=1, snap={"grad": s})
    assert list(rec.calls[0][2]) == ["enc", "head_"]                               # ("head" is the logger's own keyword)
    assert rec.calls[0][1] is None and rec.calls[1][2]["enc"] == 70000.0
    with pytest.raises(ValueError):
        ps.log(rec, "param", snap={"grad": s})
    for bad in ((), ("grad", "grad"), ("moment",)):
        with pytest.raises(ValueError):
            stats.ParamStats(torch.nn.Linear(2, 2), what=bad)
    with pytest.raises(ValueError):
        stats.ParamStats(torch.nn.Linear(2, 2), seg_chunk=6)
    with pytest.raises(ValueError):                                                # a model that is not homed
        stats.ParamStats(torch.nn.Linear(2, 2)).update()
    with pytest.raises(RuntimeError):
        stats.ParamStats(torch.nn.Linear(2, 2)).read()


# ---- ABI and argument errors ----------------------------------------------------------------------------------------------------
def test_struct_offsets_against_the_c_compiler(tmp_path):
    from vbg import stats
    from vbg.lib import StatsRec, StatsTotal
    structs = (("vbg_stats_rec", StatsRec, stats.REC_DTYPE), ("vbg_stats_total", StatsTotal, stats.TOTAL_DTYPE))
    # the two mirrors against each other and against the documented sizes: no compiler needed
    assert C.sizeof(StatsRec) == 288 and C.sizeof(StatsRec) % 16 == 0 and C.sizeof(StatsTotal) == 568
    for st, cls, dt in structs:
        assert C.sizeof(cls) == dt.itemsize and [n for n, _ in cls._fields_] == list(dt.names), st
        for name, _ in cls._fields_:
            assert getattr(cls, name).offset == dt.fields[name][1] and getattr(cls, name).size == dt.fields[name][0].itemsize, (st, name)
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    assert cc is not None, "no C compiler"
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "vbg.h"', 'int main(void) {']
    for st, cls, _ in structs:
        src.append(f'printf("{st} sizeof %zu\\n", sizeof({st}));')
        for name, _ in cls._fields_:
            src.append(f'printf("{st} {name} %zu\\n", offsetof({st}, {name}));')
    src += ['return 0; }']
    cfile = tmp_path / "off.c"
    cfile.write_text("\n".join(src))
    exe = str(tmp_path / "off")
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(cfile), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {(a, b): int(c) for a, b, c in (ln.split() for ln in out if ln)}
    for st, cls, dt in structs:
        assert got[(st, "sizeof")] == C.sizeof(cls), st
        for name, _ in cls._fields_:
            assert got[(st, name)] == getattr(cls, name).offset, (st, name)


def test_entries_are_declared_bound_and_exported():
    from vbg import lib as L
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vbg.h")).read(), flags=re.S)
    for name in ("vbg_param_stats_rows", "vbg_param_stats_finish"):
        assert re.search(r"\bint " + name + r"\(", src) and name in L.SIGNATURES and hasattr(L.lib, name)
    assert len(L.SIGNATURES["vbg_param_stats_rows"][1]) == 6 and len(L.SIGNATURES["vbg_param_stats_finish"][1]) == 6
    mk = open(os.path.join(ROOT, "vibertgrid-pytorch_amd", "csrc", "Makefile")).read()
    assert "stats.hip" in mk


def test_argument_errors_return_before_any_launch():
    from vbg import lib as L
    rows, fin = L.lib.vbg_param_stats_rows, L.lib.vbg_param_stats_finish
    # no-ops look at no pointer
    assert rows(None, None, 0, None, None, None) == 0 and fin(None, None, 0, None, None, None) == 0
    # negative counts
    assert rows(FAKE, FAKE, -1, None, FAKE, None) == -1 and fin(FAKE, FAKE, -1, FAKE, FAKE, None) == -1
    # NULL with a positive count (the scale and the running table may be NULL: checked with a NULL elsewhere)
    for args in ((None, FAKE, 1, None, FAKE), (FAKE, None, 1, None, FAKE), (FAKE, FAKE, 1, None, None)):
        assert rows(*args, None) == -1, args
    for args in ((None, FAKE, 1, FAKE, None), (FAKE, None, 1, FAKE, None), (FAKE, FAKE, 1, None, None), (None, FAKE, 1, FAKE, FAKE)):
        assert fin(*args, None) == -1, args
    # alignment: x / rows / recs / last 16 bytes, total 8, row_ptr and scale 4
    for args in ((FAKE + 4, FAKE, 1, None, FAKE), (FAKE, FAKE + 8, 1, None, FAKE), (FAKE, FAKE, 1, None, FAKE + 8), (FAKE, FAKE, 1, FAKE + 2, FAKE)):
        assert rows(*args, None) == -1, args
    for args in ((FAKE + 8, FAKE, 1, FAKE, None), (FAKE, FAKE + 2, 1, FAKE, None), (FAKE, FAKE, 1, FAKE + 8, None), (FAKE, FAKE, 1, FAKE, FAKE + 4)):
        assert fin(*args, None) == -1, args


def test_wrappers_refuse_what_the_host_can_see():
    """a row_ptr / table mismatch, short buffers and host memory are refused by the wrappers: an exception, no launch"""
    from vbg import ops, stats
    offsets, total = R.layout(NUMELS)
    rows, row_ptr = stats.stats_rows(offsets, NUMELS, 64)
    cpu = torch.device("cpu")
    t = ops.stats_table(rows, row_ptr, total, cpu)
    x = torch.zeros(total)
    recs = torch.zeros(t.n * ops.STATS_REC_BYTES, dtype=torch.uint8)
    last = torch.zeros(t.nparams * ops.STATS_REC_BYTES, dtype=torch.uint8)
    tot = torch.zeros(t.nparams * ops.STATS_TOTAL_BYTES, dtype=torch.uint8)
    with pytest.raises(ValueError):
        ops.param_stats_rows(x[:total - 32], t, recs)                              # the buffer is shorter than the table's
    with pytest.raises(ValueError):
        ops.param_stats_rows(x, t, recs[:-1])
    with pytest.raises(ValueError):
        ops.param_stats_rows(x, t, recs, scale=torch.zeros(2))
    with pytest.raises(ValueError):
        ops.param_stats_finish(recs, t, last[:-1], tot)
    with pytest.raises(ValueError):
        ops.param_stats_finish(recs, t, last, tot[:-1])
    short = ops.StatsTable(t.rows, t.row_ptr[:-1], t.n, t.nparams, t.numel)          # row_ptr does not match nparams
    with pytest.raises(ValueError):
        ops.param_stats_finish(recs, short, last, tot)
    with pytest.raises(TypeError):                                                 # host memory never reaches the library
        ops.param_stats_rows(x, t, recs)
    with pytest.raises(TypeError):
        ops.param_stats_finish(recs, t, last, tot)
