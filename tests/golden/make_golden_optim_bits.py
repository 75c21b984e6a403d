"""Generate tests/golden/optim_bits.npz: the bits that the gradient-norm row pass and its finish leave, recorded on the GPU.

    python tests/golden/make_golden_optim_bits.py [output file]

Needs a real MI355X and the built library.  Every call goes through the public wrappers of vbg.ops (grad_sumsq_seg, grad_sumsq_seg_inf,
grad_norm_seg, clip_coef, clip_coef_gate), so the script runs unchanged on any commit that has them: the committed fixture was written
by the commit BEFORE the two duplicate kernels were folded into grad_norm_seg_kernel / clip_coef_gate_kernel, and
tests/test_gpu_clip_gate.py::test_bits_of_the_recorded_calls replays `record` below against it.  The fixture is plain data
(allow_pickle=False) and holds its own inputs -- the gradients as bit patterns, the rows of the chunk tables -- so nothing depends on a
generator's version.

Table "runs": tests/test_gpu_optim_groups.py's RUNS cut at 64 (rows of 8 .. 64 elements) and at 4096 (one 4096-element row, four trips
per thread, among the short ones), NaN / 1e30 wherever no row covers.  Table "cap": 2050 rows of 8 elements, then one row of 4096 -- the
grid stops at 2048 blocks, so blocks 0 .. 2 take a second row, and block 2's is the long one: the smallest table on which the stride of
the row walk can go wrong."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

CANARY = 777.0
KINDS = (2, 1, 0)
# (max_norm, norm_scale, grad_scale): plain, a clip that does not bite, norm_scale 0.5, a power-of-two scale and one that is not
SETTINGS = ((1.0, 1.0, None), (1e7, 1.0, None), (2.0, 0.5, None), (0.37, 1.0, 1024.0), (0.37, 1.0, 1000.0))
GATES = ("none", "open64", "closed32")


def tables():
    """{table: (g0 fp32 [total] on the CPU, {cut: rows})}, from fixed seeds"""
    for d in ("oracle", "vibertgrid-pytorch_amd", "tests"):          # (what tests/conftest.py puts there for the tests)
        sys.path.insert(0, os.path.join(ROOT, d))
    from test_gpu_optim_groups import RUNS, TOTAL, cut, inside
    canary = torch.where(torch.arange(TOTAL) % 2 == 0, torch.full((), float("nan")), torch.full((), 1e30))
    ga = torch.where(inside(RUNS, TOTAL), torch.randn(TOTAL, generator=torch.Generator().manual_seed(150)), canary)
    nb = 2050 * 8 + 4096
    gb = torch.cat([torch.randn(nb, generator=torch.Generator().manual_seed(151)), canary[:8]])
    rows_b = [(8 * i, 8, i % 3) for i in range(2050)] + [(2050 * 8, 4096, 0)]
    return {"runs": (ga, {"64": cut(RUNS, 64), "4096": cut(RUNS, 4096)}), "cap": (gb, {"8": rows_b})}


def _u32(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy().view(np.uint32).copy()


def _gate(which, dev):
    if which == "open64":
        return (torch.tensor(12.5, dtype=torch.float64, device=dev), 10)
    if which == "closed32":
        return (torch.tensor([3.0], dtype=torch.float32, device=dev), 10)
    return None


def record(ops, dev, g0, rows):
    """every recorded call over one set of rows -> ({name: uint32 bits}, True when every canary around `partials` and `out` is intact and g
    holds what it held)"""
    n = len(rows)
    g = g0.to(dev)
    table = ops.chunk_table(rows, max(r[2] for r in rows) + 1, g0.numel(), dev)
    got, intact = {}, True

    def rows_of(name, call):
        nonlocal intact
        buf = torch.full((n + 16,), CANARY, device=dev)
        call(buf[8:8 + n])
        intact = intact and bool((buf[:8] == CANARY).all()) and bool((buf[8 + n:] == CANARY).all())
        got[name] = _u32(buf[8:8 + n])
        return buf[8:8 + n]

    def flagged(call):
        nonlocal intact
        flag = torch.zeros(1, device=dev)
        call(flag)
        intact = intact and float(flag) == 0.0          # (every covered element is finite)

    part = {}
    old = rows_of("sumsq", lambda p: ops.grad_sumsq_seg(g, table, p))
    rows_of("sumsq_inf", lambda p: flagged(lambda f: ops.grad_sumsq_seg_inf(g, table, p, f)))
    for kind in KINDS:
        part[kind] = rows_of(f"norm{kind}", lambda p: ops.grad_norm_seg(g, table, p, kind))
        rows_of(f"norm{kind}_inf", lambda p: flagged(lambda f: ops.grad_norm_seg(g, table, p, kind, f)))
    coef, gated = [], []
    for max_norm, norm_scale, scale in SETTINGS:
        sc = None if scale is None else torch.full((), scale, device=dev)
        buf = torch.full((8,), 5.0, device=dev)
        ops.clip_coef(old, n, max_norm, norm_scale, sc, out=buf[3:5])
        intact = intact and buf[:3].tolist() == [5.0] * 3 and buf[5:].tolist() == [5.0] * 3
        coef.append(_u32(buf[3:5]))
        for kind in KINDS:
            for which in GATES:
                buf = torch.full((9,), 5.0, device=dev)
                ops.clip_coef_gate(part[kind], n, max_norm, norm_scale, sc, kind=kind, gate=_gate(which, dev), out=buf[3:6])
                intact = intact and buf[:3].tolist() == [5.0] * 3 and buf[6:].tolist() == [5.0] * 3
                gated.append(_u32(buf[3:6]))
    got["coef"] = np.stack(coef)                                                            # [setting, 2]
    got["gate"] = np.stack(gated).reshape(len(SETTINGS), len(KINDS), len(GATES), 3)         # [setting, kind, gate, 3]
    return got, intact and bool(np.array_equal(_u32(g), _u32(g0)))


def main():
    tabs = tables()
    from vbg import ops
    dev = torch.device("cuda")
    arrs = {}
    for name, (g0, cuts) in tabs.items():
        arrs[f"g_{name}"] = _u32(g0)
        for c, rows in cuts.items():
            arrs[f"rows_{name}_{c}"] = np.asarray(rows, dtype=np.int64)
            got, intact = record(ops, dev, g0, rows)
            assert intact, (name, c)
            again, _ = record(ops, dev, g0, rows)
            assert all(np.array_equal(got[k], again[k]) for k in got), (name, c)          # the same bits on a second call
            for k in ("sumsq_inf", "norm2", "norm2_inf"):
                assert np.array_equal(got[k], got["sumsq"]), (name, c, k)
            arrs.update({f"{name}_{c}_{k}": v for k, v in got.items()})
            total, coef = got["coef"][0].view(np.float32)
            print(name, c, len(rows), "rows, total norm", float(total), "coefficient", float(coef), len(got), "arrays")
    assert not any(v.dtype == object for v in arrs.values())
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "optim_bits.npz")
    np.savez_compressed(out, **arrs)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
