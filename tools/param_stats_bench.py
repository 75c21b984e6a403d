"""Per-parameter statistics (vbg_param_stats_rows / vbg_param_stats_finish, vbg.stats.ParamStats) at the sizes the product trains:
the two cfg2 flat buffers, 108 891 648 elements (bert-base, pooler left out) and 41 799 200 elements (CNN and heads), as a stand-in
model with those parameters homed in two FlatGroups (the shapes of tools/optim_groups_bench.py).

Measured on the host clock: per variant, perf_counter around REPS calls between two device synchronisations, every variant warmed
up, ROUNDS rounds that visit the variants in turn; median (min, max) per call.  Run it as three fresh processes and keep all three.

  yardstick      vbg_grad_norm_seg (kind 2) over both gradient buffers: the row pass that reads the same bytes with one fp32 sum
  rows           vbg_param_stats_rows over both gradient buffers (normal deviates; and the same with every element in ONE binade,
                 where all lanes of a wave add to the same slot of the LDS table; and with rows four times as long, a quarter of
                 the per-row folds and records)
  update         ParamStats.update() for what=("grad",) and for what=("grad", "param"): row passes plus finishes
  torch loop     what update() replaces: torch._foreach_norm over the per-parameter gradients, isfinite().all() per parameter, and
                 the two host reads
  host           host time of update() (nothing waited for) and of read() (one copy of every table, waited for)

    python tools/param_stats_bench.py [--out FILE] [--rounds 7] [--reps 5]"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vibertgrid-pytorch_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def clocked(variants, rounds, reps):
    """[(label, fn)] -> per variant the list over the rounds of microseconds per call on the host clock, the device drained on both sides"""
    for _, fn in variants:
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in variants]
    for _ in range(rounds):
        for i, (_, fn) in enumerate(variants):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            times[i].append((time.perf_counter() - t0) / reps * 1e6)
    return times


def host_only(fn, rounds, reps):
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        out.append((time.perf_counter() - t0) / reps * 1e6)
    torch.cuda.synchronize()
    return out


def fmt(t):
    return f"{statistics.median(t):9.1f} us  (min {min(t):9.1f}, max {max(t):9.1f})"


class Bag(torch.nn.Module):
    def __init__(self, named, device):
        super().__init__()
        g = torch.Generator(device=device).manual_seed(2)
        for n, p in named:
            self.register_parameter(n.replace(".", "_"), torch.nn.Parameter(torch.randn(tuple(p.shape), device=device, generator=g) * 0.02))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("param_stats_bench: needs the GPU (no timing is taken without one)")
    from optim_groups_bench import bert_named, cnn_named
    from vbg import ops
    from vbg.optim import SEG_CHUNK, FlatGroup, chunk_rows
    from vbg.stats import ParamStats
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda")
    nb, nc = [("bert_model." + n, p) for n, p in bert_named()], cnn_named()
    model = Bag(nb + nc, dev)
    named = list(model.named_parameters())
    groups = [FlatGroup(named[len(nb):], dev), FlatGroup(named[:len(nb)], dev)]
    gen = torch.Generator(device=dev).manual_seed(3)
    for g in groups:
        g.gflat.copy_(torch.randn(g.total, device=dev, generator=gen) * 1e-3)
    nbytes = 4.0 * sum(g.total for g in groups)
    emit(f"{torch.cuda.get_device_name(0)}; {a.rounds} rounds x {a.reps} calls per variant, variants visited in turn; host clock, median (min, max) per call")
    emit(f"stand-in model: {len(named)} parameters in two flat groups of {groups[1].total} and {groups[0].total} elements "
         f"({nbytes / 1e6:.0f} MB per quantity)")

    ps_g = ParamStats(model, what=("grad",))
    ps_gp = ParamStats(model, what=("grad", "param"))
    ps_g.update()
    ps_gp.update()
    groups = ps_g.groups                                   # (the order of the binding: every list below is in it)
    assert all(b.group is g for b, g in zip(ps_gp._bound, groups))
    emit(f"tables: {sum(b.table.n for b in ps_g._bound)} rows of at most {SEG_CHUNK} elements, {len(ps_g.names)} parameters; "
         f"output tables {ps_gp._out.numel() / 1e3:.0f} kB for two quantities")
    norm_tables = [ops.chunk_table(chunk_rows([(0, g.total, 0)], SEG_CHUNK), 1, g.total, dev) for g in groups]
    partials = [torch.empty(t.n, device=dev) for t in norm_tables]
    one_binade = [torch.full_like(g.gflat, 1.5e-3) for g in groups]
    grads = [p.grad for g in groups for p in g.params]

    def yardstick():
        for g, t, p in zip(groups, norm_tables, partials):
            ops.grad_norm_seg(g.gflat, t, p, 2)

    ps_wide = ParamStats(model, what=("grad",), seg_chunk=4 * SEG_CHUNK)
    ps_wide.update()

    def rows_only(bufs, ps=ps_g):
        def run():
            for b, x in zip(ps._bound, bufs):
                ops.param_stats_rows(x, b.table, b.recs)
        return run

    def finish_only():
        for b in ps_g._bound:
            ops.param_stats_finish(b.recs, b.ext, b.last, b.total)

    def torch_loop():
        norms = torch._foreach_norm(grads)
        fin = [t.isfinite().all() for t in grads]
        return torch.stack(norms).cpu(), torch.stack(fin).cpu()

    variants = [
        ("yardstick: vbg_grad_norm_seg kind 2, both buffers", yardstick),
        ("vbg_param_stats_rows, both buffers, normal deviates", rows_only([g.gflat for g in groups])),
        ("vbg_param_stats_rows, both buffers, one binade", rows_only(one_binade)),
        (f"vbg_param_stats_rows, both buffers, rows of {4 * SEG_CHUNK} (a quarter of the rows)", rows_only([g.gflat for g in groups], ps_wide)),
        ("vbg_param_stats_finish, both buffers", finish_only),
        (f"ParamStats.update() what=(grad,), seg_chunk={4 * SEG_CHUNK}", ps_wide.update),
        ("ParamStats.update() what=(grad,)", ps_g.update),
        ("ParamStats.update() what=(grad, param)", ps_gp.update),
        (f"torch loop: _foreach_norm + isfinite().all() x {len(grads)} + 2 host reads", torch_loop),
    ]
    times = clocked(variants, a.rounds, a.reps)
    yard = statistics.median(times[0])
    for (label, _), t in zip(variants, times):
        emit(f"  {label:<74} {fmt(t)}  x{statistics.median(t) / yard:5.2f} of the yardstick")
    emit(f"  rates: yardstick {nbytes / yard / 1e6:.2f} TB/s, row pass {nbytes / statistics.median(times[1]) / 1e6:.2f} TB/s")
    emit(f"  host time of update() what=(grad,), nothing waited for:        {fmt(host_only(ps_g.update, a.rounds, a.reps))}")
    emit(f"  host time of update() what=(grad, param), nothing waited for:  {fmt(host_only(ps_gp.update, a.rounds, a.reps))}")
    emit(f"  read() of an idle device (one copy of every table, waited for): {fmt(host_only(ps_gp.read, a.rounds, a.reps))}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
