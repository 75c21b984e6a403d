"""What the crf mode's training loss costs on its two routes, and how far each is from fp64: Fn.CrfNllFn (vbg_crf_nll_fwd +
vbg_crf_nll_bwd, the default) beside Fn.CrfNllStableFn (vbg_crf_nll_stable + vbg_crf_nll_stable_bwd, ops.set_crf_stable).

Timing    forward + backward of one call -- apply, (nll * w).sum().backward() -- at ntag 7 and 25, 64 / 256 / 1024 rows per document,
          1 and 8 documents; randn emissions, 2 * randn transitions.  Host clock around the call, the device idle before it and waited
          for after it.  One fresh process per route, the routes alternating, `--procs` processes each; per process the median, minimum
          and maximum of `--steps` timed calls after `--warmup`.
Accuracy  on the device, one document of 30 / 100 / 300 / 700 rows (ntag 14 at 30 rows, 27 beyond), gout = n so that the gradients are
          marginal-scale quantities: the largest share of the tolerance 1e-6 + 1e-4 * |fp64| any entry uses, the number of entries
          outside it and the largest absolute error, against tests/crf_nll_restate.py.
Without a GPU nothing is measured and the tool says so.

    python tools/crf_nll_bench.py [--out profiles/crf_nll_stable.txt] [--procs 3] [--steps 30] [--warmup 5]"""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vibertgrid-pytorch_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

NTAGS = (7, 25)
ROWS = (64, 256, 1024)
DOCS = (1, 8)
ROUTES = ("default", "stable")
ACCURACY = ((14, 30), (27, 100), (27, 300), (27, 700))


def make_input(ntag, rows, ndoc):
    g = torch.Generator().manual_seed(1000 * ntag + rows + ndoc)
    em = torch.randn(rows * ndoc, ntag, generator=g)
    trans = torch.randn(ntag, ntag, generator=g) * 2
    trans[ntag - 2, :] = -10000
    trans[:, ntag - 1] = -10000
    tags = torch.randint(0, ntag - 2, (rows * ndoc,), generator=g).int()
    return em, trans, tags, [rows * k for k in range(ndoc + 1)]


def route_fn(route):
    from vbg import functions as Fn
    return Fn.CrfNllStableFn if route == "stable" else Fn.CrfNllFn


def grads(route, em, trans, tags, off, w):
    dev = torch.device("cuda")
    emd, trd = em.to(dev).requires_grad_(True), trans.to(dev).requires_grad_(True)
    nll = route_fn(route).apply(emd, trd, tags.to(dev), torch.tensor(off, dtype=torch.int32, device=dev), trans.shape[0] - 2, trans.shape[0] - 1)
    (nll * w.to(dev)).sum().backward()
    torch.cuda.synchronize()
    return emd.grad.cpu().numpy().astype(np.float64), trd.grad.cpu().numpy().astype(np.float64)


def child(route, steps, warmup):
    """one process, every shape; prints `TIME ntag rows ndoc median min max` (us), then `ACC ntag rows which share outside total maxerr`"""
    import crf_nll_restate as R
    dev = torch.device("cuda")
    fn = route_fn(route)
    for ntag in NTAGS:
        for rows in ROWS:
            for ndoc in DOCS:
                em, trans, tags, off = make_input(ntag, rows, ndoc)
                emd, trd = em.to(dev).requires_grad_(True), trans.to(dev).requires_grad_(True)
                tgd, offd = tags.to(dev), torch.tensor(off, dtype=torch.int32, device=dev)
                w = torch.ones(ndoc, device=dev)
                us = []
                for it in range(warmup + steps):
                    emd.grad, trd.grad = None, None
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    (fn.apply(emd, trd, tgd, offd, ntag - 2, ntag - 1) * w).sum().backward()
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    if it >= warmup:
                        us.append((t1 - t0) * 1e6)
                print(f"TIME {ntag} {rows} {ndoc} {statistics.median(us):.1f} {min(us):.1f} {max(us):.1f}", flush=True)
    for ntag, rows in ACCURACY:
        em, trans, tags, off = make_input(ntag, rows, 1)
        gem, gtr = grads(route, em, trans, tags, off, torch.tensor([float(rows)]))
        _, _, wem, wtr = R.nll_and_grads(em.numpy(), tags.numpy(), trans.numpy(), ntag - 2, ntag - 1)
        for which, got, want in (("emissions", gem, wem), ("transitions", gtr, wtr)):
            err = np.abs(got - want)
            share = err / (1e-6 + 1e-4 * np.abs(want))
            print(f"ACC {ntag} {rows} {which} {float(share.max()):.3f} {int((share > 1).sum())} {share.size} {float(err.max()):.3e}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--procs", type=int, default=3, help="alternating processes per route")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--child", default=None, help="one process of the measurement: " + " | ".join(ROUTES))
    a = ap.parse_args()
    if a.child:
        child(a.child, a.steps, a.warmup)
        return 0
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def finish(rc):
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return rc

    if not torch.cuda.is_available():
        emit("crf nll routes: no GPU in this run -- NOT MEASURED (python tools/crf_nll_bench.py --out profiles/crf_nll_stable.txt on an MI355X)")
        return finish(1)
    times = {(m, t, r, d): [] for m in ROUTES for t in NTAGS for r in ROWS for d in DOCS}
    acc = {}
    for _ in range(a.procs):
        for m in ROUTES:
            run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", m, "--steps", str(a.steps), "--warmup", str(a.warmup)],
                                 capture_output=True, text=True, timeout=300)
            if run.returncode != 0:          # (nothing more is started behind a process that failed)
                print(run.stderr[-4000:], file=sys.stderr, flush=True)
                return finish(run.returncode)
            for ln in run.stdout.splitlines():
                f = ln.split()
                if ln.startswith("TIME "):
                    times[(m, int(f[1]), int(f[2]), int(f[3]))].append([float(v) for v in f[4:]])
                elif ln.startswith("ACC "):
                    acc.setdefault((m, int(f[1]), int(f[2]), f[3]), []).append((float(f[4]), int(f[5]), int(f[6]), float(f[7])))
    emit(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    emit("linear-chain CRF training loss, forward + backward of one call for `docs` documents of `rows` segments each")
    emit("  default: Fn.CrfNllFn       -- vbg_crf_nll_fwd + vbg_crf_nll_bwd (unnormalised alpha / beta, marginals as exp(alpha + beta - logZ))")
    emit("  stable : Fn.CrfNllStableFn -- vbg_crf_nll_stable + vbg_crf_nll_stable_bwd (re-centred vectors, pairwise tables divided by their own sums)")
    emit(f"host clock around apply + backward incl. the wait for the device; median of {a.steps} calls after {a.warmup}; {a.procs} alternating fresh processes per route")
    for t in NTAGS:
        for r in ROWS:
            for d in DOCS:
                med = {}
                for m in ROUTES:
                    v = times[(m, t, r, d)]
                    med[m] = statistics.median(x[0] for x in v)
                    emit(f"  ntag {t:2d} rows {r:5d} docs {d}  {m:<7}  median us: " + "  ".join(f"{x[0]:9.1f}" for x in v) + "    min .. max us: " +
                         "  ".join(f"{x[1]:.1f} .. {x[2]:.1f}" for x in v))
                emit(f"  ntag {t:2d} rows {r:5d} docs {d}  stable / default {med['stable'] / med['default']:.2f}x   (medians over the processes)")
    emit("accuracy on the device against fp64 (tests/crf_nll_restate.py), one document, gout = rows (marginal scale); tolerance 1e-6 + 1e-4 * |fp64| per entry:")
    emit("  largest share of the tolerance / entries outside it / largest absolute error; one figure where every process gave the same")
    for t, r in ACCURACY:
        for which in ("emissions", "transitions"):
            for m in ROUTES:
                v = acc[(m, t, r, which)]
                v = v[:1] if all(x == v[0] for x in v) else v
                emit(f"  ntag {t:2d} rows {r:4d}  {which:<11} {m:<7} " + "   ".join(f"{x[0]:8.3f} / {x[1]} of {x[2]} / {x[3]:.2e}" for x in v))
    return finish(0)


if __name__ == "__main__":
    sys.exit(main())
