"""What the crf mode's scored prediction path costs: ops.crf_posterior (Viterbi + log Z + marginals, one launch) and
crf_posterior followed by vbg.decode.decode_tags (a second launch and the one copy of the table of winners to the host), beside
ops.crf_viterbi alone -- what a crf-mode `inference()` pays today for a path without scores.  ntag 25 (23 tags + START / STOP), 64,
256 and 1024 rows per document, 1 and 8 documents per call; randn emissions, 2 * randn transitions.

Host clock around the call, the device idle before it and waited for after it (decode_tags ends in a host table, the other two in a
synchronize).  One fresh process per method, the methods alternating, `--procs` processes each: every setting is measured in that many
fresh processes; per process the median, minimum and maximum of `--steps` timed calls after `--warmup`.  The grid of every kernel here is
one wave per document, so the time is the serial chain: the tool also prints the slope between 256 and 1024 rows, the cost of one step.
Without a GPU nothing is measured and the tool says so.

    python tools/crf_posterior_latency.py [--out profiles/crf_posterior.txt] [--procs 3] [--steps 30] [--warmup 5]"""
import argparse
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vibertgrid-pytorch_amd"))

NTAG = 25
ROWS = (64, 256, 1024)
DOCS = (1, 8)
METHODS = ("viterbi", "posterior", "posterior+decode_tags")


def make_input(rows, ndoc):
    g = torch.Generator().manual_seed(rows + ndoc)
    em = torch.randn(rows * ndoc, NTAG, generator=g)
    trans = torch.randn(NTAG, NTAG, generator=g) * 2
    trans[NTAG - 2, :] = -10000
    trans[:, NTAG - 1] = -10000
    return em, trans, [rows * k for k in range(ndoc + 1)]


def child(method, steps, warmup):
    """one process, every shape; prints `TIME rows ndoc median min max` (us)"""
    from vbg import decode, ops
    dev = torch.device("cuda")
    # tags: "O", then B-k / I-k for 11 fields, START, STOP
    tags = {"O": 0}
    for k in range(11):
        tags[f"B-f{k}"], tags[f"I-f{k}"] = 1 + 2 * k, 2 + 2 * k
    tags["<START>"], tags["<STOP>"] = NTAG - 2, NTAG - 1
    table = decode.tag_table(tags, ["others"] + [f"f{k}" for k in range(11)])
    for rows in ROWS:
        for ndoc in DOCS:
            em, trans, off = make_input(rows, ndoc)
            emd, trd = em.to(dev), trans.to(dev)
            offd = torch.tensor(off, dtype=torch.int32, device=dev)

            def viterbi():
                ops.crf_viterbi(emd, offd, trd, NTAG - 2, NTAG - 1)
                torch.cuda.synchronize()

            def posterior():
                ops.crf_posterior(emd, offd, trd, NTAG - 2, NTAG - 1)
                torch.cuda.synchronize()

            def both():
                path, _, _, marg = ops.crf_posterior(emd, offd, trd, NTAG - 2, NTAG - 1)
                decode.decode_tags((marg, path), table, 12, thresh=0.5, doc_off=off)

            fn = {"viterbi": viterbi, "posterior": posterior, "posterior+decode_tags": both}[method]
            us = []
            for it in range(warmup + steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                t1 = time.perf_counter()
                if it >= warmup:
                    us.append((t1 - t0) * 1e6)
            print(f"TIME {rows} {ndoc} {statistics.median(us):.1f} {min(us):.1f} {max(us):.1f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--procs", type=int, default=3, help="alternating processes per method")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--child", default=None, help="one process of the measurement: " + " | ".join(METHODS))
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
        emit("crf posterior latency: no GPU in this run -- NOT MEASURED (python tools/crf_posterior_latency.py --out profiles/crf_posterior.txt on an MI355X)")
        return finish(1)
    times = {(m, r, d): [] for m in METHODS for r in ROWS for d in DOCS}
    for _ in range(a.procs):
        for m in METHODS:
            run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", m, "--steps", str(a.steps), "--warmup", str(a.warmup)],
                                 capture_output=True, text=True, timeout=300)
            if run.returncode != 0:          # (nothing more is started behind a process that failed)
                print(run.stderr[-4000:], file=sys.stderr, flush=True)
                return run.returncode
            for ln in run.stdout.splitlines():
                if ln.startswith("TIME "):
                    f = ln.split()
                    times[(m, int(f[1]), int(f[2]))].append([float(v) for v in f[3:]])
    emit(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    emit(f"linear-chain CRF, ntag {NTAG}: one call for `docs` documents of `rows` segments each, emissions on the device")
    emit("  viterbi              : ops.crf_viterbi -- what a crf-mode inference() runs today: a path, no scores")
    emit("  posterior            : ops.crf_posterior -- the same path and score + log Z + marginals [N, ntag], one launch")
    emit("  posterior+decode_tags: the above + vbg.decode.decode_tags (one more launch, one copy of the [docs, 12] table to the host)")
    emit(f"host clock around the call incl. the wait for the device; median of {a.steps} calls after {a.warmup}; {a.procs} alternating fresh processes per method")
    med = {}
    for r in ROWS:
        for d in DOCS:
            for m in METHODS:
                v = times[(m, r, d)]
                med[(m, r, d)] = statistics.median(x[0] for x in v)
                emit(f"  rows {r:5d} docs {d}  {m:<21}  median us: " + "  ".join(f"{x[0]:9.1f}" for x in v) + "    min .. max us: " +
                     "  ".join(f"{x[1]:.1f} .. {x[2]:.1f}" for x in v))
            base = med[("viterbi", r, d)]
            emit(f"  rows {r:5d} docs {d}  posterior / viterbi {med[('posterior', r, d)] / base:.2f}x   posterior+decode_tags / viterbi "
                 f"{med[('posterior+decode_tags', r, d)] / base:.2f}x   (medians over the processes)")
    emit("cost of one step of the serial chain, (t(1024 rows) - t(256 rows)) / 768, one document:")
    for m in METHODS[:2]:
        emit(f"  {m:<10} {(med[(m, 1024, 1)] - med[(m, 256, 1)]) / 768 * 1000:.0f} ns per row")
    return finish(0)


if __name__ == "__main__":
    sys.exit(main())
