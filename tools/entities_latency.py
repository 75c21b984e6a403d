"""What listing every field with its span posterior costs behind the crf mode's posterior: ops.crf_path_logp (the log marginal and
log conditional of every row of the Viterbi path, one launch) and vbg.decode.list_crf_fields (vbg_field_runs_tags: one launch and the
one copy of the per-row records to the host), beside ops.crf_posterior measured in the same processes.  ntag 25 (23 tags + START /
STOP), 64, 256 and 1024 segments per document, 1 and 8 documents per call; randn emissions, 2 * randn transitions.

Host clock around the call, the device idle before it and waited for after it (list_crf_fields ends in host arrays, the other two in a
synchronize).  `--procs` fresh processes, each measuring every method at every shape, the methods alternating shape by shape; per
process the median, minimum and maximum of `--steps` timed calls after `--warmup`.  path_logp repeats two of the posterior's three
chains (forward, backward; no Viterbi) on one wave per document, so its time is a serial chain too: the tool prints the slope between
256 and 1024 rows, the cost of one step, next to the posterior's.  There is no threshold to meet: the numbers stand next to each other
for the next reader.  Without a GPU nothing is measured and the tool says so.

    python tools/entities_latency.py [--out profiles/crf_entities.txt] [--procs 3] [--steps 30] [--warmup 5]"""
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
METHODS = ("posterior", "path_logp", "list_crf_fields", "all_three")


def make_input(rows, ndoc):
    g = torch.Generator().manual_seed(rows + ndoc)
    em = torch.randn(rows * ndoc, NTAG, generator=g)
    trans = torch.randn(NTAG, NTAG, generator=g) * 2
    trans[NTAG - 2, :] = -10000
    trans[:, NTAG - 1] = -10000
    return em, trans, [rows * k for k in range(ndoc + 1)]


def child(steps, warmup):
    """one process, every shape and method; prints `TIME method rows ndoc median min max` (us)"""
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
            path, _, _, marg = ops.crf_posterior(emd, offd, trd, NTAG - 2, NTAG - 1)
            lm, lc = ops.crf_path_logp(emd, offd, trd, NTAG - 2, NTAG - 1, path)
            torch.cuda.synchronize()

            def posterior():
                ops.crf_posterior(emd, offd, trd, NTAG - 2, NTAG - 1)
                torch.cuda.synchronize()

            def path_logp():
                ops.crf_path_logp(emd, offd, trd, NTAG - 2, NTAG - 1, path)
                torch.cuda.synchronize()

            def listing():
                decode.list_crf_fields((marg, path), (lm, lc), table, 12, thresh=0.5, doc_off=off)

            def all_three():
                p, _, _, m = ops.crf_posterior(emd, offd, trd, NTAG - 2, NTAG - 1)
                decode.list_crf_fields((m, p), ops.crf_path_logp(emd, offd, trd, NTAG - 2, NTAG - 1, p), table, 12, thresh=0.5, doc_off=off)

            for method, fn in zip(METHODS, (posterior, path_logp, listing, all_three)):
                us = []
                for it in range(warmup + steps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    t1 = time.perf_counter()
                    if it >= warmup:
                        us.append((t1 - t0) * 1e6)
                print(f"TIME {method} {rows} {ndoc} {statistics.median(us):.1f} {min(us):.1f} {max(us):.1f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--procs", type=int, default=3, help="fresh processes, each measuring every method")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--child", action="store_true", help="one process of the measurement")
    a = ap.parse_args()
    if a.child:
        child(a.steps, a.warmup)
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
        emit("crf entities latency: no GPU in this run -- NOT MEASURED (python tools/entities_latency.py --out profiles/crf_entities.txt on an MI355X)")
        return finish(1)
    times = {(m, r, d): [] for m in METHODS for r in ROWS for d in DOCS}
    for _ in range(a.procs):
        run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--steps", str(a.steps), "--warmup", str(a.warmup)],
                             capture_output=True, text=True, timeout=300)
        if run.returncode != 0:          # (nothing more is started behind a process that failed)
            print(run.stderr[-4000:], file=sys.stderr, flush=True)
            return run.returncode
        for ln in run.stdout.splitlines():
            if ln.startswith("TIME "):
                f = ln.split()
                times[(f[1], int(f[2]), int(f[3]))].append([float(v) for v in f[4:]])
    emit(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    emit(f"linear-chain CRF, ntag {NTAG}: one call for `docs` documents of `rows` segments each, emissions on the device")
    emit("  posterior      : ops.crf_posterior -- Viterbi path and score + log Z + marginals [N, ntag], one launch")
    emit("  path_logp      : ops.crf_path_logp -- lm, lc [N] of the Viterbi path: forward + backward chain, one launch")
    emit("  list_crf_fields: vbg.decode.list_crf_fields -- vbg_field_runs_tags (one launch) + one copy of the [N] records to the host")
    emit("  all_three      : what ViBERTgridNet.inference_entities runs behind the emissions in the crf mode")
    emit(f"host clock around the call incl. the wait for the device; median of {a.steps} calls after {a.warmup}; {a.procs} fresh processes, every method in each")
    med = {}
    for r in ROWS:
        for d in DOCS:
            for m in METHODS:
                v = times[(m, r, d)]
                med[(m, r, d)] = statistics.median(x[0] for x in v)
                emit(f"  rows {r:5d} docs {d}  {m:<15}  median us: " + "  ".join(f"{x[0]:9.1f}" for x in v) + "    min .. max us: " +
                     "  ".join(f"{x[1]:.1f} .. {x[2]:.1f}" for x in v))
            base = med[("posterior", r, d)]
            emit(f"  rows {r:5d} docs {d}  path_logp / posterior {med[('path_logp', r, d)] / base:.2f}x   all_three / posterior "
                 f"{med[('all_three', r, d)] / base:.2f}x   (medians over the processes)")
    emit("cost of one step of the serial chains, (t(1024 rows) - t(256 rows)) / 768, one document:")
    for m in METHODS[:2]:
        emit(f"  {m:<10} {(med[(m, 1024, 1)] - med[(m, 256, 1)]) / 768 * 1000:.0f} ns per row")
    return finish(0)


if __name__ == "__main__":
    sys.exit(main())
