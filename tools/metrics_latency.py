"""Validation metrics after the eval forwards: the reference's path against vbg.metrics.SequenceMetrics, on the same device tensors, for
an "epoch" of DOCS documents of N segments each (C = 7, the FUNSD BIO tags; N = 64, 256, 1024).

The reference keeps every (pred_label, gt_label) pair of the epoch and scores them at its end (pipeline/train_val_utils.py:520,
:563-657; pipeline/criteria.py).  Its two paths are restated here in this tool's words, with the same device operations and the same
blocking reads:
  token   token_F1_criteria: a concatenation of the epoch, a truncation to integers, and per class four boolean-mask counts, each
          ending in a blocking read;
  entity  BIO_F1_criteria: per document an argmax and a blocking copy to a Python list for prediction and label, tag strings, then
          seqeval's entity walk and set intersection (tests/metrics_restate.py stands in for the package, which is not installed).
  fused   SequenceMetrics: reset() (one launch, inside the clock), one update (one vbg_seq_metrics launch, no host read) per document,
          then counts() -- the one device-to-host copy -- token_f1() and entity_scores(): BOTH results of the two paths above.
A host clock around the whole epoch (the device is idle at its start, and every path ends in host numbers, so every read is inside);
for `fused` the part spent in the updates and the part spent at the epoch's end are timed as well.  One fresh process per
(method, N), the settings alternating, each warmed up; per process the median, minimum and maximum of `--steps` timed epochs.  The
paths must agree on every count or the process fails.  Without a GPU nothing is measured and the tool says so.

    python tools/metrics_latency.py [--out profiles/seq_metrics.txt] [--procs 3] [--steps 20] [--warmup 3]"""
import argparse
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vibertgrid-pytorch_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

TAGS = {"O": 0, "B-HEADER": 1, "I-HEADER": 2, "B-QUESTION": 3, "I-QUESTION": 4, "B-ANSWER": 5, "I-ANSWER": 6}
C_CLASSES = len(TAGS)
DOCS = 32
SIZES = (64, 256, 1024)
METHODS = ("token", "entity", "fused")


def make_epoch(n):
    """DOCS documents: gt in runs of 1..6 segments, softmax scores whose argmax differs from gt on about one row in ten"""
    g = torch.Generator().manual_seed(n)
    docs = []
    for _ in range(DOCS):
        gt = []
        while len(gt) < n:
            gt += [int(torch.randint(0, C_CLASSES, (1,), generator=g))] * int(torch.randint(1, 7, (1,), generator=g))
        gt = torch.tensor(gt[:n])
        pred = torch.where(torch.rand(n, generator=g) < 0.1, torch.randint(0, C_CLASSES, (n,), generator=g), gt)
        x = torch.rand(n, C_CLASSES, generator=g) - 0.5
        x[torch.arange(n), pred] = 2.0 + 4.0 * torch.rand(n, generator=g)
        docs.append((x.softmax(1), gt.int()))
    return docs


def masked_count(trunc, rows, k, value):
    """how many of the masked rows hold `value` in column k: a boolean-mask gather, a comparison, an integer sum and ONE blocking read"""
    return (trunc[rows, k] == value).int().sum().item()


def ref_token(epoch):
    """the token path in this tool's words, with the device work the reference does: one concatenation of the epoch's scores and one
    of its labels, one truncation of the scores to integers, and per class one comparison of the labels and four masked counts (own
    rows holding 1 / other rows holding 0 / other rows holding 1 / own rows holding 0), each with a blocking read of its own"""
    scores = torch.cat([x for x, _ in epoch], dim=0)
    labels = torch.cat([gt for _, gt in epoch], dim=0)
    trunc = scores.int()
    cells = []
    for k in range(scores.shape[1]):
        own = labels == k
        cells.append([masked_count(trunc, rows, k, value) for rows, value in ((own, 1), (~own, 0), (~own, 1), (own, 0))])
    return cells


def tag_strings(classes, names):
    """a device vector of class indices -> host list of tag strings: a cast to int32, ONE blocking copy, a Python list"""
    return [names[k] for k in classes.int().cpu().tolist()]


def ref_entity(epoch):
    """the entity path in this tool's words, with the device work the reference does per document: an argmax over the classes, then
    prediction and label each brought to the host as lists of tag strings (two blocking copies); the entity walk and the per-type
    set intersection that the seqeval package would run on those lists are tests/metrics_restate.py's"""
    import metrics_restate as R
    names = {k: tag for tag, k in TAGS.items()}
    want, got = [], []
    for x, gt in epoch:
        got.append(tag_strings(x.argmax(dim=1), names))
        want.append(tag_strings(gt, names))
    return R.entity_counts(want, got)


def child(method, n, steps, warmup):
    """one process; prints `TIME median min max` (us per epoch) and, for fused, `PART updates end` (medians, us)"""
    from vbg import metrics
    dev = torch.device("cuda")
    epoch = [(x.to(dev), gt.to(dev)) for x, gt in make_epoch(n)]
    m = metrics.SequenceMetrics(C_CLASSES, TAGS)

    def fused():
        m.reset()
        t0 = time.perf_counter()
        for x, gt in epoch:
            m.update(x, gt)
        t1 = time.perf_counter()
        c = m.counts()
        m.token_f1()
        m.entity_scores("micro")
        return c, t1 - t0, time.perf_counter() - t1

    c = fused()[0]
    assert c.token.tolist() == ref_token(epoch), "token counts disagree"
    ent = ref_entity(epoch)
    assert {ty: c.entity[i].tolist() for i, ty in enumerate(m.types) if c.entity[i].any()} == ent, "entity counts disagree"
    fn = {"token": lambda: ref_token(epoch), "entity": lambda: ref_entity(epoch), "fused": fused}[method]
    us, upd, end = [], [], []
    for it in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        t1 = time.perf_counter()
        if it >= warmup:
            us.append((t1 - t0) * 1e6)
            if method == "fused":
                upd.append(r[1] * 1e6)
                end.append(r[2] * 1e6)
    print(f"TIME {statistics.median(us):.1f} {min(us):.1f} {max(us):.1f}", flush=True)
    if method == "fused":
        print(f"PART {statistics.median(upd):.1f} {statistics.median(end):.1f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--procs", type=int, default=3, help="alternating processes per setting")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--child", default=None, help="token|entity|fused,N (one process of the measurement)")
    a = ap.parse_args()
    if a.child:
        method, n = a.child.split(",")
        child(method, int(n), a.steps, a.warmup)
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
        emit("validation metrics latency: no GPU in this run -- NOT MEASURED (python tools/metrics_latency.py --out profiles/seq_metrics.txt on an MI355X)")
        return finish(1)
    times = {(m, n): [] for n in SIZES for m in METHODS}
    parts = {n: [] for n in SIZES}
    for _ in range(a.procs):
        for n in SIZES:
            for m in METHODS:
                run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", f"{m},{n}", "--steps", str(a.steps), "--warmup", str(a.warmup)],
                                     capture_output=True, text=True, timeout=300)
                if run.returncode != 0:          # (nothing more is started behind a process that failed)
                    print(run.stderr[-4000:], file=sys.stderr, flush=True)
                    return run.returncode
                for ln in run.stdout.splitlines():
                    if ln.startswith("TIME "):
                        times[(m, n)].append([float(v) for v in ln.split()[1:]])
                    elif ln.startswith("PART "):
                        parts[n].append([float(v) for v in ln.split()[1:]])
    emit(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    emit(f"validation metrics of an epoch of {DOCS} documents, pred_label [N, {C_CLASSES}] and gt_label [N] on the device -> counts on the host")
    emit("  token : token_F1_criteria's device work restated (concatenation, truncation, four masked counts with a blocking read each per class)")
    emit("  entity: BIO_F1_criteria's device work restated (argmax, two blocking copies to Python lists per document) + seqeval's entity walk restated in Python")
    emit("  fused : SequenceMetrics: reset (inside the clock), one vbg_seq_metrics launch per document, one copy at the end; gives BOTH results")
    emit(f"host clock around the epoch; median of {a.steps} epochs after {a.warmup}; {a.procs} alternating fresh processes per setting")
    for n in SIZES:
        for m in METHODS:
            r = times[(m, n)]
            emit(f"  N {n:5d}  {m:<6}  median us / epoch: " + "  ".join(f"{v[0]:10.1f}" for v in r) + "    min .. max: " + "  ".join(f"{v[1]:.1f} .. {v[2]:.1f}" for v in r))
        med = {m: statistics.median(v[0] for v in times[(m, n)]) for m in METHODS}
        upd, end = (statistics.median(v[i] for v in parts[n]) for i in (0, 1))
        spread = max(max(v[0] for v in times[(m, n)]) / min(v[0] for v in times[(m, n)]) for m in METHODS)
        emit(f"  N {n:5d}  per document: token {med['token'] / DOCS:.1f} us, entity {med['entity'] / DOCS:.1f} us, fused {med['fused'] / DOCS:.1f} us "
             f"(host time inside update, an enqueue: {upd / DOCS:.1f} us per document; epoch end -- the wait for the device, the copy, token_f1, entity_scores -- {end:.1f} us once)")
        emit(f"  N {n:5d}  (token + entity) / fused: {(med['token'] + med['entity']) / med['fused']:.1f}x; widest max / min of one setting's process medians: {spread:.3f}")
    return finish(0)


if __name__ == "__main__":
    sys.exit(main())
