"""Field decoding after the eval forward: the per-segment torch loop a caller of the reference runs today against
vbg.decode.field_strings, on the same [N, C] device tensor at C = 5 and N = 64, 256, 1024 (a receipt has a few hundred segments).

The loop is restated here in this tool's words with the device work the reference's call sites do per segment
(pipeline/train_val_utils.py:445-477): `pred[i].softmax(0)`, `.argmax(0)`, the score `p[k].item()`, and the class kept as a device
tensor that is compared with the previous one inside an `if` (a launch and a blocking read of its own); records are filed and the
winners picked as the reference does, joined with the " " + t rule.  Both paths end in host strings, so a host clock around the call
includes every device-to-host read.  One fresh process per (method, N), the settings alternating, each warmed up; per process the
median, minimum and maximum of `--steps` timed calls.  The tool also counts, in an untimed call, the aten operations each path
dispatches (torch's dispatcher: every kernel launch and every copy torch makes goes through one) and the library launches.
Both paths must return the same strings or the process fails.  Without a GPU nothing is measured and the tool says so.

    python tools/decode_latency.py [--out profiles/field_decode.txt] [--procs 3] [--steps 30] [--warmup 5]"""
import argparse
import collections
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vibertgrid-pytorch_amd"))

C_CLASSES = 5
SIZES = (64, 256, 1024)
METHODS = ("loop", "fused")
VIEWS = ("aten.select.int", "aten.alias.default", "aten.view.default", "aten.detach.default", "aten.t.default", "aten.reshape.default",
         "aten._unsafe_view.default", "aten.as_strided.default")


def make_input(n):
    """runs of 1..6 segments, a clear margin on every row's class (an ulp between two softmax implementations changes nothing)"""
    g = torch.Generator().manual_seed(n)
    classes = []
    while len(classes) < n:
        k = int(torch.randint(0, C_CLASSES, (1,), generator=g))
        classes += [k] * int(torch.randint(1, 7, (1,), generator=g))
    classes = classes[:n]
    x = torch.rand(n, C_CLASSES, generator=g) - 0.5
    x[torch.arange(n), torch.tensor(classes)] = 2.0 + 4.0 * torch.rand(n, generator=g)
    return x, [f"w{i}" + ("-" if i % 7 == 3 else "") for i in range(n)]


def loop_decode(pred, texts, num_classes):
    """what a caller does today: a handful of device operations and blocking reads per segment (the tool counts them)"""
    filed = [[] for _ in range(num_classes)]
    text, total, count, prev = "", 0.0, 0, -1
    last = pred.shape[0] - 1
    for i in range(pred.shape[0]):
        p = pred[i].softmax(dim=0)
        k = p.argmax(dim=0)
        s = p[k].item()
        if k == prev:
            text += texts[i] if text.endswith("-") else " " + texts[i]
            total += s
            count += 1
        else:
            if prev >= 0:
                filed[prev].append((text, total / count))
            text, total, count = texts[i], s, 1
        if i == last:
            filed[prev].append((text, total / count))
        prev = k
    out = []
    for recs in filed:
        top = None
        for r in recs:
            if top is None or r[1] > top[1]:
                top = r
        out.append("" if top is None else top[0])
    return out


def child(method, n, steps, warmup):
    """one process; prints `TIME median min max` (us) and `OPS name=count ...`"""
    from torch.utils._python_dispatch import TorchDispatchMode

    from vbg import decode, ops
    dev = torch.device("cuda")
    x, texts = make_input(n)
    pred = x.to(dev)
    fused = lambda: decode.field_strings(pred, C_CLASSES, (texts,), join="space_before")      # noqa: E731
    loop = lambda: loop_decode(pred, texts, C_CLASSES)                                         # noqa: E731
    assert fused() == loop(), "the two paths disagree"
    fn = fused if method == "fused" else loop
    us = []
    for it in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        if it >= warmup:
            us.append((t1 - t0) * 1e6)
    print(f"TIME {statistics.median(us):.1f} {min(us):.1f} {max(us):.1f}", flush=True)

    counts = collections.Counter()

    class Count(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            counts[str(func)] += 1
            return func(*args, **(kwargs or {}))

    real = ops.lib.vbg_field_decode

    def counted(*a):
        counts["vbg_field_decode"] += 1
        return real(*a)

    ops.lib.vbg_field_decode = counted
    with Count():
        fn()
    ops.lib.vbg_field_decode = real
    print("OPS " + " ".join(f"{k}={v}" for k, v in sorted(counts.items())), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--procs", type=int, default=3, help="alternating processes per setting")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--child", default=None, help="loop|fused,N (one process of the measurement)")
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
        emit("field decoding latency: no GPU in this run -- NOT MEASURED (python tools/decode_latency.py --out profiles/field_decode.txt on an MI355X)")
        return finish(1)
    times = {(m, n): [] for n in SIZES for m in METHODS}
    opsof = {}
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
                    elif ln.startswith("OPS "):
                        opsof[(m, n)] = dict((kv.rsplit("=", 1)[0], int(kv.rsplit("=", 1)[1])) for kv in ln.split()[1:])
    emit(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    emit(f"field decoding of one document, pred_label [N, {C_CLASSES}] on the device -> one string per class on the host (join: \" \" + t)")
    emit("  loop : the per-segment torch loop of the reference's call sites (softmax, argmax, score .item(), class compared as a device tensor)")
    emit("  fused: vbg.decode.field_strings (one vbg_field_decode launch, one copy of the [1, C] table of winners)")
    emit(f"host clock around the call (both end in host strings); median of {a.steps} calls after {a.warmup}; {a.procs} alternating fresh processes per setting")
    for n in SIZES:
        for m in METHODS:
            r = times[(m, n)]
            emit(f"  N {n:5d}  {m:<5}  median us: " + "  ".join(f"{v[0]:10.1f}" for v in r) + "    min .. max us: " + "  ".join(f"{v[1]:.1f} .. {v[2]:.1f}" for v in r))
        lo, fu = (statistics.median(v[0] for v in times[(m, n)]) for m in METHODS)
        spread = max(max(v[0] for v in times[(m, n)]) / min(v[0] for v in times[(m, n)]) for m in METHODS)
        emit(f"  N {n:5d}  loop / fused (medians over the processes): {lo / fu:.1f}x; widest max / min of one setting's process medians: {spread:.3f}")
    emit("operations per call (torch dispatcher counts of one untimed call; views and aliases launch nothing and are left out):")
    for n in SIZES:
        for m in METHODS:
            d = {k: v for k, v in opsof[(m, n)].items() if k not in VIEWS}
            emit(f"  N {n:5d}  {m:<5}  " + ", ".join(f"{k} x {v}" for k, v in sorted(d.items())))
    emit("  (aten._local_scalar_dense = one blocking device-to-host read; aten._to_copy in the fused path = the one copy of the table)")
    return finish(0)


if __name__ == "__main__":
    sys.exit(main())
