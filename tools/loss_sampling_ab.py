"""Device sampling of the sampled / OHEM losses (VBG_DEVICE_SAMPLING, vbg.ops.set_device_sampling) against the host route, on the
benchmark's training step: cfg2 (resnet-34 + 12-layer BERT), batch 8 x 512 x 512, fp32 and under autocast.

One fresh process per (precision, switch), the settings alternating, `--procs` processes each, every process under its own `timeout`;
nothing more is started behind a process that failed.  Per process, after `--warmup` steps, over `--steps` steps:
  * ms per step: host clock over the timed steps with one synchronize at the end (forward, backward, both fused optimizers);
  * label prologue: host milliseconds from the first label kernel to the end of the plan construction (a host clock inside
    ViBERTgridNet._forward's label block, no synchronize), and the number of library launches + torch dispatches in it;
  * host wait inside `PendingCounts.finish()` (the event wait, the host draws, the upload and the gathers); 0 when no such object is built.
Without a GPU nothing is measured and the tool says so.

    python tools/loss_sampling_ab.py [--out profiles/device_sampling.txt] [--procs 3] [--steps 20] [--warmup 5]"""
import argparse
import contextlib
import os
import statistics
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vibertgrid-pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

PRECISIONS = ("fp32", "autocast")
SWITCH = ("off", "on")
VIEWS = ("aten.select.int", "aten.alias.default", "aten.view.default", "aten.detach.default", "aten.t.default", "aten.reshape.default",
         "aten._unsafe_view.default", "aten.as_strided.default", "aten.slice.Tensor", "aten.unsqueeze.default", "aten.expand.default")


def child(precision, switch, steps, warmup):
    """one process; prints `STEP ms`, `PROLOGUE ms launches`, `FINISH ms`"""
    import ctypes

    from torch.utils._python_dispatch import TorchDispatchMode

    import bench
    import pipeline.custom_loss as CL
    from vbg import lib as L
    from vbg import ops
    from vbg.batch import PackedBatch
    from vbg.optim import FusedAdamW, FusedSGD, split_parameters

    ops.set_device_sampling(switch == "on")
    dev = torch.device("cuda", 0)
    with contextlib.redirect_stdout(sys.stderr):
        torch.manual_seed(42)
        net = bench.build_model(tempfile.mkdtemp(prefix="vbg_sampling_ab_")).to(dev).train()
    cnn, bert = split_parameters(net)
    opts = [FusedSGD(cnn, dev, lr=0.005, momentum=0.9, weight_decay=0.005), FusedAdamW(bert, dev, lr=5e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)]
    batch = PackedBatch.pack(*bench.synthetic_batch(8, 512, 512, 512, 128, bench.NCLS, bench.VOCAB, 1234)).to(dev)

    # host clocks: the label block = seg_head.make_labels ... the last plan; PendingCounts.finish
    acc = {"prologue": 0.0, "finish": 0.0, "t0": None}
    seg, cls = net.semantic_segmentation_head, net.field_type_classification_head
    make_labels, cls_plans, finish = seg.make_labels, cls.plans, CL.PendingCounts.finish

    def timed_make_labels(*a, **k):
        acc["t0"] = time.perf_counter()
        return make_labels(*a, **k)

    def timed_cls_plans(*a, **k):
        r = cls_plans(*a, **k)
        acc["prologue"] += time.perf_counter() - acc["t0"]
        return r

    def timed_finish(self):
        t = time.perf_counter()
        finish(self)
        acc["finish"] += time.perf_counter() - t

    seg.make_labels, cls.plans, CL.PendingCounts.finish = timed_make_labels, timed_cls_plans, timed_finish

    def step():
        for o in opts:
            o.zero_grad()
        with (torch.autocast("cuda", dtype=torch.float16) if precision == "autocast" else contextlib.nullcontext()):
            loss = net(*batch)
        loss.backward()
        for o in opts:
            o.step()

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    acc["prologue"] = acc["finish"] = 0.0
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    pro, fin = acc["prologue"] * 1e3 / steps, acc["finish"] * 1e3 / steps

    # launches of the label block, in one untimed step: library entries called + torch dispatches that are not views
    counts = {"n": 0, "on": False}

    class Count(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            if counts["on"] and str(func) not in VIEWS:
                counts["n"] += 1
            return func(*args, **(kwargs or {}))

    class CountingLib:
        def __getattr__(self, name):
            fn = getattr(L.lib, name)
            if not isinstance(fn, ctypes._CFuncPtr) or name.endswith("_bytes"):
                return fn

            def call(*a):
                if counts["on"]:
                    counts["n"] += 1
                return fn(*a)
            return call

    def counting_make_labels(*a, **k):
        counts["on"] = True
        return make_labels(*a, **k)

    def counting_cls_plans(*a, **k):
        r = cls_plans(*a, **k)
        counts["on"] = False
        return r

    seg.make_labels, cls.plans = counting_make_labels, counting_cls_plans
    real = ops.lib
    ops.lib = CountingLib()
    try:
        with Count():
            step()
    finally:
        ops.lib = real
    torch.cuda.synchronize()
    print(f"STEP {ms:.3f}", flush=True)
    print(f"PROLOGUE {pro:.3f} {counts['n']}", flush=True)
    print(f"FINISH {fin:.3f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--procs", type=int, default=3, help="alternating processes per setting")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per process")
    ap.add_argument("--child", default=None, help="fp32|autocast,off|on (one process of the measurement)")
    a = ap.parse_args()
    if a.child:
        precision, switch = a.child.split(",")
        child(precision, switch, a.steps, a.warmup)
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
        emit("device sampling A/B: no GPU in this run -- NOT MEASURED (python tools/loss_sampling_ab.py --out profiles/device_sampling.txt on an MI355X)")
        return finish(1)
    res = {(p, s): [] for p in PRECISIONS for s in SWITCH}
    for _ in range(a.procs):
        for p in PRECISIONS:
            for s in SWITCH:
                cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", f"{p},{s}",
                       "--steps", str(a.steps), "--warmup", str(a.warmup)]
                run = subprocess.run(cmd, capture_output=True, text=True)
                if run.returncode != 0:          # (nothing more is started behind a process that failed)
                    print(run.stderr[-4000:], file=sys.stderr, flush=True)
                    emit(f"process {p},{s} ended with status {run.returncode}: measurement stopped")
                    return finish(run.returncode)
                got = {}
                for ln in run.stdout.splitlines():
                    w = ln.split()
                    if w and w[0] in ("STEP", "PROLOGUE", "FINISH"):
                        got[w[0]] = [float(v) for v in w[1:]]
                res[(p, s)].append(got)
                print(f"{p},{s}: {got}", file=sys.stderr, flush=True)
    emit(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    emit("cfg2 training step (resnet-34 + 12-layer BERT, batch 8 x 512 x 512; forward, backward, FusedSGD + FusedAdamW), device sampling off / on")
    emit(f"host clock; mean over {a.steps} steps after {a.warmup}; {a.procs} alternating fresh processes per setting, one value per process")
    for p in PRECISIONS:
        for s in SWITCH:
            r = res[(p, s)]
            emit(f"  {p:<8} switch {s:<3}  ms/step: " + "  ".join(f"{g['STEP'][0]:8.3f}" for g in r)
                 + "   label prologue host ms: " + "  ".join(f"{g['PROLOGUE'][0]:6.3f}" for g in r)
                 + f"   launches in it: {int(r[0]['PROLOGUE'][1])}"
                 + "   host ms in PendingCounts.finish: " + "  ".join(f"{g['FINISH'][0]:6.3f}" for g in r))
        off = [g["STEP"][0] for g in res[(p, "off")]]
        on = [g["STEP"][0] for g in res[(p, "on")]]
        emit(f"  {p:<8} median off {statistics.median(off):.3f} ms, on {statistics.median(on):.3f} ms "
             f"(on - off {statistics.median(on) - statistics.median(off):+.3f} ms; spread of the off processes {max(off) - min(off):.3f} ms, of the on processes {max(on) - min(on):.3f} ms)")
    return finish(0)


if __name__ == "__main__":
    sys.exit(main())
