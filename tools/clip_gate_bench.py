"""The conditional clip of the reference's fp32 step (`if train_loss > loss_clip_tresh: clip_grad_norm(...)`, pipeline/train_val_utils.py:
280-282) at the tail of the cfg2 batch-8 training step with FusedSGD / FusedAdamW:

  host-if      what bench.py does: AsyncScalar.get() after backward(), `val > 10` on the host, the synchronous clip_grad_norm_ (a second
               .item(), a scale pass) when it fires;
  gate         vbg.optim.clip_in_step(opts, 2.0, when=(loss.detach(), 10)): the decision, the norm and the coefficient stay on the
               device; the logged loss value is read after step() has returned;
  host-if-open / gate-open   the same two with threshold 0: the clip fires in every step;
  gate-closed  the gate with a threshold no loss reaches: what a gate that stays closed costs ...
  no-clip      ... against a step that does not clip at all (the loss still read after step()).

Per setting a fresh process (the settings alternating, `--procs` rounds), warmed up.  Per process:
  tail us   median over the timed steps of the host clock from backward() returning to the second step() returning: how long the tail
            keeps the host (for host-if that includes waiting for the device to finish the forward pass);
  step ms   wall clock of the timed steps, synchronised at both ends, per step;
  fired     the timed steps in which the clip was applied.
Without a GPU nothing is measured and the tool says so.

    python tools/clip_gate_bench.py [--out profiles/clip_gate.txt] [--procs 3] [--steps 20] [--warmup 5]"""
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
sys.path.insert(0, os.path.join(ROOT, "vibertgrid-pytorch_amd"))
sys.path.insert(0, ROOT)

SETTINGS = ("host-if", "gate", "host-if-open", "gate-open", "gate-closed", "no-clip")
THRESHOLDS = {"host-if": 10, "gate": 10, "host-if-open": 0, "gate-open": 0, "gate-closed": 1e30}
MAX_NORM = 2.0


def child(setting, steps, warmup):
    """one process; prints `TIME tail_us step_ms fired last_loss`"""
    import random

    import bench
    from vbg.batch import AsyncScalar, PackedBatch
    from vbg.optim import FusedAdamW, FusedSGD, clip_grad_norm_, clip_in_step, split_parameters
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(42)
    random.seed(42)
    tmp = tempfile.mkdtemp(prefix="vbg_clip_gate_")
    with contextlib.redirect_stdout(sys.stderr):
        net = bench.build_model(tmp, backbone="resnet_34_fpn_pretrained", vocab=bench.VOCAB, img=512, ncls=bench.NCLS, roberta=False)
    net = net.to(dev).train()
    cnn, bert = split_parameters(net)
    opt_cnn = FusedSGD(cnn, dev, lr=0.005, momentum=0.9, weight_decay=0.005)
    opt_bert = FusedAdamW(bert, dev, lr=5e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    opts = [opt_cnn, opt_bert]
    dbatch = PackedBatch.pack(*bench.synthetic_batch(8, 512, 512, 512, 128, bench.NCLS, bench.VOCAB, 1234)).to(dev)
    torch.cuda.synchronize()
    tails, totals, fired_host = [], [], [0]

    def step(timed):
        loss = net(*dbatch)
        val = AsyncScalar(loss)
        opt_cnn.zero_grad()
        opt_bert.zero_grad()
        loss.backward()
        t0 = time.perf_counter()
        if setting.startswith("host-if"):
            v = val.get()
            if v > THRESHOLDS[setting]:
                clip_grad_norm_(opts, MAX_NORM, 1.0)
                fired_host[0] += int(timed)
        elif setting != "no-clip":
            total = clip_in_step(opts, MAX_NORM, when=(loss.detach(), THRESHOLDS[setting]))
            if timed:
                totals.append(total)
        opt_cnn.step()
        opt_bert.step()
        t1 = time.perf_counter()
        if not setting.startswith("host-if"):
            v = val.get()          # (the reference logs the value every step: read here, behind the enqueued update)
        if timed:
            tails.append((t1 - t0) * 1e6)
        return v

    for _ in range(warmup):
        step(False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        last = step(True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    fired = fired_host[0] if setting.startswith("host-if") else sum(int(float(t) != 0.0) for t in totals)
    print(f"TIME {statistics.median(tails):.1f} {dt / steps * 1e3:.3f} {fired} {last:.4f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--procs", type=int, default=3, help="alternating processes per setting")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--child", default=None, help="one setting (one process of the measurement)")
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
        emit("clip gate: no GPU in this run -- NOT MEASURED (python tools/clip_gate_bench.py --out profiles/clip_gate.txt on an MI355X)")
        return finish(1)
    times = {s: [] for s in SETTINGS}
    for _ in range(a.procs):
        for s in SETTINGS:
            run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", s, "--steps", str(a.steps), "--warmup", str(a.warmup)],
                                 capture_output=True, text=True, timeout=300)
            if run.returncode != 0:          # (nothing more is started behind a process that failed)
                print(run.stderr[-4000:], file=sys.stderr, flush=True)
                return run.returncode
            for ln in run.stdout.splitlines():
                if ln.startswith("TIME "):
                    f = ln.split()
                    times[s].append((float(f[1]), float(f[2]), int(f[3]), float(f[4])))
    emit(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    emit("cfg2 batch-8 fp32 training step, FusedSGD + FusedAdamW, one GPU; the conditional clip of pipeline/train_val_utils.py:280-282 (threshold 10, max_norm 2)")
    emit("  host-if: AsyncScalar.get() + host `if` + clip_grad_norm_ (bench.py's tail);  gate: clip_in_step(when=(loss, 10));")
    emit("  host-if-open / gate-open: the same two with threshold 0 (the clip fires in every step);")
    emit("  gate-closed: clip_in_step(when=(loss, 1e30));  no-clip: no clip at all")
    emit(f"host clock; {a.steps} timed steps after {a.warmup}; {a.procs} alternating fresh processes per setting; one value per process")
    for col, name, fmt in ((0, "tail us (backward() returned -> step() returned, median)", "{:10.1f}"), (1, "step ms", "{:10.3f}"), (2, "fired", "{:10d}")):
        emit(f"  {name}")
        for s in SETTINGS:
            emit(f"    {s:<13} " + "  ".join(fmt.format(v[col]) for v in times[s]))
    med = {s: statistics.median(v[1] for v in times[s]) for s in SETTINGS}
    spread = {s: max(v[1] for v in times[s]) - min(v[1] for v in times[s]) for s in SETTINGS}
    emit(f"  step ms, medians over the processes: " + ", ".join(f"{s} {med[s]:.3f}" for s in SETTINGS))
    emit(f"  gate - host-if: {med['gate'] - med['host-if']:+.3f} ms (max - min of the host-if processes: {spread['host-if']:.3f} ms)")
    emit(f"  gate-open - host-if-open: {med['gate-open'] - med['host-if-open']:+.3f} ms (max - min of the host-if-open processes: {spread['host-if-open']:.3f} ms)")
    emit(f"  gate-closed - no-clip: {med['gate-closed'] - med['no-clip']:+.3f} ms (max - min of the no-clip processes: {spread['no-clip']:.3f} ms; of the host-if processes: {spread['host-if']:.3f} ms)")
    emit(f"  last loss of each process: " + ", ".join(f"{s} {times[s][-1][3]:.4f}" for s in SETTINGS))
    return finish(0)


if __name__ == "__main__":
    sys.exit(main())
