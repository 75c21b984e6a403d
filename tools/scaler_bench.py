"""vbg.optim.fuse_scaler against a plain torch.amp.GradScaler, at the sizes the product steps (tools/stock_optim_bench.py's GradScaler
mode: SGD over the 41.8 M-element CNN-shaped layout, AdamW over the 108.9 M-element bert-base layout, homed, gradients present, both
fused with amp_scaling=True, one shared scaler).  Timed from the end of backward() to the return of update():

    no clip :                                   scaler.step(sgd); scaler.step(adamw); scaler.update()
    clip    : clip_in_step([sgd, adamw], scaler=scaler); scaler.step(sgd); scaler.step(adamw); scaler.update()

each with a plain scaler (the base: what the loop does without fuse_scaler) and a fused one, in alternating processes, host us and
device us (two events) per iteration.  Every process also times the row-walk kernels alone on both buffers with device events --
vbg_grad_sumsq_seg, vbg_grad_sumsq_seg_inf, vbg_grad_unscale_check_seg with inv 1 (read-only) and with an inverse that stores -- and the two
conditions of DESIGN.md section 2.4 for variants of a kernel are checked per process and buffer: sumsq_inf <= 1.05 x sumsq, and the
read-only check no slower than sumsq beyond the spread of that process's own repeats.  Exits 1 when a condition fails.

    python tools/scaler_bench.py [--out FILE] [--procs 3] [--steps 20] [--warmup 5] [--reps 10] [--rounds 5]"""
import argparse
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vibertgrid-pytorch_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from optim_groups_bench import bert_named, cnn_named  # noqa: E402
from stock_optim_bench import ADAMW_KW, SGD_KW, real  # noqa: E402

SETTINGS = (("plain", "noclip"), ("fused", "noclip"), ("plain", "clip"), ("fused", "clip"))
BOUND = 1.05


def child(which, clip, steps, warmup, reps, rounds):
    """one process; prints `LOOP host_us device_us scaler_launches reused fallbacks` and `KERNEL buffer|label|bytes per element|us of
    each round ...`"""
    from vbg import ops
    from vbg import optim as vo
    dev = torch.device("cuda")
    sides = []
    for kind, meta in (("sgd", cnn_named()), ("adamw", bert_named())):
        nm = real(meta, dev, 1)
        group = vo.FlatGroup(nm, dev)
        cls, kw = (torch.optim.AdamW, ADAMW_KW) if kind == "adamw" else (torch.optim.SGD, SGD_KW)
        opt = vo.fuse(cls([p for _, p in nm], **kw), amp_scaling=True)
        scaled = torch.randn(group.total, device=dev, generator=torch.Generator(device=dev).manual_seed(2)) * (0.02 * 65536.0)
        sides.append((kind, group, opt, scaled))
    scaler = torch.amp.GradScaler("cuda", growth_interval=10 ** 9)          # (the scale stays at 65536: every iteration does the same work)
    if which == "fused":
        vo.fuse_scaler(scaler)
    opts = [opt for _, _, opt, _ in sides]
    x = torch.zeros((), device=dev)
    host, devt = [], []
    for it in range(warmup + steps):
        for _, group, _, scaled in sides:
            group.gflat.copy_(scaled)
        scaler.scale(x)                                                      # (backward's side of the iteration)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        t0 = time.perf_counter()
        if clip:
            vo.clip_in_step(opts, 2.0, scaler=scaler)
        for opt in opts:
            scaler.step(opt)
        scaler.update()
        t1 = time.perf_counter()
        e1.record()
        e1.synchronize()
        if it >= warmup:
            host.append((t1 - t0) * 1e6)
            devt.append(e0.elapsed_time(e1) * 1e3)
    for opt in opts:
        f_ = opt._vbg_fused
        f_.reconcile()
        assert f_.fallbacks == 0 and f_.launches == warmup + steps and f_.skipped == 0, f_.last_fallback
    fs = getattr(scaler, "_vbg_fused", None)
    n = warmup + steps
    if fs is not None:
        assert fs.fallbacks == 0 and (fs.launches, fs.reused) == ((0, 2 * n) if clip else (2 * n, 0)), (fs.launches, fs.reused, fs.last_fallback)
    print(f"LOOP {statistics.median(host):.1f} {statistics.median(devt):.1f} " + ("- - -" if fs is None else f"{fs.launches // n} {fs.reused // n} {fs.fallbacks}"),
          flush=True)
    # the row-walk kernels alone over the whole layout: `reps` back-to-back calls between two events, `rounds` times each, interleaved
    one, inv = torch.ones((), device=dev), torch.full((), 0.5, device=dev)          # (0.5: the repeats keep g in the normal range)
    for kind, group, opt, scaled in sides:
        table = opt._vbg_norm_table()[1]
        part, flag = torch.empty(table.n, device=dev), torch.zeros((), device=dev)
        calls = (("vbg_grad_sumsq_seg", 4, lambda: ops.grad_sumsq_seg(group.gflat, table, part)),
                 ("vbg_grad_sumsq_seg_inf", 4, lambda: ops.grad_sumsq_seg_inf(group.gflat, table, part, flag)),
                 ("vbg_grad_unscale_check_seg, inv 1", 4, lambda: ops.grad_unscale_check_seg(group.gflat, table, one, flag)),
                 ("vbg_grad_unscale_check_seg, inv 0.5", 8, lambda: ops.grad_unscale_check_seg(group.gflat, table, inv, flag)))
        us = {label: [] for label, _, _ in calls}
        for _ in range(rounds):
            for label, _, fn in calls:
                group.gflat.copy_(scaled)
                for _ in range(2):
                    fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                e1.synchronize()
                us[label].append(e0.elapsed_time(e1) / reps * 1e3)
        assert float(flag) == 0.0
        for label, nbytes, _ in calls:
            print(f"KERNEL {kind} {group.total}|{label}|{nbytes}|" + " ".join(f"{v:.2f}" for v in us[label]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--procs", type=int, default=3, help="alternating processes per setting")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--child", default=None, help="plain|fused,noclip|clip (one process of the measurement)")
    a = ap.parse_args()
    if a.child:
        which, clip = a.child.split(",")
        child(which, clip == "clip", a.steps, a.warmup, a.reps, a.rounds)
        return 0
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    loops = {s: [] for s in SETTINGS}
    kern = []          # per process: {(buffer, label): (bytes per element, [us per round])}
    for _ in range(a.procs):
        for s in SETTINGS:
            run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", ",".join(s), "--steps", str(a.steps), "--warmup", str(a.warmup),
                                  "--reps", str(a.reps), "--rounds", str(a.rounds)], capture_output=True, text=True, timeout=600)
            if run.returncode != 0:          # (nothing more is started behind a process that failed)
                print(run.stderr[-4000:], file=sys.stderr, flush=True)
                return run.returncode
            out = run.stdout
            k = {}
            for ln in out.splitlines():
                if ln.startswith("LOOP "):
                    loops[s].append(ln.split()[1:])
                elif ln.startswith("KERNEL "):
                    buf, label, nbytes, us = ln[7:].split("|")
                    k[(buf, label)] = (int(nbytes), [float(v) for v in us.split()])
            kern.append(k)
    emit(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    emit("GradScaler loop, cfg2's two optimizers (SGD over the CNN-shaped layout, AdamW over bert-base), homed, gradients present, both")
    emit("fuse(opt, amp_scaling=True), one shared scaler; timed from the end of backward() to the return of update():")
    emit("  no clip: scaler.step(sgd); scaler.step(adamw); scaler.update()        clip: clip_in_step([sgd, adamw], 2.0, scaler=scaler) first")
    emit(f"median of {a.steps} iterations after {a.warmup}; {a.procs} alternating processes per setting; the base is the plain torch.amp.GradScaler")
    med = {}
    for s in SETTINGS:
        r = loops[s]
        med[s] = (statistics.median(float(v[0]) for v in r), statistics.median(float(v[1]) for v in r))
        emit(f"  {s[0] + ' scaler, ' + s[1]:<22} host us: " + "  ".join(f"{float(v[0]):8.1f}" for v in r) + "    device us: " + "  ".join(f"{float(v[1]):8.1f}" for v in r)
             + ("" if s[0] == "plain" else f"    scaler launches / reused / fallbacks per iteration: {r[0][2]} / {r[0][3]} / {r[0][4]}"))
    for c in ("noclip", "clip"):
        p, f_ = med[("plain", c)], med[("fused", c)]
        spread = max(max(float(v[0]) for v in loops[(w, c)]) / min(float(v[0]) for v in loops[(w, c)]) for w in ("plain", "fused"))
        emit(f"  {c}: plain / fused (medians over the processes): host {p[0] / f_[0]:.3f}x, device {p[1] / f_[1]:.3f}x; widest max / min of one setting's processes (host): {spread:.3f}")
    emit(f"the row-walk kernels alone ({a.reps} back-to-back calls between two events, {a.rounds} rounds interleaved; every process), median us per call (GB/s), min .. max:")
    ok = True
    for key in sorted({k for d in kern for k in d}):
        emit(f"  {key[0]:<18} {key[1]}")
        for i, d in enumerate(kern):
            nbytes, us = d[key]
            m = statistics.median(us)
            emit(f"      process {i:2d}: {m:8.1f} ({nbytes * int(key[0].split()[1]) / m * 1e-3:5.0f})   {min(us):8.1f} .. {max(us):8.1f}")
    emit(f"conditions (per process and buffer): sumsq_inf / sumsq <= {BOUND}; check-only / sumsq <= the process's own spread of sumsq (max / min of its rounds)")
    for buf in sorted({k[0] for d in kern for k in d}):
        for i, d in enumerate(kern):
            base = d[(buf, "vbg_grad_sumsq_seg")][1]
            r_inf = statistics.median(d[(buf, "vbg_grad_sumsq_seg_inf")][1]) / statistics.median(base)
            r_chk = statistics.median(d[(buf, "vbg_grad_unscale_check_seg, inv 1")][1]) / statistics.median(base)
            spread = max(base) / min(base)
            good = r_inf <= BOUND and r_chk <= spread
            ok = ok and good
            emit(f"  {buf:<18} process {i:2d}: sumsq_inf / sumsq {r_inf:.3f}   check-only / sumsq {r_chk:.3f}   spread {spread:.3f}   {'ok' if good else 'FAILED'}")
    emit("conditions: " + ("all hold" if ok else "NOT all hold"))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
