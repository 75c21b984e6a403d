"""One step() of a stock torch.optim object over homed parameters, plain and after vbg.optim.fuse, with FusedAdamW / FusedSGD as the
floor, at the sizes the product steps: the bert-base AdamW buffer and a 41.8 M-element SGD buffer (the two layouts of
tools/optim_groups_bench.py, here with real parameters homed in a vbg.optim.FlatGroup).  Then the kernels alone: the segmented entries
with torch's options (vbg_adam_step_seg_opt / vbg_sgd_step_seg_opt) against vbg_adamw_step_seg / vbg_sgd_step_seg over the same
table -- bound set beforehand, as in profiles/optim_groups.txt: at most 1.05x.  Both pairs of entries launch ONE kernel per rule
(sgd_seg_kernel / adam_seg_kernel), so the `_seg` row and the `_opt`, flags 0 row time the same code through two entries; both rows
stay, as the measurement that the one kernel serves both (profiles/optim_seg_merge.txt).

Same protocol as that tool: one process, every variant warmed up, ROUNDS rounds that visit the variants in turn; per variant the
median, min and max over the rounds.  Reported per step() call: device time between two events around REPS back-to-back calls, and
host time of the call itself (perf_counter around it, device idle at the start).  `--e2e N` adds the stock-loop shape of
tests/test_gpu_train_loop.py (torch.optim.SGD + AdamW around the model on the e2e fixture) with and without fuse(), N alternating
processes each, milliseconds per step.

`--gradscaler N` measures GradScaler's two routes instead (nothing else runs then): cfg2's two optimizers -- AdamW over the bert-base
layout, SGD with momentum over the CNN-shaped one --, homed, gradients present, one shared torch.amp.GradScaler, and per iteration
`scaler.scale(x); scaler.step(sgd); scaler.step(adamw); scaler.update()`, with `fuse(opt)` and with `fuse(opt, amp_scaling=True)`, N
alternating processes per setting.  Per iteration (device idle at its start, the scaled gradients put back before it, outside the
timed window): host time of the four calls, device time between two events around them; then the step kernels alone, with their bytes
per second.

`--clip N` measures gradient-norm clipping in front of the step (nothing else runs then), on the same two optimizers, homed, gradients
present, N alternating processes per setting: `vbg.optim.clip_grad_norm_` + FusedSGD / FusedAdamW against `vbg.optim.clip_in_step` + the
same; `fuse(opt)` + torch.nn.utils.clip_grad_norm_ against `fuse(opt)` + clip_in_step; and the GradScaler loop with `unscale_` + torch's
clip against `clip_in_step(scaler=...)` on `fuse(opt, amp_scaling=True)` -- each with the clip biting (max_norm = norm / 2) and not
biting (2 x norm).  Per iteration (device idle at its start, the gradients put back before it, outside the timed window): host time of
the calls from the clip to the last step / update, device time between two events around them, and the device operations (kernels,
copies, memsets) one iteration issues, counted by torch.profiler in an iteration of its own after the timed ones.

    python tools/stock_optim_bench.py [--out FILE] [--rounds 9] [--reps 10] [--e2e 3]
    python tools/stock_optim_bench.py --gradscaler 3 [--out FILE] [--steps 20] [--warmup 5]
    python tools/stock_optim_bench.py --clip 3 [--out FILE] [--steps 20] [--warmup 5]"""
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

from optim_groups_bench import NO_DECAY, bert_named, cnn_named  # noqa: E402

ADAMW_KW = dict(lr=5e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
SGD_KW = dict(lr=0.005, momentum=0.9, weight_decay=0.005)


def real(named, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return [(n, torch.nn.Parameter(torch.randn(p.shape, device=dev, generator=g) * 0.02)) for n, p in named]


def decay_split(named):
    return [{"params": [p for n, p in named if not any(k in n for k in NO_DECAY)]},
            {"params": [p for n, p in named if any(k in n for k in NO_DECAY)], "weight_decay": 0.0}]


def optimizer_variants(kind, meta_named, dev):
    """[(label, step callable, FlatGroup)]: each variant on parameters and flat buffers of its own"""
    from vbg import optim as vo
    cls, kw = (torch.optim.AdamW, ADAMW_KW) if kind == "adamw" else (torch.optim.SGD, SGD_KW)
    name = cls.__name__
    out = []
    for label, build in ((f"torch.optim.{name}, one group", lambda nm: cls([p for _, p in nm], **kw)),
                         (f"torch.optim.{name}, decay split", lambda nm: cls(decay_split(nm), **kw)),
                         (f"fuse(torch.optim.{name}), one group", lambda nm: vo.fuse(cls([p for _, p in nm], **kw))),
                         (f"fuse(torch.optim.{name}), decay split", lambda nm: vo.fuse(cls(decay_split(nm), **kw))),
                         (f"fuse(torch.optim.{name}(amsgrad / nesterov)), decay split",
                          lambda nm: vo.fuse(cls(decay_split(nm), **kw, **({"amsgrad": True} if kind == "adamw" else {"nesterov": True})))),
                         (f"Fused{name} (whole-range launch)", None)):
        nm = real(meta_named, dev, 1)
        if build is None:
            opt = (vo.FusedAdamW if kind == "adamw" else vo.FusedSGD)(nm, dev, **{k: v for k, v in kw.items()})
            group = opt.group
        else:
            group = vo.FlatGroup(nm, dev)
            opt = build(nm)
        group.gflat.normal_(0.0, 0.02, generator=torch.Generator(device=dev).manual_seed(2))
        out.append((label, opt.step, group, opt))
    return out


def kernel_variants(kind, group, dev):
    """the entries alone over the decay-split table of `group`'s layout: old segmented, new with flags 0, new with every option"""
    from vbg import ops
    from vbg.optim import SEG_CHUNK, chunk_rows, run_table
    group_of = {id(p): int(any(k in n for k in NO_DECAY)) for n, p in zip(group.names, group.params)}
    table = ops.chunk_table(chunk_rows(run_table(group, group_of), SEG_CHUNK), 2, group.total, dev)
    n = group.total
    g = torch.Generator(device=dev).manual_seed(3)
    bufs = [torch.randn(n, device=dev, generator=g) * 0.02 for _ in range(5 if kind == "adamw" else 3)]
    for b in bufs[3:]:
        b.abs_()
    if kind == "adamw":
        hp = (5e-5, 0.9, 0.999, 1e-8, 0.01)
        return [("vbg_adamw_step_seg, decay split", lambda: ops.adamw_step_seg(*bufs[:4], table, [hp] * 2, 3, 1.0)),
                ("vbg_adam_step_seg_opt, flags 0", lambda: ops.adam_step_seg_opt(*bufs[:4], None, table, [hp + (3, 0)] * 2, 1.0)),
                ("vbg_adam_step_seg_opt, coupled + maximize", lambda: ops.adam_step_seg_opt(*bufs[:4], None, table, [hp + (3, 6)] * 2, 1.0)),
                ("vbg_adam_step_seg_opt, amsgrad (32 B per element)", lambda: ops.adam_step_seg_opt(*bufs, table, [hp + (3, 1)] * 2, 1.0))]
    hp = (0.005, 0.9, 0.005)
    return [("vbg_sgd_step_seg, decay split", lambda: ops.sgd_step_seg(*bufs, table, [hp] * 2, False, 1.0)),
            ("vbg_sgd_step_seg_opt, flags 0", lambda: ops.sgd_step_seg_opt(*bufs, table, [(0.005, 0.9, 0.0, 0.005, 0)] * 2, 1.0)),
            ("vbg_sgd_step_seg_opt, nesterov + dampening", lambda: ops.sgd_step_seg_opt(*bufs, table, [(0.005, 0.9, 0.1, 0.005, 1)] * 2, 1.0)),
            ("vbg_sgd_step_seg_opt, momentum 0 (12 B per element)", lambda: ops.sgd_step_seg_opt(*bufs, table, [(0.005, 0.0, 0.0, 0.005, 2)] * 2, 1.0))]


def timed(variants, rounds, reps, emit, base_label):
    for _, fn in variants:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    dev_t, host_t = [[] for _ in variants], [[] for _ in variants]
    for _ in range(rounds):
        for i, (_, fn) in enumerate(variants):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            t1 = time.perf_counter()
            e1.record()
            e1.synchronize()
            dev_t[i].append(e0.elapsed_time(e1) / reps * 1e3)
            host_t[i].append((t1 - t0) / reps * 1e6)
    base = next(statistics.median(t) for (label, _), t in zip(variants, dev_t) if label == base_label)
    res = {}
    for (label, _), d, h in zip(variants, dev_t, host_t):
        us = statistics.median(d)
        res[label] = us
        emit(f"  {label:<62} device {us:8.1f} us (min {min(d):8.1f}, max {max(d):8.1f})  x{us / base:6.3f}   host {statistics.median(h):8.1f} us (min {min(h):7.1f}, max {max(h):8.1f})")
    return res


def measure(kind, meta_named, rounds, reps, emit):
    dev = torch.device("cuda")
    name = "AdamW" if kind == "adamw" else "SGD"
    opts = optimizer_variants(kind, meta_named, dev)
    for label, _, group, opt in opts:
        fs = getattr(opt, "_vbg_fused", None)
        if fs is not None:                   # the fused objects must be on the fused path for what follows to mean anything
            opt.step()
            assert (fs.launches, fs.fallbacks) == (1, 0), (label, fs.last_fallback)
    emit(f"  {len(opts[0][2].params)} parameters, {opts[0][2].total} elements in the buffer; x = device time over the plain one-group torch step")
    timed([(label, step) for label, step, _, _ in opts], rounds, reps, emit, f"torch.optim.{name}, one group")
    emit("  the entries alone, decay-split table; x = device time over the existing segmented entry")
    kv = kernel_variants(kind, opts[0][2], dev)
    res = timed(kv, rounds, reps, emit, kv[0][0])
    ratio = res[kv[1][0]] / res[kv[0][0]]
    emit(f"  default case of the new entry / existing segmented entry: x{ratio:.3f} (bound 1.05)")
    return ratio <= 1.05


def e2e_child(mode, steps, warmup):
    """the stock loop of tests/test_gpu_train_loop.py on the e2e fixture; prints milliseconds per step"""
    import random
    import tempfile
    import numpy as np
    for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
        sys.path.insert(0, p)
    from test_gpu_model import build_product, load_synth, to_dev
    from test_oracle_golden import _e2e_inputs, e2e_cfg
    from vbg import optim as vo
    dev = torch.device("cuda")
    cfg = e2e_cfg("resnet_18_fpn")
    net = build_product(tempfile.mkdtemp(prefix="vbg_stock_"), "resnet_18_fpn", cfg)
    load_synth(net, cfg, 1200)
    net = net.to(dev).train()
    batch = to_dev(_e2e_inputs(np.load(os.path.join(ROOT, "tests", "golden", "e2e.npz"))), dev)
    oc = torch.optim.SGD([p for n, p in net.named_parameters() if "bert_model" not in n], **SGD_KW)
    ob = torch.optim.AdamW([p for n, p in net.named_parameters() if "bert_model" in n], **ADAMW_KW)
    if mode == "fuse":
        oc, ob = vo.fuse(oc), vo.fuse(ob)
    for step in range(warmup + steps):
        if step == warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        random.seed(100 + step)
        loss = net(*batch)
        oc.zero_grad()
        ob.zero_grad()
        loss.backward()
        oc.step()
        ob.step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    if mode == "fuse":
        for o in (oc, ob):
            assert o._vbg_fused.fallbacks == 0 and o._vbg_fused.launches == warmup + steps, o._vbg_fused.last_fallback
    print(f"E2E {mode} {ms:.3f}", flush=True)


def e2e(n, steps, warmup, emit):
    res = {"fuse": [], "plain": []}
    for _ in range(n):
        for mode in ("fuse", "plain"):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--e2e-child", mode, "--steps", str(steps), "--warmup", str(warmup)],
                                 check=True, capture_output=True, text=True, timeout=300).stdout
            res[mode].append(float([ln for ln in out.splitlines() if ln.startswith("E2E ")][-1].split()[2]))
    emit(f"stock loop on the e2e fixture (resnet_18_fpn, 2 documents), {steps} steps after {warmup}, ms per step, {n} alternating processes each:")
    emit("  with fuse()   : " + "   ".join(f"{v:7.2f}" for v in res["fuse"]))
    emit("  plain         : " + "   ".join(f"{v:7.2f}" for v in res["plain"]))


def gradscaler_child(amp, steps, warmup, reps):
    """one process of the GradScaler mode; prints `GS <amp> host_us device_us launches fallbacks skipped` and the kernels' rates"""
    from vbg import ops
    from vbg import optim as vo
    dev = torch.device("cuda")
    sides = []
    for kind, meta in (("sgd", cnn_named()), ("adamw", bert_named())):
        nm = real(meta, dev, 1)
        group = vo.FlatGroup(nm, dev)
        cls, kw = (torch.optim.AdamW, ADAMW_KW) if kind == "adamw" else (torch.optim.SGD, SGD_KW)
        opt = vo.fuse(cls([p for _, p in nm], **kw), amp_scaling=amp)
        scaled = torch.randn(group.total, device=dev, generator=torch.Generator(device=dev).manual_seed(2)) * (0.02 * 65536.0)
        sides.append((kind, group, opt, scaled))
    scaler = torch.amp.GradScaler("cuda", growth_interval=10 ** 9)          # (the scale stays at 65536: every iteration does the same work)
    x = torch.zeros((), device=dev)
    host, devt = [], []
    for it in range(warmup + steps):
        for _, group, _, scaled in sides:
            group.gflat.copy_(scaled)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        t0 = time.perf_counter()
        scaler.scale(x)
        for _, _, opt, _ in sides:
            scaler.step(opt)
        scaler.update()
        t1 = time.perf_counter()
        e1.record()
        e1.synchronize()
        if it >= warmup:
            host.append((t1 - t0) * 1e6)
            devt.append(e0.elapsed_time(e1) * 1e3)
    fs = [opt._vbg_fused for _, _, opt, _ in sides]
    for f_ in fs:
        f_.reconcile()
        assert f_.fallbacks == 0 and f_.launches == warmup + steps and f_.skipped == 0, f_.last_fallback
    print(f"GS {int(amp)} {statistics.median(host):.1f} {statistics.median(devt):.1f} {sum(f_.launches for f_ in fs) // (warmup + steps)} "
          f"{sum(f_.fallbacks for f_ in fs)} {sum(f_.skipped for f_ in fs)}", flush=True)
    # the step kernels alone, one group over the whole layout: REPS back-to-back calls between two events
    one, zero = torch.ones((), device=dev), torch.zeros((), device=dev)
    for kind, group, opt, scaled in sides:
        table = opt._vbg_fused.table(tuple([0] * len(group.params)), 1)
        st = [opt._vbg_fused.flat[k] for k in (("momentum_buffer",) if kind == "sgd" else ("exp_avg", "exp_avg_sq"))]
        if kind == "sgd":
            hp = [(0.005, 0.9, 0.0, 0.005, 0)]
            calls = (("vbg_sgd_step_seg_opt", 20, lambda: ops.sgd_step_seg_opt(group.pflat, group.gflat, st[0], table, hp, 1.0)),
                     ("vbg_sgd_step_seg_amp", 24, lambda: ops.sgd_step_seg_amp(group.pflat, group.gflat, st[0], table, hp, one, zero)),
                     ("vbg_sgd_step_seg_amp, found_inf set", 0, lambda: ops.sgd_step_seg_amp(group.pflat, group.gflat, st[0], table, hp, one, one)))
        else:
            hp = [(5e-5, 0.9, 0.999, 1e-8, 0.01, 3, 0)]
            calls = (("vbg_adam_step_seg_opt", 28, lambda: ops.adam_step_seg_opt(group.pflat, group.gflat, st[0], st[1], None, table, hp, 1.0)),
                     ("vbg_adam_step_seg_amp", 32, lambda: ops.adam_step_seg_amp(group.pflat, group.gflat, st[0], st[1], None, table, hp, one, zero)),
                     ("vbg_adam_step_seg_amp, found_inf set", 0, lambda: ops.adam_step_seg_amp(group.pflat, group.gflat, st[0], st[1], None, table, hp, one, one)))
        group.gflat.normal_(0.0, 0.02, generator=torch.Generator(device=dev).manual_seed(4))
        for label, nbytes, fn in calls:
            for _ in range(3):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            us = e0.elapsed_time(e1) / reps * 1e3
            print(f"KERNEL {int(amp)} {label}|{us:.1f}|{nbytes * group.total / us * 1e-3:.0f}", flush=True)


def gradscaler(n, steps, warmup, reps, emit):
    res, kern = {0: [], 1: []}, {}
    for _ in range(n):
        for amp in (0, 1):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--gradscaler-child", str(amp), "--steps", str(steps), "--warmup", str(warmup),
                                  "--reps", str(reps)], check=True, capture_output=True, text=True, timeout=300).stdout
            for ln in out.splitlines():
                if ln.startswith("GS "):
                    res[amp].append(ln.split()[2:])
                elif ln.startswith("KERNEL "):
                    label, us, gbs = ln[9:].split("|")
                    kern.setdefault(label, []).append((float(us), float(gbs)))
    emit(f"GradScaler loop, cfg2's two optimizers (SGD over the CNN-shaped layout, AdamW over bert-base), homed, gradients present, one shared scaler;")
    emit(f"per iteration scale -> step(sgd) -> step(adamw) -> update; median of {steps} iterations after {warmup}; {n} alternating processes per setting:")
    for amp, label in ((0, "fuse(opt)"), (1, "fuse(opt, amp_scaling=True)")):
        emit(f"  {label:<30} host us / iteration: " + "  ".join(f"{float(r[0]):8.1f}" for r in res[amp]) + "    device us / iteration: "
             + "  ".join(f"{float(r[1]):8.1f}" for r in res[amp]) + f"    fused launches / iteration {res[amp][0][2]}, fallbacks {res[amp][0][3]}, skipped {res[amp][0][4]}")
    emit(f"the step kernels alone (one group, {reps} back-to-back calls between two events; every process of both settings), us per call (GB/s):")
    for label, v in kern.items():
        emit(f"  {label:<40} " + "  ".join(f"{us:7.1f} ({gbs:5.0f})" if gbs else f"{us:7.1f}" for us, gbs in v))


CLIP_SETTINGS = (("flat_old", "FusedSGD / FusedAdamW, clip_grad_norm_"), ("flat_new", "FusedSGD / FusedAdamW, clip_in_step"),
                 ("stock_old", "fuse(opt), torch clip_grad_norm_"), ("stock_new", "fuse(opt), clip_in_step"),
                 ("gs_old", "GradScaler: unscale_, torch clip, step"), ("gs_new", "GradScaler: clip_in_step(scaler=), step"))


def clip_child(setting, steps, warmup):
    """one process of the clip mode; prints `CLIP <setting> <bite> host_us device_us device_ops` for the clip biting and not biting"""
    from vbg import optim as vo
    dev = torch.device("cuda")
    flat, gs = setting.startswith("flat"), setting.startswith("gs")
    new = setting.endswith("new")
    scale = 65536.0 if gs else 1.0
    sides = []
    for kind, meta in (("sgd", cnn_named()), ("adamw", bert_named())):
        nm = real(meta, dev, 1)
        cls, kw = (torch.optim.AdamW, ADAMW_KW) if kind == "adamw" else (torch.optim.SGD, SGD_KW)
        if flat:
            opt = (vo.FusedAdamW if kind == "adamw" else vo.FusedSGD)(nm, dev, **kw)
            group = opt.group
        else:
            group = vo.FlatGroup(nm, dev)
            opt = vo.fuse(cls([p for _, p in nm], **kw), amp_scaling=gs)
        saved = torch.zeros_like(group.gflat)          # gradients where parameters are, zeros in the padding (as backward leaves the buffer)
        for p, off in zip(group.params, group.offsets):
            saved[off:off + p.numel()].normal_(0.0, 0.02 * scale, generator=torch.Generator(device=dev).manual_seed(2 + off % 97))
        sides.append((group, opt, saved))
    opts = [opt for _, opt, _ in sides]
    params = [p for group, _, _ in sides for p in group.params]
    norm = float(torch.sqrt(sum((saved.double() ** 2).sum() for _, _, saved in sides))) / scale
    scaler = torch.amp.GradScaler("cuda", growth_interval=10 ** 9) if gs else None
    x = torch.zeros((), device=dev)

    def iteration(max_norm):
        if gs:
            scaler.scale(x)
            if new:
                vo.clip_in_step(opts, max_norm, scaler=scaler)
            else:
                for opt in opts:
                    scaler.unscale_(opt)
                torch.nn.utils.clip_grad_norm_(params, max_norm)
            for opt in opts:
                scaler.step(opt)
            scaler.update()
            return
        if new:
            vo.clip_in_step(opts, max_norm)
        elif flat:
            vo.clip_grad_norm_(opts, max_norm)
        else:
            torch.nn.utils.clip_grad_norm_(params, max_norm)
        for opt in opts:
            opt.step()

    def put_back():
        for group, _, saved in sides:
            group.gflat.copy_(saved)
            for p, gv in zip(group.params, group.gviews):
                if p.grad is not gv:
                    p.grad = gv

    for bite in (1, 0):
        max_norm = norm * (0.5 if bite else 2.0)
        host, devt = [], []
        for it in range(warmup + steps):
            put_back()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            t0 = time.perf_counter()
            iteration(max_norm)
            t1 = time.perf_counter()
            e1.record()
            e1.synchronize()
            if it >= warmup:
                host.append((t1 - t0) * 1e6)
                devt.append(e0.elapsed_time(e1) * 1e3)
        # the clip did what the setting says: .grad holds the unscaled gradient, times 1/2 where it bites
        got = float(torch.sqrt(sum((group.gflat.double() ** 2).sum() for group, _, _ in sides)))
        want = norm * (0.5 if bite else 1.0)
        assert abs(got - want) <= 1e-3 * want, (setting, bite, got, want)
        ops_n = -1
        try:
            from torch.profiler import ProfilerActivity, profile
            put_back()
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                iteration(max_norm)
                torch.cuda.synchronize()
            ops_n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
        except Exception as e:          # (the count is reported as not measured)
            print("profiler:", type(e).__name__, e, file=sys.stderr)
        print(f"CLIP {setting} {bite} {statistics.median(host):.1f} {statistics.median(devt):.1f} {ops_n}", flush=True)
    for opt in opts:
        fs = getattr(opt, "_vbg_fused", None)
        if fs is not None:
            fs.reconcile()
            assert fs.fallbacks == 0 and fs.skipped == 0, fs.last_fallback


def clip(n, steps, warmup, emit):
    res = {}
    for _ in range(n):
        for setting, _ in CLIP_SETTINGS:
            try:
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--clip-child", setting, "--steps", str(steps), "--warmup", str(warmup)],
                                     check=True, capture_output=True, text=True, timeout=300).stdout
            except subprocess.CalledProcessError as e:
                print(e.stderr[-4000:], file=sys.stderr, flush=True)
                raise
            print(f"  ({setting}: done)", file=sys.stderr, flush=True)
            for ln in out.splitlines():
                if ln.startswith("CLIP "):
                    _, s_, bite, host, devt, ops_n = ln.split()
                    res.setdefault((s_, int(bite)), []).append((float(host), float(devt), int(ops_n)))
    emit("gradient-norm clipping in front of the step, cfg2's two optimizers (SGD over the CNN-shaped layout, AdamW over bert-base), homed, gradients")
    emit(f"present; per iteration clip -> step(sgd) -> step(adamw) (GradScaler settings: scale -> [unscale_ x2] -> clip -> scaler.step x2 -> update);")
    emit(f"median of {steps} iterations after {warmup}; {n} alternating processes per setting; device ops: kernels + copies + memsets of one iteration (-1: not measured)")
    for bite in (1, 0):
        emit("clip biting (max_norm = norm / 2):" if bite else "clip not biting (max_norm = 2 x norm):")
        for setting, label in CLIP_SETTINGS:
            r = res[(setting, bite)]
            emit(f"  {label:<42} host us / iteration: " + "  ".join(f"{h:8.1f}" for h, _, _ in r) + "    device us / iteration: "
                 + "  ".join(f"{d:8.1f}" for _, d, _ in r) + f"    device ops / iteration {r[0][2]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--e2e", type=int, default=0, help="alternating processes per mode of the end-to-end stock loop (0: skip)")
    ap.add_argument("--e2e-child", default=None, choices=["fuse", "plain"])
    ap.add_argument("--gradscaler", type=int, default=0, help="alternating processes per setting of the GradScaler loop (runs only that)")
    ap.add_argument("--gradscaler-child", default=None, choices=["0", "1"])
    ap.add_argument("--clip", type=int, default=0, help="alternating processes per setting of the clipping loop (runs only that)")
    ap.add_argument("--clip-child", default=None, choices=[s_ for s_, _ in CLIP_SETTINGS])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stock_optim_bench: needs the GPU (no timing is taken without one)")
    if a.e2e_child:
        return e2e_child(a.e2e_child, a.steps, a.warmup)
    if a.gradscaler_child:
        return gradscaler_child(a.gradscaler_child == "1", a.steps, a.warmup, a.reps)
    if a.clip_child:
        return clip_child(a.clip_child, a.steps, a.warmup)
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    if a.gradscaler or a.clip:
        emit(f"{torch.cuda.get_device_name(0)}")
        if a.clip:
            clip(a.clip, a.steps, a.warmup, emit)
        else:
            gradscaler(a.gradscaler, a.steps, a.warmup, a.reps, emit)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    emit(f"{torch.cuda.get_device_name(0)}; {a.rounds} rounds x {a.reps} calls per variant, variants visited in turn; median (min, max) per call")
    emit("AdamW over the bert-base layout (pooler left out):")
    ok = measure("adamw", bert_named(), a.rounds, a.reps, emit)
    torch.cuda.empty_cache()
    emit("SGD with momentum over the CNN-shaped layout:")
    ok = measure("sgd", cnn_named(), a.rounds, a.reps, emit) and ok
    torch.cuda.empty_cache()
    if a.e2e:
        e2e(a.e2e, a.steps, a.warmup, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if not ok:
        raise SystemExit("the default case of a new entry is outside the 1.05x bound")


if __name__ == "__main__":
    main()
