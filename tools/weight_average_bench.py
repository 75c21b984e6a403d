"""Weight averaging (vbg_lerp / vbg_swap, vbg.optim.WeightAverage) at the sizes the product trains: the two cfg2 flat buffers,
108 891 648 elements (bert-base, pooler left out) and 41 799 200 elements (CNN and heads).

Part 1, the kernels: vbg_lerp (12 B per element) and vbg_swap (16 B per element) on both sizes, with vbg_sgd_step (20 B per element)
on the 41.8 M buffer as the yardstick of what a stream of this shape reaches here.  One process, every variant warmed up, then ROUNDS
rounds that visit the variants in turn; per variant the median (min, max) over the rounds of the mean of REPS back-to-back launches
between two device events; microseconds per launch and effective TB/s.

Part 2, the class: a stand-in model with the parameters of both buffers (shapes from the bert-base names on the meta device and from
the ResNet-34-shaped list of tools/optim_groups_bench.py), homed in two FlatGroups.  `avg.update()` and `applied()` entry + exit:
host time per call (perf_counter around the call, nothing waited for) and device time (events around REPS calls); next to them
torch's route on the same parameter list: `AveragedModel(twin).update_parameters(twin)` on a plain twin (the deep copy it needs is
reported in MB) and `torch._foreach_lerp_` over the per-parameter views of the flat buffers.  Needs the GPU.

    python tools/weight_average_bench.py [--out FILE] [--rounds 9] [--reps 10]"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vibertgrid-pytorch_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

N_BERT, N_CNN = 108_891_648, 41_799_200


def timed(variants, rounds, reps):
    """[(label, fn, ...)] -> per variant the list over the rounds of microseconds per call, device time between two events"""
    for _, fn, *_ in variants:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in variants]
    for _ in range(rounds):
        for i, (_, fn, *_) in enumerate(variants):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            times[i].append(e0.elapsed_time(e1) / reps * 1e3)
    return times


def host_timed(fn, rounds, reps):
    """microseconds of host time per call: perf_counter around `reps` calls that wait for nothing; the device drains between rounds"""
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


def kernels(rounds, reps, emit):
    from vbg import ops
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(1)
    big = [torch.randn(N_BERT, device=dev, generator=g) * 0.02 for _ in range(2)]
    small = [torch.randn(N_CNN, device=dev, generator=g) * 0.02 for _ in range(3)]
    variants = [
        ("vbg_sgd_step  41.8 M (yardstick, 20 B/el)", lambda: ops.sgd_step(small[0], small[1], small[2], 0.005, 0.9, 0.005, False, 1.0), 20.0 * N_CNN),
        ("vbg_lerp      41.8 M (12 B/el), w = 1e-3", lambda: ops.lerp_(small[1], small[0], 1e-3), 12.0 * N_CNN),
        ("vbg_lerp      41.8 M (12 B/el), w = 0.5", lambda: ops.lerp_(small[1], small[0], 0.5), 12.0 * N_CNN),
        ("vbg_swap      41.8 M (16 B/el)", lambda: ops.swap_(small[0], small[1]), 16.0 * N_CNN),
        ("vbg_lerp     108.9 M (12 B/el), w = 1e-3", lambda: ops.lerp_(big[1], big[0], 1e-3), 12.0 * N_BERT),
        ("vbg_swap     108.9 M (16 B/el)", lambda: ops.swap_(big[0], big[1]), 16.0 * N_BERT),
    ]
    times = timed(variants, rounds, reps)
    yard = 20.0 * N_CNN / statistics.median(times[0]) / 1e6
    for (label, _, nbytes), t in zip(variants, times):
        tbs = nbytes / statistics.median(t) / 1e6
        emit(f"  {label:<44} {fmt(t)}  {tbs:5.2f} TB/s  x{tbs / yard:.2f} of the yardstick's rate")


class Bag(torch.nn.Module):
    """parameters only, under the names given (dots replaced), in the order given"""

    def __init__(self, named, device):
        super().__init__()
        g = torch.Generator(device=device).manual_seed(2)
        for n, p in named:
            self.register_parameter(n.replace(".", "_"), torch.nn.Parameter(torch.randn(tuple(p.shape), device=device, generator=g) * 0.02))


def the_class(rounds, reps, emit):
    from optim_groups_bench import bert_named, cnn_named
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    from vbg.optim import FlatGroup, WeightAverage
    dev = torch.device("cuda")
    nb, nc = [("bert_model." + n, p) for n, p in bert_named()], cnn_named()
    model, twin = Bag(nb + nc, dev), Bag(nb + nc, dev)
    named = list(model.named_parameters())
    groups = [FlatGroup(named[len(nb):], dev), FlatGroup(named[:len(nb)], dev)]
    emit(f"  stand-in model: {len(named)} parameters in two flat groups of {groups[1].total} and {groups[0].total} elements")
    avg = WeightAverage(model, kind="ema", decay=0.999)
    avg.update()
    ref = AveragedModel(twin, multi_avg_fn=get_ema_multi_avg_fn(0.999))
    ref.update_parameters(twin)
    copy_mb = sum(p.numel() for p in ref.module.parameters()) * 4 / 1e6
    shadow_views = [g.view(s, i) for g, s in zip(avg.groups, avg.shadows) for i in range(len(g.params))]
    live_views = [p.data for g in avg.groups for p in g.params]

    def cycle():
        with avg.applied():
            pass

    variants = [
        ("WeightAverage.update(): 2 x vbg_lerp", avg.update),
        (f"AveragedModel.update_parameters, {len(named)} tensors", lambda: ref.update_parameters(twin)),
        (f"torch._foreach_lerp_ over {len(shadow_views)} views of the flat buffers", lambda: torch._foreach_lerp_(shadow_views, live_views, 1e-3)),
        ("applied() entry + exit: 4 x vbg_swap", cycle),
    ]
    dev_t = timed(variants, rounds, reps)
    for (label, fn), t in zip(variants, dev_t):
        emit(f"  {label:<62} device {fmt(t)}   host {fmt(host_timed(fn, rounds, reps))}")
    emit(f"  memory: WeightAverage {sum(s.numel() for s in avg.shadows) * 4 / 1e6:.0f} MB (one buffer per group); AveragedModel {copy_mb:.0f} MB "
         "of parameters in a second module (on the product: plus that module's plane / filter images once it runs a forward)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("weight_average_bench: needs the GPU (no timing is taken without one)")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"{torch.cuda.get_device_name(0)}; {a.rounds} rounds x {a.reps} calls per variant, variants visited in turn; median (min, max) per call")
    emit("1. kernels (device time):")
    kernels(a.rounds, a.reps, emit)
    torch.cuda.empty_cache()
    emit("2. vbg.optim.WeightAverage against torch's route (device time between events; host time of the call, nothing waited for):")
    the_class(a.rounds, a.reps, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
