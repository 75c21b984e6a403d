"""Segmented optimizer launches (vbg_adamw_step_seg / vbg_sgd_step_seg) against the whole-range launches they stand beside, at the
sizes the product steps: the bert-base AdamW buffer (layout from the parameter names on the meta device, no weights) and a
41.8 M-element SGD buffer cut into slots of a ResNet-34 trunk and 3x3 head convolutions.

One process, every variant warmed up, then ROUNDS rounds that visit the variants in turn (so drift of the machine hits all of them
alike); per variant the median over the rounds of the mean of REPS back-to-back launches between two device events.  Reported:
microseconds per launch, effective TB/s (28 B per element for AdamW, 20 B for SGD, over the elements the launch covers), and the
ratio to the whole-range launch of the same round set.  Needs the GPU; `--layout-only` prints the tables' sizes without one.

    python tools/optim_groups_bench.py [--out FILE] [--chunks 1024,4096,16384] [--rounds 9] [--reps 10]"""
import argparse
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vibertgrid-pytorch_amd"))

NO_DECAY = ("bias", "LayerNorm.weight", "bn")


def flat_layout(named):
    """what vbg.optim.FlatGroup does with a (name, parameter) list, without touching the parameters: fusion order, slots padded to 8
    elements, total rounded up to 32"""
    from vbg.optim import _fusion_order
    named = _fusion_order(named)
    offsets, o = [], 0
    for _, p in named:
        offsets.append(o)
        o += (p.numel() + 7) // 8 * 8
    return types.SimpleNamespace(names=[n for n, _ in named], params=[p for _, p in named], offsets=offsets, end=o, total=(o + 31) // 32 * 32)


def bert_named():
    from transformers import BertConfig, BertModel
    with torch.device("meta"):
        m = BertModel(BertConfig())
    return [(n, p) for n, p in m.named_parameters() if "pooler." not in n]


def cnn_named(total=41_800_000):
    """slot sizes of a ResNet-34 trunk -- every convolution followed by its BatchNorm weight / bias pair -- then 3x3 convolutions of
    256 channels with a bias (FPN / head shaped) until the buffer holds `total` elements; registration order"""
    out, cin = [], 3
    def conv(name, co, ci, k, bn=True):
        out.append((f"{name}.weight", torch.empty((co, ci, k, k), device="meta")))
        if bn:
            out.append((f"{name}.bn.weight", torch.empty((co,), device="meta")))
            out.append((f"{name}.bn.bias", torch.empty((co,), device="meta")))
        else:
            out.append((f"{name}.bias", torch.empty((co,), device="meta")))
    conv("stage0.conv1", 64, 3, 7)
    cin = 64
    for s, (blocks, c) in enumerate(((3, 64), (4, 128), (6, 256), (3, 512)), start=1):
        for b in range(blocks):
            conv(f"stage{s}.{b}.conv1", c, cin, 3)
            conv(f"stage{s}.{b}.conv2", c, c, 3)
            if b == 0 and cin != c:
                conv(f"stage{s}.{b}.downsample", c, cin, 1)
            cin = c
    k = 0
    while sum(p.numel() for _, p in out) + 256 * 256 * 9 + 256 <= total:
        conv(f"stage5.head{k}", 256, 256, 3, bn=False)
        k += 1
    co = (total - sum(p.numel() for _, p in out)) // (256 * 9 + 1)
    if co > 0:
        conv(f"stage5.head{k}", co, 256, 3, bn=False)
    return out


def depth(name):
    """embeddings 0, encoder layer N -> N + 1; CNN: the stage number"""
    if "layer." in name:
        return int(name.split("layer.")[1].split(".")[0]) + 1
    if name.startswith("stage"):
        return int(name[5])
    return 0


GROUPINGS = {
    "one group": lambda n: 0,
    "decay split": lambda n: int(any(k in n for k in NO_DECAY)),
    "layer-wise x decay": lambda n: 2 * depth(n) + int(any(k in n for k in NO_DECAY)),
}


def tables(layout, chunk):
    """{grouping: (ngroups, runs, chunk rows)}"""
    from vbg.optim import chunk_rows, run_table
    out = {}
    for label, key in GROUPINGS.items():
        ids = sorted({key(n) for n in layout.names})
        group_of = {id(p): ids.index(key(n)) for n, p in zip(layout.names, layout.params)}
        runs = run_table(layout, group_of)
        out[label] = (len(ids), runs, chunk_rows(runs, chunk))
    return out


def describe(title, layout, chunk, bpe, emit):
    sizes = [p.numel() for p in layout.params]
    emit(f"{title}: {len(sizes)} parameters, {sum(sizes) / 1e6:.1f} M elements ({layout.total} in the buffer), slots {min(sizes)} .. {max(sizes)}")
    for label, (ng, runs, rows) in tables(layout, chunk).items():
        emit(f"  {label:<20} {ng:>2} groups {len(runs):>3} runs {len(rows):>6} chunk rows of <= {chunk} ({16 * len(rows) / 1e3:.0f} KB table, "
             f"{100 * 16 * len(rows) / (bpe * layout.end):.3f} % of the step's traffic)")


def measure(kind, layout, chunks, rounds, reps, emit):
    from vbg import ops
    dev = torch.device("cuda")
    n, bpe = layout.total, (28.0 if kind == "adamw" else 20.0)
    g = torch.Generator(device=dev).manual_seed(1)
    bufs = [torch.randn(n, device=dev, generator=g) * 0.02 for _ in range(4 if kind == "adamw" else 3)]
    bufs[-1].abs_()
    hp = (5e-5, 0.9, 0.999, 1e-8, 0.01) if kind == "adamw" else (0.005, 0.9, 0.005)

    def whole():
        if kind == "adamw":
            ops.adamw_step(*bufs, *hp, 3, 1.0)
        else:
            ops.sgd_step(*bufs, *hp, False, 1.0)

    def seg(table, ng):
        def run():
            if kind == "adamw":
                ops.adamw_step_seg(*bufs, table, [hp] * ng, 3, 1.0)
            else:
                ops.sgd_step_seg(*bufs, table, [hp] * ng, False, 1.0)
        return run

    name = "vbg_adamw_step" if kind == "adamw" else "vbg_sgd_step"
    variants = [(f"{name} (whole range)", whole, n)]
    for chunk in chunks:
        for label, (ng, runs, rows) in tables(layout, chunk).items():
            table = ops.chunk_table(rows, ng, n, dev)
            variants.append((f"{name}_seg, {label}: {ng} groups {len(runs)} runs, chunk {chunk}", seg(table, ng), int(rows[:, 1].sum())))
    # the same bits at the size that is timed: one step of the widest grouping (identical hyper-parameters) against the whole range
    keep = [b.clone() for b in bufs]
    variants[len(GROUPINGS)][1]()
    segd = [b.clone() for b in bufs]
    for b, k in zip(bufs, keep):
        b.copy_(k)
    whole()
    same = all(torch.equal(a[:layout.end], b[:layout.end]) for a, b in zip(segd, bufs))
    emit(f"  one step, {variants[len(GROUPINGS)][0]} == whole range, bit for bit over the slots: {same}")
    del keep, segd
    for _, fn, _ in variants:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in variants]
    for _ in range(rounds):
        for i, (_, fn, _) in enumerate(variants):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            times[i].append(e0.elapsed_time(e1) / reps * 1e3)
    base = statistics.median(times[0])
    for (label, _, covered), t in zip(variants, times):
        us = statistics.median(t)
        emit(f"  {label:<78} {us:8.1f} us  (min {min(t):8.1f}, max {max(t):8.1f})  {bpe * covered / us / 1e6:5.2f} TB/s  x{us / base:.3f}")
    return same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--chunks", default=None, help="chunk lengths to time, comma separated (default: vbg.optim.SEG_CHUNK)")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--layout-only", action="store_true")
    a = ap.parse_args()
    from vbg.optim import SEG_CHUNK
    chunks = [int(c) for c in a.chunks.split(",")] if a.chunks else [SEG_CHUNK]
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    bert, cnn = flat_layout(bert_named()), flat_layout(cnn_named())
    describe("bert-base (pooler left out), AdamW", bert, chunks[0], 28.0, emit)
    describe("CNN-shaped buffer, SGD", cnn, chunks[0], 20.0, emit)
    ok = True
    if not a.layout_only:
        if not torch.cuda.is_available():
            raise SystemExit("optim_groups_bench: needs the GPU (no timing is taken without one)")
        emit(f"{torch.cuda.get_device_name(0)}; {a.rounds} rounds x {a.reps} launches per variant, variants visited in turn; median (min, max) per launch")
        emit("AdamW, 28 B per element:")
        ok = measure("adamw", bert, chunks, a.rounds, a.reps, emit) and ok
        emit("SGD with momentum, 20 B per element:")
        ok = measure("sgd", cnn, chunks, a.rounds, a.reps, emit) and ok
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if not ok:
        raise SystemExit("segmented and whole-range results differ")


if __name__ == "__main__":
    main()
