#!/usr/bin/env python3
"""Host cost of ONE encoder layer backward (BertLayerFn.backward) in training at cfg2, batch 8: wall time per call, and -- where the tree
has the one-call entry -- of its wrapper (ops.bert_layer_bwd: descriptor + C call) and of the C call alone, plus the library calls one
layer's backward makes.  The switch is read from the environment (VBG_LAYER_BWD_ENTRY), one fresh process per setting; the same file runs
on a checkout without the entry (the yardstick): it then reports the per-call time alone.  `--amp`: inside an autocast region."""
import contextlib, os, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.environ.get("VBG_TREE"):            # measure another checkout (the parent commit's) with this file
    ROOT = os.path.abspath(os.environ["VBG_TREE"])
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "vibertgrid-pytorch_amd"))
import torch
import bench
from vbg import ops, functions as Fn
from vbg.batch import PackedBatch
from vbg.lib import lib, SIGNATURES
from vbg.optim import FusedAdamW, FusedSGD, split_parameters

AMP = "--amp" in sys.argv
STEPS, WARM = 12, 4
dev = torch.device("cuda")
with contextlib.redirect_stdout(sys.stderr):
    torch.manual_seed(42)
    net = bench.build_model(tempfile.mkdtemp(prefix="vbg_lbe_")).to(dev).train()
cnn, bert = split_parameters(net)
opts = [FusedSGD(cnn, dev, lr=0.005, momentum=0.9, weight_decay=0.005), FusedAdamW(bert, dev, lr=5e-5, weight_decay=0.01)]
dbatch = PackedBatch.pack(*bench.synthetic_batch(8, 512, 512, 512, 128, bench.NCLS, bench.VOCAB, 1234)).to(dev)


def step():
    with torch.autocast("cuda", dtype=torch.float16, enabled=AMP):
        loss = net(*dbatch)
    for o in opts:
        o.zero_grad()
    loss.backward()
    for o in opts:
        o.step()


acc = {}


def timed(obj, name, key):
    f = getattr(obj, name)

    def w(*a, **k):
        t = time.perf_counter()
        r = f(*a, **k)
        acc.setdefault(key, []).append(time.perf_counter() - t)
        return r
    setattr(obj, name, w)
    return f


has_entry = hasattr(ops, "bert_layer_bwd")
state = f"VBG_LAYER_BWD_ENTRY={int(ops._LAYER_BWD_ENTRY[0])}" if has_entry else "no backward entry in this tree"
for _ in range(WARM):
    step()
torch.cuda.synchronize()

# pass 1: the layer backward alone (one timer around BertLayerFn.backward: 12 calls per step)
f0 = Fn.BertLayerFn.backward
def bwd(*a, **k):
    t = time.perf_counter(); r = f0(*a, **k); acc.setdefault("BertLayerFn.backward", []).append(time.perf_counter() - t); return r
Fn.BertLayerFn.backward = staticmethod(bwd)
for _ in range(STEPS):
    step()
torch.cuda.synchronize()
per_call = acc.pop("BertLayerFn.backward")
layers = len(per_call) // STEPS

# pass 2: inside it (more timers, so pass 1 is the figure to compare between trees)
inner = []
if has_entry:
    inner.append((ops, "bert_layer_bwd", timed(ops, "bert_layer_bwd", "ops.bert_layer_bwd (wrapper + C call)")))
    inner.append((ops, "bert_layer_bwd_launches", timed(ops, "bert_layer_bwd_launches", "ops.bert_layer_bwd_launches (per-launch sequence)")))
    inner.append((lib, "vbg_bert_layer_bwd", timed(lib, "vbg_bert_layer_bwd", "lib.vbg_bert_layer_bwd (C call alone)")))
for _ in range(STEPS):
    step()
torch.cuda.synchronize()
for obj, name, f in inner:
    setattr(obj, name, f)
acc.pop("BertLayerFn.backward", None)
inside = {k: v for k, v in acc.items()}
acc.clear()

# pass 3: library calls made from inside one layer's backward (counted, not timed)
calls, live = {}, [False]
saved = {}
for name in SIGNATURES:
    f = getattr(lib, name)
    saved[name] = f
    def cw(*a, _f=f, _n=name):
        if live[0]:
            calls[_n] = calls.get(_n, 0) + 1
        return _f(*a)
    setattr(lib, name, cw)
def bwd_count(*a, **k):
    live[0] = True
    try:
        return f0(*a, **k)
    finally:
        live[0] = False
Fn.BertLayerFn.backward = staticmethod(bwd_count)
step()
torch.cuda.synchronize()
Fn.BertLayerFn.backward = staticmethod(f0)
for name, f in saved.items():
    setattr(lib, name, f)

us = [1e6 * t for t in per_call]
per_step = [1e3 * sum(per_call[i * layers:(i + 1) * layers]) for i in range(STEPS)]
print(f"[{state}; {'amp' if AMP else 'fp32-grade'}; cfg2 batch 8, {layers} layers, {STEPS} steps]")
print(f"  BertLayerFn.backward host time: median {statistics.median(us):7.1f} us per layer (mean {statistics.fmean(us):7.1f}, min {min(us):7.1f}); "
      f"{statistics.median(per_step):6.3f} ms per step over {layers} layers")
for k, v in sorted(inside.items()):
    print(f"    {k:52s} {len(v) / STEPS:5.1f} calls per step, median {1e6 * statistics.median(v):7.1f} us each")
launching = {k: v for k, v in calls.items() if not k.endswith(("_ws_rows", "_ws_elems", "_thr16"))}
print(f"  library calls per layer backward: {sum(launching.values()) / layers:.1f}  " +
      ", ".join(f"{k} x{v / layers:g}" for k, v in sorted(launching.items())))
