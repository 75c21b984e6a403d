"""What a rectangular RoIAlign output costs: RoIAlign forward, default backward and deterministic backward on cfg2-like boxes
(8 documents of 512 x 512 -> a 128 x 128 x 256 P_fuse map, 128 boxes each), and one cfg2 training step (forward + backward, batch 8),
for roi_shape 7 against (3, 21).  Prints one table; profiles/roi_shapes.txt holds one such measurement.

    python tools/roi_shapes_bench.py [--iters 50] [--steps 5]
"""
import argparse
import functools
import os
import random
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vibertgrid-pytorch_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import roi_align_restate as R  # noqa: E402
from vbg import ops  # noqa: E402

DEV = torch.device("cuda")
SHAPES = (7, (3, 21))


def _time(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters            # us


def kernels(iters):
    rng = np.random.default_rng(0)
    B, H, W, C = 8, 128, 128, 256
    boxes, doc = R.cfg2_like_boxes(rng, B, 121, H, W)        # 121 text boxes + 7 special ones per document
    feat = torch.randn((B, H, W, C), device=DEV)
    bx, bd = torch.from_numpy(boxes).to(DEV), torch.from_numpy(doc).to(DEV)
    rows = []
    for s in SHAPES:
        oh, ow = ops.roi_out_hw(s)
        dy = torch.randn((len(boxes), oh, ow, C), device=DEV)
        df = torch.zeros((B, H, W, C), device=DEV)
        fwd = _time(lambda: ops.roi_align_fwd(feat, bx, bd, s, 0.25), iters)
        bwd = _time(lambda: ops.roi_align_bwd(dy, (B, H, W, C), bx, bd, s, 0.25, df), iters)
        with ops.deterministic_scope(True):
            det = _time(lambda: ops.roi_align_bwd(dy, (B, H, W, C), bx, bd, s, 0.25, df), max(1, iters // 5))
        rows.append((s, len(boxes), fwd, bwd, ops.roi_bwd_form(H, W, oh, ow), det))
    return rows


def step(shape, steps):
    import bench
    import model.ViBERTgrid_net as M
    orig = M.ViBERTgridNet
    M.ViBERTgridNet = functools.partial(orig, roi_shape=shape)
    try:
        net = bench.build_model(tempfile.mkdtemp(prefix="vbg_roi_bench_"))
    finally:
        M.ViBERTgridNet = orig
    net = net.to(DEV).train()
    batch = bench.synthetic_batch(8, 512, 512, 512, 128, bench.NCLS, bench.VOCAB, 1234)
    imgs, segs, classes, coors, corpus, mask = batch
    mv = lambda ts: tuple(t.to(DEV) for t in ts)
    dbatch = (mv(imgs), mv(segs), mv(classes), mv(coors), corpus.to(DEV), mask.to(DEV))
    times = []
    for it in range(steps + 2):
        net.zero_grad(set_to_none=True)
        random.seed(it)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss = net(*dbatch)
        loss.backward()
        torch.cuda.synchronize()
        if it >= 2:
            times.append((time.perf_counter() - t0) * 1000.0)
    del net
    torch.cuda.empty_cache()
    return float(np.median(times)), float(loss)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=5)
    a = ap.parse_args()
    print(f"# {torch.cuda.get_device_name(0)}; RoIAlign on a [8, 128, 128, 256] P_fuse map, cfg2-like boxes; mean of {a.iters} launches")
    print(f"{'roi_shape':>10} {'rois':>6} {'fwd us':>9} {'bwd us':>9} {'bwd form':>9} {'det bwd us':>11}")
    for s, n, fwd, bwd, form, det in kernels(a.iters):
        print(f"{str(s):>10} {n:>6} {fwd:>9.1f} {bwd:>9.1f} {form:>9} {det:>11.1f}")
    print(f"# cfg2 training step (forward + backward, 8 documents, resnet_34_fpn + 12-layer BERT), median of {a.steps} after 2 warm-up")
    for s in SHAPES:
        ms, loss = step(s, a.steps)
        print(f"{str(s):>10}  step {ms:8.2f} ms   loss {loss:.5f}")


if __name__ == "__main__":
    main()
