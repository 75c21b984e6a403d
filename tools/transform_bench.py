"""The input transform (a1) in front of a batch-8 forward: the per-image route (a zero fill, one resize launch and one box launch per
image, pack_boxes) against vbg_transform_batch (one launch), for fp32 images and for the same pixels as bytes (uint8 CHW, and a decoded
HWC array seen through permute), plus what the byte formats change in front of the transform: the PackedBatch size and its H2D copy.

Two workloads, B = 8, 128 boxes per image:
  cfg2     3 x 512 x 512 images, min_size = max_size = 512: the identity path of bench.py's synthetic documents;
  receipts images of 8 different sizes between 700 x 330 and 1290 x 620, min_size 512 / max_size 512: every image is downscaled.
Per setting a fresh process (the settings alternating, `--procs` rounds), warmed up; per process the median of `--steps` calls of
  host    host clock around transform.forward_packed(images, coors): the time the call keeps the host (launches are asynchronous);
  synced  the same call followed by a device synchronize (the device had been idle: launch latency plus the kernels);
  h2d     PackedBatch.to(device) of the whole collated batch plus a synchronize (pinned, one copy), with the pack's bytes.
The tool also counts, in one untimed call, the library launches and the aten operations the call dispatches (torch's dispatcher sees
every kernel launch and copy torch makes).  The batched and per-image routes must give the same bits, and the byte formats the bits of
the fp32 route on their /255 floats, or the process fails.  Without a GPU nothing is measured and the tool says so.

    python tools/transform_bench.py [--out profiles/transform_batch.txt] [--procs 3] [--steps 30] [--warmup 5]"""
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

SETTINGS = ("per-image fp32", "batched fp32", "batched u8 chw", "batched u8 hwc")
WORKLOADS = ("cfg2", "receipts")
B, S = 8, 128
MEAN, STD = [0.9248, 0.9224, 0.9215], [0.1532, 0.1545, 0.1536]
VIEWS = ("aten.select.int", "aten.alias.default", "aten.view.default", "aten.detach.default", "aten.t.default", "aten.reshape.default",
         "aten._unsafe_view.default", "aten.as_strided.default", "aten.slice.Tensor", "aten.permute.default", "aten.view.dtype")
LIBCALLS = ("vbg_transform_batch", "vbg_normalize_resize", "vbg_rescale_boxes")


def make_bytes(workload):
    """-> (uint8 HWC images, int64 boxes) on the host"""
    g = torch.Generator().manual_seed(17)
    if workload == "cfg2":
        shapes = [(512, 512)] * B
    else:
        shapes = [(700 + 84 * b + b % 3, 330 + 41 * b + b % 2) for b in range(B)]
    imgs = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8) for h, w in shapes]
    coors = []
    for h, w in shapes:
        x1, y1 = torch.randint(0, w - 72, (S,), generator=g), torch.randint(0, h - 24, (S,), generator=g)
        coors.append(torch.stack([x1, y1, x1 + torch.randint(8, 73, (S,), generator=g), y1 + torch.randint(8, 25, (S,), generator=g)], 1).long())
    return imgs, coors


def as_setting(hwc, setting):
    if setting.endswith("hwc"):
        return [t.permute(2, 0, 1) for t in hwc]
    chw = [t.permute(2, 0, 1).contiguous() for t in hwc]
    return chw if setting.endswith("chw") else [t.float().div(255) for t in chw]


def collate(images, coors):
    z = [torch.zeros(512, dtype=torch.int32) for _ in images]
    cl = [torch.zeros(S, dtype=torch.int32) for _ in images]
    return tuple(images), tuple(z), tuple(cl), tuple(coors), torch.zeros((len(images), 512), dtype=torch.int64), torch.ones((len(images), 512), dtype=torch.int32)


def median_us(fn, steps, warmup, sync):
    us = []
    for it in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        t1 = time.perf_counter()
        if it >= warmup:
            us.append((t1 - t0) * 1e6)
    return statistics.median(us)


def child(setting, steps, warmup):
    """one process; per workload prints `TIME workload host synced h2d bytes` and `OPS workload name=count ...`"""
    from torch.utils._python_dispatch import TorchDispatchMode

    from pipeline.transform import GeneralizedViBERTgridTransform
    from vbg import ops
    from vbg.batch import PackedBatch
    dev = torch.device("cuda")
    tr = GeneralizedViBERTgridTransform(MEAN, STD, [512], 512, 512).eval()
    for workload in WORKLOADS:
        hwc, coors = make_bytes(workload)
        host_imgs = as_setting(hwc, setting)
        pb = PackedBatch.pack(*collate(host_imgs, coors))
        moved = pb.to(dev)
        imgs, dcoors = moved[0], moved[3]
        ops.set_transform_batch(not setting.startswith("per-image"))
        fn = lambda: tr.forward_packed(imgs, dcoors)                                 # noqa: E731
        # the same bits from every route: the fp32 per-image route on the /255 floats is the yardstick
        got = fn()
        ops.set_transform_batch(False)
        ref = tr.forward_packed(tuple(t.to(dev) for t in as_setting(hwc, "per-image fp32")), dcoors)
        ops.set_transform_batch(not setting.startswith("per-image"))
        same = torch.equal(got[0].view(torch.int32), ref[0].view(torch.int32)) and all(torch.equal(a, b) for a, b in zip(got[3], ref[3]))
        assert same, f"{setting} / {workload}: the routes disagree"
        host = median_us(fn, steps, warmup, False)
        synced = median_us(fn, steps, warmup, True)
        h2d = median_us(lambda: pb.to(dev), steps, warmup, True)
        print(f"TIME {workload} {host:.1f} {synced:.1f} {h2d:.1f} {pb.nbytes()}", flush=True)

        counts = collections.Counter()

        class Count(TorchDispatchMode):
            def __torch_dispatch__(self, func, types, args=(), kwargs=None):
                counts[str(func)] += 1
                return func(*args, **(kwargs or {}))

        real = {n: getattr(ops.lib, n) for n in LIBCALLS}

        def counted(name):
            def f(*a):
                counts[name] += 1
                if name == "vbg_transform_batch":           # (one launch per TRANSFORM_MAX_IMAGES descriptors)
                    counts["launches"] += -(-a[1] // ops.TRANSFORM_MAX_IMAGES)
                else:
                    counts["launches"] += 1
                return real[name](*a)
            return f

        for n in LIBCALLS:
            setattr(ops.lib, n, counted(n))
        with Count():
            fn()
        for n in LIBCALLS:
            setattr(ops.lib, n, real[n])
        print(f"OPS {workload} " + " ".join(f"{k}={v}" for k, v in sorted(counts.items())), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--procs", type=int, default=3, help="alternating processes per setting")
    ap.add_argument("--steps", type=int, default=30)
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
        emit("input transform: no GPU in this run -- NOT MEASURED (python tools/transform_bench.py --out profiles/transform_batch.txt on an MI355X)")
        return finish(1)
    times = {(s, w): [] for s in SETTINGS for w in WORKLOADS}
    opsof = {}
    for _ in range(a.procs):
        for s in SETTINGS:
            run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", s, "--steps", str(a.steps), "--warmup", str(a.warmup)],
                                 capture_output=True, text=True, timeout=300)
            if run.returncode != 0:          # (nothing more is started behind a process that failed)
                print(run.stderr[-4000:], file=sys.stderr, flush=True)
                return run.returncode
            for ln in run.stdout.splitlines():
                f = ln.split()
                if ln.startswith("TIME "):
                    times[(s, f[1])].append([float(v) for v in f[2:]])
                elif ln.startswith("OPS "):
                    opsof[(s, f[1])] = dict((kv.rsplit("=", 1)[0], int(kv.rsplit("=", 1)[1])) for kv in f[2:])
    emit(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    emit(f"input transform of a batch of {B} images with {S} boxes each: transform.forward_packed -> padded NHWC batch, boxes, box_off, box_doc")
    emit("  cfg2    : 3 x 512 x 512 images to 512 (identity path);  receipts: 8 sizes from 700 x 330 to 1290 x 620, downscaled to max 512")
    emit("  per-image fp32: zero fill + vbg_normalize_resize + vbg_rescale_boxes per image + pack_boxes;  batched: vbg_transform_batch")
    emit(f"host clock; median of {a.steps} calls after {a.warmup}; {a.procs} alternating fresh processes per setting; one value per process")
    for w in WORKLOADS:
        for col, name in ((0, "host us  "), (1, "synced us")):
            for s in SETTINGS:
                r = times[(s, w)]
                emit(f"  {w:<8} {name}  {s:<15} " + "  ".join(f"{v[col]:9.1f}" for v in r))
            base = statistics.median(v[col] for v in times[(SETTINGS[0], w)])
            spread = max(v[col] for v in times[(SETTINGS[0], w)]) / min(v[col] for v in times[(SETTINGS[0], w)])
            emit(f"  {w:<8} {name}  per-image / batched (medians over the processes): " +
                 ", ".join(f"{s.split(' ', 1)[1]} {base / statistics.median(v[col] for v in times[(s, w)]):.2f}x" for s in SETTINGS[1:]) +
                 f"; max / min of the per-image processes: {spread:.3f}")
    emit("PackedBatch of the collated batch (images, boxes, 512 token ids and mask per document), pinned, one H2D copy + synchronize:")
    for w in WORKLOADS:
        for s in (SETTINGS[0], SETTINGS[2], SETTINGS[3]):
            r = times[(s, w)]
            emit(f"  {w:<8} {s.split(' ', 1)[1]:<7} bytes {int(r[0][3]):10d}   h2d us " + "  ".join(f"{v[2]:9.1f}" for v in r))
        fb, ub = times[(SETTINGS[0], w)][0][3], times[(SETTINGS[3], w)][0][3]
        ft, ut = (statistics.median(v[2] for v in times[(s, w)]) for s in (SETTINGS[0], SETTINGS[3]))
        emit(f"  {w:<8} fp32 / u8 hwc: bytes {fb / ub:.2f}x, h2d time {ft / ut:.2f}x")
    emit("operations per call (library launches; torch dispatcher counts of one untimed call, views left out):")
    for w in WORKLOADS:
        for s in SETTINGS:
            d = {k: v for k, v in opsof[(s, w)].items() if k not in VIEWS}
            emit(f"  {w:<8} {s:<15} " + ", ".join(f"{k} x {v}" for k, v in sorted(d.items())))
    return finish(0)


if __name__ == "__main__":
    sys.exit(main())
