#!/usr/bin/env python3
"""Deployment-style latency of ViBERTgridNet.inference (reference deployment/inference_SROIE.py:143-151 prints the same
quantity): one document at a time, 512x512, T = 512 tokens, S = 128 segments, resnet_34_fpn_pretrained + bert-base (12 layers).

python tools/infer_latency.py            one process, the switches as the environment has them
python tools/infer_latency.py --ab [N]   frozen-BatchNorm epilogue off / on (VBG_BN_EPILOGUE=0 / 1) in N (default 3) ALTERNATING fresh
                                         processes per setting, one at a time; prints every run and the medians per batch size"""
import contextlib, os, re, statistics, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if len(sys.argv) > 1 and sys.argv[1] == "--ab":
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    runs = {"0": {}, "1": {}}
    for i in range(n):
        for setting in ("0", "1"):
            env = dict(os.environ, VBG_BN_EPILOGUE=setting)
            out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, check=True, capture_output=True, text=True).stdout
            for ln in out.splitlines():
                print(f"[run {i} epilogue {'on ' if setting == '1' else 'off'}] {ln}", flush=True)
                m = re.match(r"inference batch (\d+): ([0-9.]+) ms", ln)
                if m:
                    runs[setting].setdefault(int(m.group(1)), []).append(float(m.group(2)))
    for B in sorted(runs["0"]):
        off, on = statistics.median(runs["0"][B]), statistics.median(runs["1"][B])
        print(f"median of {n} processes, batch {B}: epilogue off {off:.3f} ms   on {on:.3f} ms   ({(on - off) * 1e3:+.0f} us, {(on / off - 1) * 100:+.2f} %)")
    sys.exit(0)

sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "vibertgrid-pytorch_amd"))
import torch
import bench
from vbg import ops

dev = torch.device("cuda")
with contextlib.redirect_stdout(sys.stderr):
    net = bench.build_model(tempfile.mkdtemp()).to(dev).eval()
print(f"frozen-BatchNorm epilogue: {'on' if ops.bn_epilogue_enabled() else 'off'}")
for B in [int(b) for b in os.environ.get("VBG_INFER_BATCHES", "1,8").split(",")]:
    batch = bench.synthetic_batch(B, 512, 512, 512, 128, 5, 30522, 7)
    mv = lambda ts: tuple(t.to(dev) for t in ts)
    args = (mv(batch[0]), mv(batch[1]), mv(batch[3]), batch[4].to(dev), batch[5].to(dev))
    with torch.no_grad():
        for _ in range(5):
            net.inference(*args)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 30
        for _ in range(n):
            p = net.inference(*args)
            p.cpu()                      # the caller reads the probabilities
        dt = (time.perf_counter() - t0) / n
        print(f"inference batch {B}: {dt * 1e3:.2f} ms per call, {B / dt:.1f} docs/s")
        # both routes once in this process: launches per call that the switch moves, and whether the probabilities differ bitwise
        was, res = ops.bn_epilogue_enabled(), {}
        for on in (False, True):
            ops.set_bn_epilogue(on)
            log = ops.dispatch_log(True)
            res[on] = (net.inference(*args), dict(log))
            ops.dispatch_log(False)
        ops.set_bn_epilogue(was)
        (p0, l0), (p1, l1) = res[False], res[True]
        print(f"  batch {B}: off = {l0.get('bn:apply', 0)} bn_apply launches; on = {l1.get('bn:epilogue', 0)} epilogues "
              f"({l1.get('bn:epilogue_conv3', 0)} conv3 + {l1.get('bn:epilogue_gemm', 0)} gemm), {l1.get('bn:apply', 0)} bn_apply: "
              f"{l0.get('bn:apply', 0) - l1.get('bn:apply', 0)} launches fewer per call; probabilities bitwise equal: {torch.equal(p0, p1)}, "
              f"max |on - off| = {float((p0 - p1).abs().max()):.3e}")
