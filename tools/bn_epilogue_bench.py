#!/usr/bin/env python3
"""What the frozen-BatchNorm epilogue costs and saves per convolution of the cfg2 trunk (eval mode): the convolution with a plain store,
the same launch with the epilogue (BatchNorm + residual + ReLU + amax word), and the two launches it replaces (convolution + bn_apply).
python tools/bn_epilogue_bench.py [reps]   batch 8 and batch 1 (single-document inference) rows"""
import os, sys, math
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vibertgrid-pytorch_amd"))
import torch
from vbg import ops
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
dev = torch.device("cuda")
torch.manual_seed(0)
def t(fn):
    for _ in range(3): fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3
# (B, H, W, Cin, Cout, k, stride, pad): the trunk's 3x3 / s1 stages (row-reuse kernels), its strided 3x3 and 1x1 shortcut convolutions
# (generic kernel), at batch 8 and for one document
SHAPES = [(B, *s) for B in (8, 1) for s in ((128, 128, 64, 64, 3, 1, 1), (64, 64, 128, 128, 3, 1, 1), (32, 32, 256, 256, 3, 1, 1), (16, 16, 512, 512, 3, 1, 1),
                                            (128, 128, 64, 128, 3, 2, 1), (128, 128, 64, 128, 1, 2, 0), (32, 32, 256, 512, 3, 2, 1), (32, 32, 256, 512, 1, 2, 0))]
with torch.no_grad():
    for (B, H, W, C, N, k, stride, pad) in SHAPES:
        x = torch.randn(B, H, W, C, device=dev)
        wd = (torch.randn(N, C, k, k, device=dev) / math.sqrt(k * k * C)).contiguous(memory_format=torch.channels_last)
        w4 = wd.permute(0, 2, 3, 1)
        Ho, Wo = ops.conv_out_hw(H, W, k, stride, pad)
        mean, var = 0.1 * torch.randn(N, device=dev), 0.5 + torch.rand(N, device=dev)
        gamma, beta, invstd = 0.5 + torch.rand(N, device=dev), torch.randn(N, device=dev), torch.rsqrt(var + 1e-5)
        res = torch.randn(B, Ho, Wo, N, device=dev)
        out, y = torch.empty(B, Ho, Wo, N, device=dev), torch.empty(B, Ho, Wo, N, device=dev)
        slot = ops.amax_slot(dev)
        epi = ops.BnEpi(mean, invstd, gamma, beta, res, True, slot)
        log = ops.dispatch_log(True)
        conv = lambda bn=None: ops.conv2d_fwd(x, w4, stride, pad, out=out, w_owner=wd, bn=bn)
        conv()
        kind = "conv3" + ("+split" if "conv3:split" in log else "") if "conv3:fwd" in log else "gemm"
        ops.dispatch_log(False)
        a = t(conv)
        b = t(lambda: conv(epi))
        c = t(lambda: (conv(), ops.bn_apply(out.view(-1, N), res.view(-1, N), mean, invstd, gamma, beta, True, out=y.view(-1, N), y_amax=slot)))
        print(f"B{B} {H}x{W} {C}->{N} k{k} s{stride} [{kind}]:  plain store {a:7.1f} us   fused epilogue {b:7.1f} us   conv + bn_apply {c:7.1f} us   "
              f"fused - two launches {b - c:+7.1f} us{'   (SLOWER fused)' if b > c else ''}", flush=True)
