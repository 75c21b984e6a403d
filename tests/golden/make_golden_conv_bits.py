"""Generate tests/golden/conv_bits.npz: what the convolution nodes (vbg.functions.ConvFn / ConvBnFn) leave, forward and backward, recorded
on the GPU.

    python tests/golden/make_golden_conv_bits.py [output file]

Needs a real MI355X and the built library.  Every call goes through ConvFn.apply / ConvBnFn.apply and the public switches of vbg.ops, so
the script runs unchanged on any commit that has them: the committed fixture was written by the commit BEFORE the nodes took their kernel,
form and amax routing from one plan per pass (DESIGN.md "Convolution plans"), and tests/test_gpu_conv_bits.py replays `run_case` below
against it.

Per case and tensor (y, dx, dw, db, dgamma, dbeta, dres, running_mean, running_var) the fixture holds a SHA-256 of the bytes and eight
values at fixed flat indices -- a mismatch says roughly where --, never the tensor; and the ops.dispatch_log dict of the case, in
deterministic mode and in the default mode.  Bits are recorded in deterministic mode only (the default mode adds BatchNorm statistics with
float atomics).  Inputs come from seeded CPU generators, one set per shape.

SHAPES: the smallest at which each route of the dispatch is reached at default settings; `routes()` states what each is there for in
terms of the predicates, and main() asserts it before anything is recorded."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

# name: (x NHWC, Cout, k, stride, pad)
SHAPES = {
    "wide256": ((1, 128, 128, 256), 128, 3, 1, 1),       # row-reuse fwd + dgrad + wgrad, 128-pixel tiles, pre-split filter
    "wide128": ((1, 128, 128, 128), 128, 3, 1, 1),       # row-reuse fwd, generic dgrad (256 tiles < 480)
    "late4": ((1, 32, 32, 256), 256, 3, 1, 1),           # late stage, 64-filter tiles, 4 workgroups per tile
    "late1": ((8, 32, 32, 256), 256, 3, 1, 1),           # late stage, 64-filter tiles, 1 workgroup per tile
    "last": ((1, 16, 16, 512), 512, 3, 1, 1),            # last stage, statistics not fused (K = 4608)
    "roi": ((480, 7, 7, 128), 128, 3, 1, 1),             # 7 x 7 region maps
    "bn64": ((2, 128, 128, 64), 64, 3, 1, 1),            # 64-wide filter tiles (odd multiple of 64)
    "g1x1": ((1, 16, 16, 64), 32, 1, 1, 0),              # generic 1x1 / s1 / p0
    "g3x3s2": ((1, 16, 16, 16), 32, 3, 2, 1),            # generic 3x3 / s2 / p1
    "stem": ((1, 32, 32, 3), 64, 7, 2, 3),               # stem 7x7 / s2 / p3, Cin = 3 (im2col; the image takes no gradient)
}
# ConvBnFn with a backward: (training statistics, residual, ReLU); the no-grad frozen call with set_bn_epilogue(True): (residual, ReLU)
BN_CASES = [(t, r, a) for t in (True, False) for r in (False, True) for a in (False, True)]
EPI_CASES = [(r, a) for r in (False, True) for a in (False, True)]
TENSORS = ("y", "dx", "dw", "db", "dgamma", "dbeta", "dres", "running_mean", "running_var")
NSAMPLE = 8


def routes(ops):
    """{shape: True when the predicates, at default settings, send the shape where SHAPES says}"""
    ok = {}

    def late(n):
        return ops.conv3_late_choice(*SHAPES[n][0], SHAPES[n][1])

    def c3(n, **k):
        (B, H, W, Ci), Co, kk, s, p = SHAPES[n]
        return ops.conv3_ok(B, H, W, Ci, Co, kk, kk, s, p, **k)

    def c3d(n):
        (B, H, W, Ci), Co, kk, s, p = SHAPES[n]
        return ops.conv3_ok(B, H, W, Co, Ci, kk, kk, s, p)

    def c3w(n):
        (B, H, W, Ci), Co, kk, s, p = SHAPES[n]
        return ops.conv3w_ok(B, H, W, Ci, Co, kk, kk, s, p)

    (B, H, W, Ci), Co = SHAPES["wide256"][:2]
    ok["wide256"] = c3("wide256", fwd=True) and c3d("wide256") and c3w("wide256") and late("wide256") is None and ops.conv3_pw_ok(B, H, W, Ci, Co) \
        and ops.conv3_pw_ok(B, H, W, Co, Ci)
    ok["wide128"] = c3("wide128", fwd=True) and not c3d("wide128") and late("wide128") is None
    ok["late4"] = c3("late4", fwd=True) and late("late4") == (64, 4)
    ok["late1"] = c3("late1", fwd=True) and late("late1") == (64, 1)
    (B, H, W, Ci), Co = SHAPES["last"][:2]
    ok["last"] = c3("last", fwd=True) and not ops.fuse_stats_ok(B * H * W, Co, 9 * Ci)
    ok["roi"] = c3("roi", fwd=True) and c3w("roi")
    ok["bn64"] = c3("bn64", fwd=True) and c3w("bn64")
    for n in ("g1x1", "g3x3s2", "stem"):
        ok[n] = not c3(n, fwd=True) and not c3d(n) and not c3w(n)
    return ok


def inputs(name):
    """the CPU tensors of one shape, from one seeded generator: x, w (OIHW), bias, gamma, beta, running mean / var, residual, dy"""
    (B, H, W, Ci), Co, k, s, p = SHAPES[name]
    g = torch.Generator().manual_seed(4000 + sorted(SHAPES).index(name))
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    return {"x": torch.randn(B, H, W, Ci, generator=g), "w": torch.randn(Co, Ci, k, k, generator=g) / (Ci * k * k) ** 0.5,
            "b": 0.1 * torch.randn(Co, generator=g), "gamma": 1 + 0.1 * torch.randn(Co, generator=g), "beta": 0.05 * torch.randn(Co, generator=g),
            "rm": 0.1 * torch.randn(Co, generator=g), "rv": 0.5 + torch.rand(Co, generator=g), "res": torch.randn(B, Ho, Wo, Co, generator=g),
            "dy": torch.randn(B, Ho, Wo, Co, generator=g)}


def case_ids():
    """[(id, shape, kind, args)]: kind "conv" (ConvFn with bias), "bn" (ConvBnFn forward + backward) or "epi" (no-grad frozen epilogue call)"""
    out = []
    for n in SHAPES:
        out.append((f"{n}/conv", n, "conv", ()))
        out += [(f"{n}/bn/{'train' if t else 'frozen'}/res{int(r)}/relu{int(a)}", n, "bn", (t, r, a)) for t, r, a in BN_CASES]
        out += [(f"{n}/epi/res{int(r)}/relu{int(a)}", n, "epi", (r, a)) for r, a in EPI_CASES]
    return out


def digest(t):
    """(sha256 hex of the bytes, NSAMPLE float32 bit patterns at fixed flat indices)"""
    a = t.detach().contiguous().cpu().view(-1).view(torch.int32).numpy().view(np.uint32)
    idx = (np.arange(NSAMPLE, dtype=np.int64) * 2654435761 + 12345) % a.size
    return hashlib.sha256(a.tobytes()).hexdigest(), a[idx].copy()


def run_case(ops, Fn, dev, src, name, kind, args):
    """one case on the device -> ({tensor: (sha256, samples)}, dispatch dict).  The caller sets the mode (ops.deterministic_scope)."""
    (B, H, W, Ci), Co, k, s, p = SHAPES[name]
    grad_x = Ci % 4 == 0                                                  # (the stem's image takes no gradient)
    x = src["x"].to(dev).requires_grad_(grad_x and kind != "epi")
    w = src["w"].to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(kind != "epi")
    dy = src["dy"].to(dev)
    got = {}
    torch.cuda.synchronize()
    log = ops.dispatch_log(True)
    try:
        if kind == "conv":
            b = src["b"].to(dev).requires_grad_(True)
            y = Fn.ConvFn.apply(x, w, b, s, p)
            y.backward(dy)
            got = {"y": y, "dx": x.grad, "dw": w.grad, "db": b.grad}
        else:
            gamma, beta = (src[n].to(dev).requires_grad_(kind == "bn") for n in ("gamma", "beta"))
            rm, rv = src["rm"].to(dev), src["rv"].to(dev)
            if kind == "bn":
                training, has_res, relu = args
                res = src["res"].to(dev).requires_grad_(True) if has_res else None
                y = Fn.ConvBnFn.apply(x, w, gamma, beta, rm, rv, res, s, p, relu, training, 0.1, 1e-5, False)
                y.backward(dy)
                got = {"y": y, "dx": x.grad, "dw": w.grad, "dgamma": gamma.grad, "dbeta": beta.grad, "dres": None if res is None else res.grad}
            else:
                has_res, relu = args
                res = src["res"].to(dev) if has_res else None
                was = ops.bn_epilogue_enabled()
                ops.set_bn_epilogue(True)
                try:
                    with torch.no_grad():
                        y = Fn.ConvBnFn.apply(x, w, gamma, beta, rm, rv, res, s, p, relu, False, 0.1, 1e-5, False)
                finally:
                    ops.set_bn_epilogue(was)
                got = {"y": y}
            got.update(running_mean=rm, running_var=rv)
        torch.cuda.synchronize()
    finally:
        log = dict(log)
        ops.dispatch_log(False)
    return {n: digest(t) for n, t in got.items() if t is not None}, log


def main():
    for d in ("oracle", "vibertgrid-pytorch_amd", "tests"):
        sys.path.insert(0, os.path.join(ROOT, d))
    from vbg import functions as Fn
    from vbg import ops
    bad = [n for n, v in routes(ops).items() if not v]
    assert not bad, bad
    dev = torch.device("cuda")
    rec, src_name, src = {}, None, None
    for cid, name, kind, args in case_ids():
        if name != src_name:
            src_name, src = name, inputs(name)
        with ops.deterministic_scope(True):
            got, log_det = run_case(ops, Fn, dev, src, name, kind, args)
            again, _ = run_case(ops, Fn, dev, src, name, kind, args)
        assert all(got[n][0] == again[n][0] for n in got), cid          # the same bits on a second call
        with ops.deterministic_scope(False):
            _, log_def = run_case(ops, Fn, dev, src, name, kind, args)
        rec[cid] = (got, log_det, log_def)
        print(cid, sorted(got), json.dumps(log_def, sort_keys=True))
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "conv_bits.npz")
    save(out, rec)
    print("wrote", out, os.path.getsize(out), "bytes", len(case_ids()), "cases")


def save(out, rec):
    """{case: ({tensor: (sha256 hex, samples)}, dispatch dict in deterministic mode, in default mode)} -> four arrays: the names
    "case:tensor" and the dispatch dicts as JSON text, the hashes [n, 32] uint8, the samples [n, NSAMPLE] uint32"""
    names = [f"{cid}:{t}" for cid, (got, _, _) in rec.items() for t in got]
    sha = np.array([list(bytes.fromhex(got[t][0])) for got, _, _ in rec.values() for t in got], dtype=np.uint8)
    samples = np.stack([got[t][1] for got, _, _ in rec.values() for t in got]).astype(np.uint32)
    dispatch = {cid: [det, default] for cid, (_, det, default) in rec.items()}
    np.savez_compressed(out, names=np.array(json.dumps(names)), sha=sha, samples=samples, dispatch=np.array(json.dumps(dispatch, sort_keys=True)))


def load(fix):
    """the inverse of save(), from the opened .npz"""
    dispatch = json.loads(str(fix["dispatch"]))
    rec = {cid: ({}, det, default) for cid, (det, default) in dispatch.items()}
    for name, sha, samples in zip(json.loads(str(fix["names"])), fix["sha"], fix["samples"]):
        cid, t = name.rsplit(":", 1)
        rec[cid][0][t] = (bytes(sha.tolist()).hex(), samples)
    return rec


if __name__ == "__main__":
    main()
