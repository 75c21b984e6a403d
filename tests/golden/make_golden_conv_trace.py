"""Generate tests/golden/conv_launch_trace.json: which leaf wrappers a convolution product calls, in which order and with which
kernel-selecting arguments, for every route of the dispatch under every switch that bears on it.  No GPU needed.

    python tests/golden/make_golden_conv_trace.py [output file]

The leaf wrappers (ops.conv3x3, conv3x3_wgrad, conv3x3_wflip, conv3_planes, amax, im2col, gemm_raw) are replaced by recorders and
ops.conv2d_fwd / conv2d_dgrad / conv2d_wgrad and functions._conv_any / _conv_wgrad_any are called on meta tensors, so the script runs
unchanged on any commit that has these names: the committed fixture was written by the commit BEFORE the three products took their
kernel, form and amax routing from one plan each (DESIGN.md "Convolution plans"), and tests/test_conv_plan_host.py replays `trace()`
below against it, entry for entry.

Beside the leaf wrappers two things are recorded or relaxed, because nothing launches here: Tensor.zero_ (whether a weight gradient is
cleared first is part of the split-k / accumulate rule), and ops._chk_f32, which insists on device memory (here: dtype only).
ops.conv2d_* are not called for the stem (3 input channels): at the recording commit only functions._conv_any took it."""
import contextlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

# (x NHWC, Cout, k, stride, pad): the routes of tests/golden/make_golden_conv_bits.py SHAPES ...
ROUTE_SHAPES = [((1, 128, 128, 256), 128, 3, 1, 1), ((1, 128, 128, 128), 128, 3, 1, 1), ((1, 32, 32, 256), 256, 3, 1, 1),
                ((8, 32, 32, 256), 256, 3, 1, 1), ((1, 16, 16, 512), 512, 3, 1, 1), ((480, 7, 7, 128), 128, 3, 1, 1),
                ((2, 128, 128, 64), 64, 3, 1, 1), ((1, 16, 16, 64), 32, 1, 1, 0), ((1, 16, 16, 16), 32, 3, 2, 1), ((1, 32, 32, 3), 64, 7, 2, 3)]
# ... and every convolution of one training step of the bench configuration (batch 8 at 512 x 512, ResNet-34 + FPN, 128 regions per
# document) as (H, W, Cin, Cout, k, stride), pad = k // 2: the forward calls tools/conv_shapes.py lists on an MI355X, and the stem, which
# it did not see at the recording commit (the im2col product did not pass ops.conv2d_fwd)
BENCH_B, BENCH_ROI_B = 8, 8 * 128
BENCH_CONVS = [(512, 512, 3, 64, 7, 2), (7, 7, 256, 256, 3, 1), (16, 16, 512, 256, 1, 1), (16, 16, 512, 512, 3, 1), (32, 32, 256, 256, 1, 1),
               (32, 32, 256, 256, 3, 1), (32, 32, 256, 512, 1, 2), (32, 32, 256, 512, 3, 2), (64, 64, 128, 128, 3, 1), (64, 64, 128, 256, 1, 1),
               (64, 64, 128, 256, 1, 2), (64, 64, 128, 256, 3, 2), (64, 64, 256, 256, 3, 1), (128, 128, 64, 64, 3, 1), (128, 128, 64, 128, 1, 2),
               (128, 128, 64, 128, 3, 2), (128, 128, 64, 256, 1, 1), (128, 128, 256, 3, 1, 1), (128, 128, 256, 5, 1, 1), (128, 128, 256, 256, 3, 1)]

SETTINGS = ("default", "conv3_off", "conv3_f16_off", "conv3_splitk_off", "deterministic", "amp_fast", "amp_generic")


def shapes():
    out = list(ROUTE_SHAPES)
    for H, W, Ci, Co, k, s in BENCH_CONVS:
        B = BENCH_ROI_B if (H, W) == (7, 7) else BENCH_B
        sh = ((B, H, W, Ci), Co, k, s, k // 2)
        if sh not in out:
            out.append(sh)
    return out


@contextlib.contextmanager
def setting(ops, name):
    """one switch away from the defaults (restored on exit)"""
    prev = (ops._CONV3[0], ops._CONV3_F16[0], ops._CONV3_SPLITK[0], ops._AMP_FAST[0])
    scope = contextlib.nullcontext()
    if name == "conv3_off":
        ops.set_conv3(False)
    elif name == "conv3_f16_off":
        ops.set_conv3_f16(False)
    elif name == "conv3_splitk_off":
        ops._CONV3_SPLITK[0] = False
    elif name == "deterministic":
        scope = ops.deterministic_scope(True)
    elif name in ("amp_fast", "amp_generic"):
        ops.set_amp_fast(name == "amp_fast")
        scope = ops.amp_scope(True)
    else:
        assert name == "default", name
    try:
        with scope:
            yield
    finally:
        ops._CONV3[0], ops._CONV3_F16[0], ops._CONV3_SPLITK[0], ops._AMP_FAST[0] = prev


class _Planes:
    """what the conv3_planes recorder hands out for a filter that has an owner"""


@contextlib.contextmanager
def recorders(ops, log):
    """the leaf wrappers as recorders that append [name, {kernel-selecting arguments}] to `log` and return a tensor of the right shape"""
    f32 = torch.float32

    def has(v):
        return v is not None

    def conv3x3(x, w_ohwi, bias=None, out=None, stats=None, accumulate=False, f16x2=False, x_amax=None, nsplit=None, w_planes=None, n_out=None,
                bn=0, bn_epi=None):
        log.append(["conv3x3", dict(f16x2=bool(f16x2), nsplit=nsplit, bn=int(bn), n_out=n_out, accumulate=bool(accumulate), w_planes=has(w_planes),
                                    x_amax=has(x_amax), stats=has(stats), bias=has(bias), bn_epi=has(bn_epi))])
        N = w_ohwi.shape[0] if n_out is None else int(n_out)
        return out if out is not None else torch.empty(tuple(x.shape[:3]) + (N,), device=x.device, dtype=f32)

    def conv3x3_wgrad(dy, x, dw_ohwi, slabs=True, f16x2=False, dy_amax=None, x_amax=None):
        log.append(["conv3x3_wgrad", dict(slabs=bool(slabs), f16x2=bool(f16x2), dy_amax=has(dy_amax), x_amax=has(x_amax))])
        return dw_ohwi

    def conv3x3_wflip(w_ohwi):
        log.append(["conv3x3_wflip", {}])
        Cout, _, _, Cin = w_ohwi.shape
        return torch.empty((Cin, 3, 3, Cout), device=w_ohwi.device, dtype=f32)

    def conv3_planes(owner, w_ohwi, flip, bn=0):
        log.append(["conv3_planes", dict(owner=has(owner), flip=bool(flip), bn=int(bn))])
        return _Planes() if owner is not None else None

    def amax(x, slot=None):
        log.append(["amax", dict(slot=has(slot))])
        return torch.empty((1,), device=x.device, dtype=torch.int32) if slot is None else slot

    def im2col(x, kh, kw, stride, pad, Kpad):
        log.append(["im2col", dict(k=[kh, kw], stride=stride, pad=pad, Kpad=Kpad)])
        B, H, W, _ = x.shape
        Ho, Wo = ops.conv_out_hw(H, W, kh, stride, pad)
        return torch.empty((B * Ho * Wo, Kpad), device=x.device, dtype=f32)

    def gemm_raw(M, N, K, A, lda, a_kind, B, ldb, b_kind, Cout, ldc, *, bias=None, accumulate=False, splitk=1, geo=None, stats=None, f16=False,
                 bn=None, **other):
        assert not other, other
        log.append(["gemm_raw", dict(mnk=[int(M), int(N), int(K)], ld=[int(lda), int(ldb), int(ldc)], a_kind=int(a_kind), b_kind=int(b_kind),
                                     accumulate=bool(accumulate), splitk=int(splitk), f16=bool(f16), bias=has(bias), stats=has(stats), bn_epi=has(bn),
                                     geo=None if geo is None else [geo.Hs, geo.Ws, geo.Cs, geo.Hr, geo.Wr, geo.kh, geo.kw, geo.stride, geo.pad, geo.dgrad])])

    def chk_f32(*ts):
        for t in ts:
            assert t is None or t.dtype == f32

    zero_ = torch.Tensor.zero_

    def rec_zero_(t):
        log.append(["zero_", {}])
        return zero_(t)

    new = dict(conv3x3=conv3x3, conv3x3_wgrad=conv3x3_wgrad, conv3x3_wflip=conv3x3_wflip, conv3_planes=conv3_planes, amax=amax, im2col=im2col,
               gemm_raw=gemm_raw, _chk_f32=chk_f32)
    old = {k: getattr(ops, k) for k in new}
    for k, v in new.items():
        setattr(ops, k, v)
    torch.Tensor.zero_ = rec_zero_
    try:
        yield
    finally:
        torch.Tensor.zero_ = zero_
        for k, v in old.items():
            setattr(ops, k, v)


def _param(shape_oihw, sunk):
    """a filter parameter in channels_last memory on the meta device; sunk: with the flat gradient view the weight gradient goes into"""
    w = torch.empty(shape_oihw, device="meta").contiguous(memory_format=torch.channels_last)
    if sunk:
        w._vbg_sunk = True
        w.grad = torch.empty(shape_oihw, device="meta").contiguous(memory_format=torch.channels_last)
    return w


def calls(ops, Fn, shape):
    """[(label, thunk)]: every call variant of one convolution shape"""
    (B, H, W, Ci), Co, k, s, p = shape
    Ho, Wo = ops.conv_out_hw(H, W, k, s, p)
    meta = dict(device="meta", dtype=torch.float32)
    x, dy = torch.empty((B, H, W, Ci), **meta), torch.empty((B, Ho, Wo, Co), **meta)
    word = torch.empty((1,), device="meta", dtype=torch.int32)
    vec = torch.empty((Co,), **meta)
    out = []
    for owned in (False, True):
        wp = _param((Co, Ci, k, k), False)
        w4 = Fn.ohwi(wp)
        own = wp if owned else None
        o = f"owner{int(owned)}"
        if Ci % 16 == 0:
            out.append((f"fwd/{o}", lambda w4=w4, own=own: ops.conv2d_fwd(x, w4, s, p, w_owner=own)))
            out.append((f"fwd/{o}/bias+stats+amax", lambda w4=w4, own=own: ops.conv2d_fwd(x, w4, s, p, bias=vec, stats=vec, w_owner=own, x_amax=word)))
            out.append((f"fwd/{o}/bn_epi", lambda w4=w4, own=own: ops.conv2d_fwd(x, w4, s, p, w_owner=own, x_amax=word, bn=_Planes())))
            out.append((f"dgrad/{o}", lambda w4=w4, own=own: ops.conv2d_dgrad(dy, w4, (B, H, W, Ci), s, p, w_owner=own)))
            out.append((f"dgrad/{o}/amax+acc", lambda w4=w4, own=own: ops.conv2d_dgrad(dy, w4, (B, H, W, Ci), s, p, out=torch.empty((B, H, W, Ci), **meta),
                                                                                       accumulate=True, dy_amax=word, w_owner=own)))
        out.append((f"any/{o}", lambda w4=w4, own=own: Fn._conv_any(x, w4, s, p, w_owner=own, x_amax=word)))
        out.append((f"any/{o}/bias+bn_epi", lambda w4=w4, own=own: Fn._conv_any(x, w4, s, p, bias=vec, w_owner=own, bn=_Planes())))
    if Ci % 16 == 0:
        for acc in (False, True):
            out.append((f"wgrad/acc{int(acc)}", lambda acc=acc: ops.conv2d_wgrad(dy, x, torch.empty((Co, k, k, Ci), **meta), s, p, accumulate=acc)))
            out.append((f"wgrad/acc{int(acc)}/amax", lambda acc=acc: ops.conv2d_wgrad(dy, x, torch.empty((Co, k, k, Ci), **meta), s, p, accumulate=acc,
                                                                                      dy_amax=word, x_amax=word)))

    def wgrad_any(sunk, amax):
        # the col buffer is what the forward of the same node returned
        col = Fn._conv_any(x, Fn.ohwi(_param((Co, Ci, k, k), False)), s, p)[1]
        mark = len(LOG[0])
        Fn._conv_wgrad_any(dy, x, col, (Co, k, k, Ci), s, p, _param((Co, Ci, k, k), True) if sunk else None,
                           dy_amax=word if amax else None, x_amax=word if amax else None)
        del LOG[0][:mark]          # (the forward's own entries are those of "any/...")

    for sunk in (False, True):
        for amax in (False, True):
            out.append((f"wgrad_any/sunk{int(sunk)}/amax{int(amax)}", lambda sunk=sunk, amax=amax: wgrad_any(sunk, amax)))
    return out


LOG = [None]


def trace(ops, Fn):
    """{"setting|shape|call": [[leaf wrapper, {arguments}], ...]}"""
    table = {}
    for name in SETTINGS:
        for shape in shapes():
            (B, H, W, Ci), Co, k, s, p = shape
            tag = f"{B}x{H}x{W}x{Ci}->{Co} k{k} s{s} p{p}"
            for label, thunk in calls(ops, Fn, shape):
                LOG[0] = log = []
                with setting(ops, name), recorders(ops, log), torch.no_grad():
                    thunk()
                table[f"{name}|{tag}|{label}"] = log
    return table


def pack(table):
    """the file's form: most calls share their trace with others (a switch that does not bear on the shape, a shape on the same route),
    so each distinct trace is stored once, one per line, its entries as [wrapper, values in the order of "fields"] --
    {"fields": {wrapper: [argument names]}, "traces": [...], "calls": {shape: {call: index, or [index per setting of SETTINGS]}}}"""
    fields, traces, where, calls = {}, [], {}, {}
    for key, log in table.items():
        name, tag, label = key.split("|")
        for wrapper, args in log:
            assert fields.setdefault(wrapper, sorted(args)) == sorted(args)
        text = json.dumps([[wrapper] + [args[k] for k in fields[wrapper]] for wrapper, args in log], separators=(",", ":"))
        if text not in where:
            where[text] = len(traces)
            traces.append(text)
        calls.setdefault(tag, {}).setdefault(label, [None] * len(SETTINGS))[SETTINGS.index(name)] = where[text]
    lines = ['{"fields": ' + json.dumps(fields) + ",", '"traces": ['] + [" " + t + ("," if i + 1 < len(traces) else "") for i, t in enumerate(traces)]
    lines.append('], "calls": {')
    for i, (tag, labels) in enumerate(calls.items()):
        labels = {k: v[0] if len(set(v)) == 1 else v for k, v in labels.items()}          # (one index: the same under every setting)
        lines.append(f' {json.dumps(tag)}: ' + json.dumps(labels, separators=(",", ":")) + ("," if i + 1 < len(calls) else ""))
    return "\n".join(lines + ["}}"]) + "\n"


def unpack(packed):
    """{"setting|shape|call": [[wrapper, {arguments}], ...]} again"""
    traces = [[[e[0], dict(zip(packed["fields"][e[0]], e[1:]))] for e in t] for t in packed["traces"]]
    return {f"{name}|{tag}|{label}": traces[idx if isinstance(idx, int) else idx[i]] for tag, labels in packed["calls"].items()
            for label, idx in labels.items() for i, name in enumerate(SETTINGS)}


def main():
    for d in ("oracle", "vibertgrid-pytorch_amd", "tests"):
        sys.path.insert(0, os.path.join(ROOT, d))
    from vbg import functions as Fn
    from vbg import ops
    table = trace(ops, Fn)
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "conv_launch_trace.json")
    with open(out, "w") as f:
        f.write(pack(table))
    names = sorted({e[0] for log in table.values() for e in log})
    print("wrote", out, os.path.getsize(out), "bytes", len(table), "calls", names)


if __name__ == "__main__":
    main()
