"""The element-wise, pooling / resampling, loss / selection, grid and optimizer kernels (csrc/convaux.hip, loss.hip, optim.hip,
grid.hip, the row gather / scatter of loss.hip, row_softmax of rowops.hip) at the edges the one-small-shape tests of
test_gpu_kernels.py do not reach: a second trip of the grid-stride loop, destinations that are accumulated into or written exactly
once, tied maxima, dropped trailing rows, empty inputs.  References are plain torch on the CPU in fp64 (or the oracle); every
tolerance is written where it is used.  Needs a real MI355X.

"Loop shape": these kernels launch at most 2048 blocks of 256 threads and loop with `i += stride`; a loop shape has more than
LOOP = 2048 * 256 work items (float4 items where the kernel is vectorised) and a ragged last trip."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import vbg_oracle as O

LOOP = 2048 * 256
U24 = 2.0 ** -24
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    from vbg import ops as _ops
    return _ops


def dev():
    return torch.device("cuda")


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=gen(seed)) * scale


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def close(a, b, rtol, atol):
    """|a - b| <= atol + rtol * |b| everywhere, in fp64 (b: the reference)"""
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    d = (a - b).abs()
    ok = bool((d <= atol + rtol * b.abs()).all()) and a.shape == b.shape
    if not ok:
        print("max abs", float(d.max()), "at", int(d.argmax()), "ref", float(b.flatten()[d.argmax()]))
    return ok


def within(a, ref, bound):
    """|a - ref| <= bound element-wise, in fp64"""
    d = (a.detach().cpu().double() - ref).abs()
    ok = bool((d <= bound).all())
    if not ok:
        k = int((d - bound).argmax())
        print("error", float(d.flatten()[k]), "bound", float(bound.flatten()[k]) if torch.is_tensor(bound) else bound, "at", k)
    return ok


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def call(ops, name, *args):
    """a C entry with raw arguments on the current stream; raises VbgError as the ops wrappers do"""
    ops.check(getattr(ops.lib, name)(*args, ops._stream()), name)


# ------------------------------------------------------------------------------------------
# max-pool 3x3 / s2 / p1
# ------------------------------------------------------------------------------------------
def _pool_input(kind, B, C, H, W):
    x = rnd(B, C, H, W, seed=1000 + H * 31 + W * 7 + C)
    if kind == "neg":            # the -inf padding must never win
        return -(x.abs() + 0.25)
    if kind == "tied":           # post-ReLU-like data: most windows hold their maximum more than once
        return torch.relu(torch.round(2 * x) / 2)
    return x


def _tied_share(x):
    """share of the pooling windows whose maximum occurs more than once inside the window"""
    B, C, H, W = x.shape
    cols = F.unfold(F.pad(x, (1, 1, 1, 1), value=float("-inf")), 3, stride=2).view(B, C, 9, -1)
    mx = cols.max(2, keepdim=True).values
    return float(((cols == mx).sum(2) > 1).float().mean())


def _check_maxpool(ops, x, bwd=True):
    d = dev()
    B, C, H, W = x.shape
    xr = x.clone().requires_grad_(True)
    y, idx = F.max_pool2d(xr, 3, 2, 1, return_indices=True)
    Ho, Wo = y.shape[2:]
    yo, am = ops.maxpool_fwd(nhwc(x).to(d))
    assert torch.equal(yo.cpu(), nhwc(y.detach()))
    assert torch.equal(am.cpu().long(), nhwc(idx))
    if not bwd:
        return
    gy = rnd(*y.shape, seed=7)
    y.backward(gy)
    gyd = nhwc(gy).to(d)
    dx = torch.full((B, H, W, C), NAN, device=d)          # "every dx element is written exactly once": nothing is left of the fill
    call(ops, "vbg_maxpool3x3s2_bwd", ops.P(gyd), ops.P(am), B, Ho, Wo, C, H, W, ops.P(dx))
    dxc = dx.cpu()
    assert not torch.isnan(dxc).any()
    ref = nhwc(xr.grad)
    hits = torch.zeros(B, C, H * W).scatter_add_(2, idx.view(B, C, -1), torch.ones(B, C, Ho * Wo)).view(B, C, H, W)
    once = nhwc(hits) <= 1                                # no sum of two windows' gradients: nothing to round
    assert torch.equal(dxc[once], ref[once])
    assert close(dxc, ref, 1e-6, 1e-6)
    assert torch.equal(ops.maxpool_bwd(gyd, am, H, W).cpu(), dxc)


@pytest.mark.parametrize("kind", ["randn", "neg", "tied"])
@pytest.mark.parametrize("C", [4, 68])
@pytest.mark.parametrize("H,W", [(1, 7), (2, 2), (13, 10), (9, 16)])
def test_maxpool(ops, H, W, C, kind):
    x = _pool_input(kind, 2, C, H, W)
    if kind == "tied":
        assert _tied_share(x) >= 0.2
    _check_maxpool(ops, x)


@pytest.mark.parametrize("kind", ["randn", "neg", "tied"])
@pytest.mark.parametrize("H,W", [(1, 7), (2, 2), (13, 10), (9, 16)])
def test_maxpool_fwd_scalar_channels(ops, H, W, kind):
    _check_maxpool(ops, _pool_input(kind, 2, 6, H, W), bwd=False)


@pytest.mark.parametrize("kind", ["randn", "tied"])
def test_maxpool_loop_shape(ops, kind):
    B, C, H, W = 2, 60, 131, 137
    assert B * 66 * 69 * C > LOOP and B * H * W * (C // 4) > LOOP          # forward items, backward float4 items
    _check_maxpool(ops, _pool_input(kind, B, C, H, W))


# ------------------------------------------------------------------------------------------
# AvgPool2d(2, 2)
# ------------------------------------------------------------------------------------------
def _check_avgpool2(ops, B, C, H, W, fwd=True, bwd=True):
    d = dev()
    x = rnd(B, C, H, W, seed=20 + H + W + C)
    if fwd:
        ref = F.avg_pool2d(x.double(), 2)
        got = ops.avgpool2_fwd(nhwc(x).to(d))
        assert got.shape == (B, H // 2, W // 2, C)
        # three fp32 additions of the window's four values, then an exact * 0.25
        assert within(nchw(got.cpu()), ref, 3 * U24 * 4 * F.avg_pool2d(x.double().abs(), 2))
    if bwd:
        gy = rnd(B, C, H // 2, W // 2, seed=21)
        xr = x.double().requires_grad_(True)
        F.avg_pool2d(xr, 2).backward(gy.double())
        dx = torch.full((B, H, W, C), NAN, device=d)
        call(ops, "vbg_avgpool2_bwd", ops.P(nhwc(gy).to(d)), B, H, W, C, ops.P(dx))
        dxc = dx.cpu()
        assert not torch.isnan(dxc).any()
        assert torch.equal(nchw(dxc).double(), xr.grad)             # dy * 0.25 is exact
        assert not dxc[:, 2 * (H // 2):].any() and not dxc[:, :, 2 * (W // 2):].any()          # dropped trailing row / column
        assert torch.equal(ops.avgpool2_bwd(nhwc(gy).to(d), H, W).cpu(), dxc)


@pytest.mark.parametrize("C", [4, 36])
@pytest.mark.parametrize("H,W", [(2, 2), (3, 5), (8, 6), (7, 7)])
def test_avgpool2(ops, H, W, C):
    _check_avgpool2(ops, 2, C, H, W)


def test_avgpool2_loop_shapes(ops):
    assert 4 * 65 * 64 * 33 > LOOP and 2 * 131 * 129 * 16 > LOOP
    _check_avgpool2(ops, 4, 132, 131, 129, bwd=False)
    _check_avgpool2(ops, 2, 64, 131, 129, fwd=False)


# ------------------------------------------------------------------------------------------
# sum-pool (the FPN backward of the nearest up-sampling), up-sampling, layout changes
# ------------------------------------------------------------------------------------------
def _check_sumpool(ops, B, H, W, C, f, accumulate):
    d = dev()
    hi = rnd(B, H, W, C, seed=30 + f)
    out0 = rnd(B, H // f, W // f, C, seed=31)
    s = F.avg_pool2d(nchw(hi).double(), f) * (f * f)
    sa = F.avg_pool2d(nchw(hi).double().abs(), f) * (f * f)
    ref = s + (nchw(out0).double() if accumulate else 0)
    out = out0.to(d)          # (without accumulate the old content must be gone)
    assert ops.sumpool(hi.to(d), f, out=out, accumulate=accumulate) is out
    # f * f additions (the last one the old content) of partial sums no larger than sum |x| + |out0|
    assert within(nchw(out.cpu()), ref, f * f * U24 * (sa + nchw(out0).double().abs()))


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("f", [1, 2, 4, 8])
def test_sumpool(ops, f, accumulate):
    _check_sumpool(ops, 2, 16, 24, 12, f, accumulate)


def test_sumpool_loop_shape(ops):
    assert 2 * 129 * 130 * 16 > LOOP
    _check_sumpool(ops, 2, 258, 260, 64, 2, True)


def _check_upsample2_add(ops, B, H, W, C):
    d = dev()
    lo, sk = rnd(B, H // 2, W // 2, C, seed=40), rnd(B, H, W, C, seed=41)
    ref = nhwc(F.interpolate(nchw(lo), scale_factor=2, mode="nearest")) + sk
    assert torch.equal(ops.upsample2_add(lo.to(d), sk.to(d)).cpu(), ref)


@pytest.mark.parametrize("B,H,W,C", [(2, 2, 2, 4), (2, 6, 10, 36), (1, 12, 8, 8), (2, 130, 130, 64)])
def test_upsample2_add(ops, B, H, W, C):
    assert (B, H, W, C) != (2, 130, 130, 64) or B * H * W * (C // 4) > LOOP
    _check_upsample2_add(ops, B, H, W, C)


@pytest.mark.parametrize("C", [1, 3, 40])
@pytest.mark.parametrize("f", [1, 2, 4])
def test_upsample_nhwc_to_nchw(ops, f, C):
    x = rnd(2, 5, 7, C, seed=42)
    ref = F.interpolate(nchw(x), scale_factor=f, mode="nearest")
    assert torch.equal(ops.upsample_nhwc_to_nchw(x.to(dev()), f).cpu(), ref)


def test_upsample_nhwc_to_nchw_loop_shape(ops):
    B, h, w, C, f = 2, 67, 65, 5, 4
    assert B * C * h * f * w * f > LOOP
    x = rnd(B, h, w, C, seed=43)
    assert torch.equal(ops.upsample_nhwc_to_nchw(x.to(dev()), f).cpu(), F.interpolate(nchw(x), scale_factor=f, mode="nearest"))


@pytest.mark.parametrize("C,HW", [(1, 1), (3, 33), (65, 31), (32, 64), (40, 1025)])
def test_layout_changes(ops, C, HW):
    d = dev()
    x = rnd(2, C, HW, 1, seed=44)          # [B, C, H = HW, W = 1]
    y = ops.nchw_to_nhwc(x.to(d))
    assert torch.equal(y.cpu(), x.permute(0, 2, 3, 1))
    assert torch.equal(ops.nhwc_to_nchw(y).cpu(), x)
    z = rnd(2, HW, 1, C, seed=45)
    assert torch.equal(ops.nhwc_to_nchw(z.to(d)).cpu(), z.permute(0, 3, 1, 2))


def test_pool_resample_argument_errors(ops):
    """what the entries refuse before any launch (their VBG_CHECK_ARG lines): the destination keeps its content"""
    d = dev()
    P = ops.P
    src = torch.zeros(4096, device=d)
    am = torch.zeros(4096, device=d, dtype=torch.int32)
    dst = torch.full((4096,), 7.0, device=d)

    def refused(name, *args):
        with pytest.raises(ops.VbgError):
            call(ops, name, *args)
        assert bool((dst == 7.0).all())

    refused("vbg_maxpool3x3s2_bwd", P(src), P(am), 2, 4, 4, 6, 8, 8, P(dst))           # C = 6
    refused("vbg_maxpool3x3s2_bwd", P(src), P(am), 2, 5, 4, 4, 8, 8, P(dst))           # Ho = 5 is not the pooled height of H = 8
    refused("vbg_avgpool2_fwd", P(src), 2, 8, 8, 6, P(dst))
    refused("vbg_avgpool2_bwd", P(src), 2, 8, 8, 6, P(dst))
    refused("vbg_sumpool", P(src), 2, 8, 8, 6, 2, P(dst), 0)
    refused("vbg_sumpool", P(src), 2, 9, 8, 4, 2, P(dst), 1)                           # H % f != 0
    refused("vbg_upsample2_add", P(src), P(src), 2, 8, 8, 6, P(dst))
    refused("vbg_upsample2_add", P(src), P(src), 2, 7, 8, 4, P(dst))                   # odd H
    refused("vbg_upsample2_add", P(src), P(src[1:]), 2, 8, 8, 4, P(dst))               # a view offset by one float
    refused("vbg_upsample2_add", P(src), P(src), 2, 8, 8, 4, P(dst[1:]))


# ------------------------------------------------------------------------------------------
# cross-entropy from (low-resolution) logits, row softmax
# ------------------------------------------------------------------------------------------
def _saturated(rows, ncls, seed):
    """rows = a common offset of +-2^13 plus multiples of 2^-8 in [-40, 40]: exact in fp32, and so is the subtraction of the row maximum"""
    # (offset + value stays below 2^14, where fp32 resolves 2^-10)
    g = gen(seed)
    v = torch.randint(-40 * 256, 40 * 256 + 1, (rows, ncls), generator=g).float() / 256
    dom = torch.rand(rows, generator=g) < 0.5          # half of the rows: one class at 40, the others at most 20 (its probability rounds to 1)
    top = F.one_hot(torch.randint(0, ncls, (rows,), generator=g), ncls).bool()
    v = torch.where(dom[:, None], torch.where(top, torch.tensor(40.0), v.clamp(max=20.0)), v)
    off = (torch.randint(0, 2, (rows, 1), generator=g).float() * 2 - 1) * 8192
    return v + off


def _check_ce(ops, logits, labels, elem, w, up=0, B=0, H=0, W=0, seed=0):
    """ce_fwd / ce_bwd (default form) on `logits` [rows, ncls] handed over as a column slice of an [rows, 80] tensor, the gradient added
    into the same slice of a non-zero destination with a device scalar and gmul = 0.3; -> the losses"""
    d = dev()
    rows, ncls = logits.shape
    ld, c0 = 80, 3
    wide = rnd(rows, ld, seed=seed + 1)
    wide[:, c0:c0 + ncls] = logits
    lg = wide.to(d)[:, c0:c0 + ncls]
    n = labels.numel() if elem is None else elem.numel()
    lab_d, el_d = labels.int().to(d), None if elem is None else elem.int().to(d)
    w_d = None if w is None else w.to(d)
    got = ops.ce_fwd(lg, el_d, lab_d, n, w_d, up, H, W)
    x = logits.double().requires_grad_(True)
    full = x
    if up:
        full = F.interpolate(x.view(B, H >> up, W >> up, ncls).permute(0, 3, 1, 2), scale_factor=1 << up, mode="nearest")
        full = full.permute(0, 2, 3, 1).reshape(-1, ncls)
    pick = torch.arange(labels.numel()) if elem is None else elem.long()
    ref = F.cross_entropy(full[pick], labels.long()[pick], weight=None if w is None else w.double(), reduction="none")
    assert bool(torch.isfinite(got).all())
    assert close(got, ref, 1e-5, 1e-6)
    gs = torch.tensor([1.7])
    (ref.sum() * 0.3 * float(gs)).backward()
    R = rnd(rows, ld, seed=seed + 2, scale=0.05)
    dl = R.to(d)
    ops.ce_bwd(lg, el_d, lab_d, n, w_d, gs.to(d), 0.3, up, H, W, dl[:, c0:c0 + ncls])
    want = R.double()
    want[:, c0:c0 + ncls] += x.grad
    dlc = dl.cpu()
    assert bool(torch.isfinite(dlc).all())
    assert close(dlc, want, 1e-4, 1e-6)
    assert torch.equal(dlc[:, :c0], R[:, :c0]) and torch.equal(dlc[:, c0 + ncls:], R[:, c0 + ncls:])
    return got


def _weights(ncls):
    w = torch.tensor([0.5, 0.0, 2.0, 1.5, 1.0, 0.25, 3.0])[torch.arange(ncls) % 7]
    return torch.tensor([0.7]) if ncls == 1 else w


@pytest.mark.parametrize("ncls", [1, 2, 5, 64])
def test_ce_strided_logits_repeated_picks(ops, ncls):
    rows, n = 1000, 700
    g = gen(50 + ncls)
    logits = rnd(rows, ncls, seed=51 + ncls, scale=2.0)
    labels = torch.randint(0, ncls, (rows,), generator=g)
    elem = torch.randint(0, rows, (n,), generator=g)
    elem[:40] = elem[40:80]                                 # (certainly repeated)
    _check_ce(ops, logits, labels, elem, _weights(ncls), seed=52)
    _check_ce(ops, logits, labels, None, None, seed=53)


@pytest.mark.parametrize("B,H,W", [(2, 16, 24), (2, 512, 520)])
def test_ce_upsampled_labels(ops, B, H, W):
    """up_shift = 2: 16 label cells read, and add their gradient into, one logits row; (2, 512, 520) is a loop shape"""
    assert (B, H, W) == (2, 16, 24) or B * H * W > LOOP
    ncls = 3
    logits = rnd(B * (H // 4) * (W // 4), ncls, seed=54, scale=2.0)
    labels = torch.randint(0, ncls, (B * H * W,), generator=gen(55))
    _check_ce(ops, logits, labels, None, torch.tensor([0.5, 2.0, 1.0]), up=2, B=B, H=H, W=W, seed=56)


@pytest.mark.parametrize("ncls", [2, 5, 64])
def test_ce_saturated_rows(ops, ncls):
    """saturated rows give finite results at the usual tolerances, and every loss that is exactly zero carries the same sign bit -- with a
    class of weight 0 among them (its elements' losses are zeros too).  The OHEM selection sorts these losses with a radix sort and is
    compared with torch's comparison sort, which keeps -0.0 and +0.0 tied; a radix sort on bit patterns orders -0.0 below +0.0."""
    rows = 2000
    logits = _saturated(rows, ncls, seed=57 + ncls)
    g = gen(58)
    labels = torch.where(torch.rand(rows, generator=g) < 0.6, logits.argmax(1), torch.randint(0, ncls, (rows,), generator=g))
    for w in (_weights(ncls), None):
        got = _check_ce(ops, logits, labels, None, w, seed=59).cpu()
        zero = got == 0
        assert int(zero.sum()) >= rows // 10                  # (a condition on this input: there are zeros to compare)
        if w is not None:
            assert bool(zero[labels == 1].all()) and bool((labels == 1).any())
        sign = bits(got)[zero] < 0
        assert bool(sign.all()) or not bool(sign.any()), (int(sign.sum()), int(zero.sum()))


@pytest.mark.parametrize("cols", [1, 2, 5, 64])
@pytest.mark.parametrize("rows", [1, 255, 256, 257, 5000])
def test_row_softmax(ops, rows, cols):
    x = rnd(rows, cols, seed=60 + cols, scale=3.0)
    x[::2] = _saturated(rows, cols, seed=61)[::2]
    y = ops.row_softmax(x.to(dev())).cpu()
    assert bool(torch.isfinite(y).all())
    assert close(y, torch.softmax(x.double(), 1), 1e-5, 1e-6)
    # y_c = e_c * (1 / s), s the fp32 sum of the e_c: cols - 1 additions, one division, one product each
    assert within(y.double().sum(1), torch.ones(rows, dtype=torch.float64), cols * 2.0 ** -23)


# ------------------------------------------------------------------------------------------
# selection: compaction, stable descending sort, gathers, row scatter, sums
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 257, 2 ** 20 + 3])
def test_compact(ops, n):
    d = dev()
    g = gen(70 + n % 1000)
    for value in (2, -3):
        cases = {"none": torch.full((n,), value + 1), "all": torch.full((n,), value),
                 "half": torch.where(torch.rand(n, generator=g) < 0.5, torch.tensor(value), torch.randint(-5, 6, (n,), generator=g))}
        for name, lab in cases.items():
            for eq in (True, False):
                idx, cnt = ops.compact(lab.int().to(d), value, eq)
                ref = torch.nonzero((lab == value) == eq).flatten()
                k = int(cnt.item())
                assert k == ref.numel(), (name, value, eq)
                assert torch.equal(idx[:k].cpu().long(), ref), (name, value, eq)


def _sort_keys(n, seed):
    """multiples of 1/4 (heavy ties, negative values), +-inf and subnormals; every zero is +0.0: a radix sort on bit patterns orders -0.0 below
    +0.0, torch's comparison sort keeps them tied, so the two are compared without a mix of the two zeros"""
    g = gen(seed)
    k = torch.round(rnd(n, seed=seed + 1) * 4) / 4 + 0.0
    special = torch.tensor([float("inf"), float("-inf"), 1e-40, -1e-40, 3e-45, -3e-45, 1e-40, float("inf")])
    if n >= 16:
        pos = torch.randperm(n, generator=g)[:n // 8]
        k[pos] = special[torch.randint(0, 8, (pos.numel(),), generator=g)]
    elif n == 2:
        k = torch.tensor([1e-40, 1e-40])
    assert not bool(((k == 0) & (bits(k) < 0)).any())
    return k


@pytest.mark.parametrize("n", [1, 2, 257, 2 ** 20 + 5])
def test_sort_desc(ops, n):
    d = dev()
    for keys in (_sort_keys(n, 80 + n % 1000), torch.full((n,), -0.0), torch.full((n,), 0.75)):
        ko, io = ops.sort_desc(keys.to(d))
        rs, ri = torch.sort(keys, descending=True, stable=True)
        assert torch.equal(bits(ko), bits(rs))
        assert torch.equal(io.cpu().long(), ri)


@pytest.mark.parametrize("n", [1, LOOP + 4099])
def test_gather_scalars(ops, n):
    d = dev()
    g = gen(90)
    idx = torch.randint(0, 300, (n,), generator=g)
    idx[-1] = idx[0]
    sf, si = rnd(300, seed=91), torch.randint(-2 ** 31, 2 ** 31 - 1, (300,), generator=g).int()
    assert torch.equal(ops.gather_f32(sf.to(d), idx.int().to(d)).cpu(), sf[idx])
    assert torch.equal(ops.gather_i32(si.to(d), idx.int().to(d)).cpu(), si[idx])


ROW_SHAPES = [(1, 1), (1, 5), (1, 256), (LOOP + 4099, 1), (105001, 5), (2049, 256)]


@pytest.mark.parametrize("n,C", ROW_SHAPES)
def test_gather_rows(ops, n, C):
    assert n == 1 or n * C > LOOP
    src = rnd(300, C, seed=92)
    idx = torch.randint(0, 300, (n,), generator=gen(93))
    idx[-1] = idx[0]
    assert torch.equal(ops.gather_rows(src.to(dev()), idx.int().to(dev())).cpu(), src[idx])


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("n,C", ROW_SHAPES)
def test_scatter_rows_add(ops, n, C, det):
    """onto a non-zero destination; every destination row receives zero, one or two source rows, so at most two roundings"""
    d = dev()
    R = n // 2 + 3
    g = gen(94)
    idx = torch.cat([torch.randperm(R, generator=g), torch.randperm(R, generator=g)])[:n]
    idx = idx[torch.randperm(n, generator=g)]
    if n > 1:
        assert int(torch.bincount(idx).max()) == 2
    src, dst0 = rnd(n, C, seed=95), rnd(R, C, seed=96)
    ref = dst0.double().index_add_(0, idx, src.double())
    mag = dst0.double().abs().index_add_(0, idx, src.double().abs())
    dst = dst0.to(d)
    with ops.deterministic_scope(det):
        ops.scatter_rows_add(src.to(d), idx.int().to(d), dst)
    assert within(dst.cpu(), ref, 2.0 ** -23 * mag)


@pytest.mark.parametrize("n", [1, 1023, 1025, 3 * 10 ** 6 + 7])
def test_sums(ops, n):
    """sum_f32 / sumsq add into `out`.  The kernels' own summation order: G = min(ceil(n / 1024), 2048) blocks; a thread adds
    k = ceil(n / (256 G)) terms in sequence (k - 1 roundings), the block reduces in 6 + 3 additions, and G atomics land on `out`"""
    d = dev()
    x = rnd(n, seed=97)
    G = min(-(-n // 1024), 2048)
    k = -(-n // (256 * G))
    for name, terms, extra in (("sum_f32", x.double(), 0), ("sumsq", x.double() ** 2, 1)):          # (sumsq: one rounding per square)
        out = torch.tensor([3.25], device=d)
        getattr(ops, name)(x.to(d), out)
        ref = 3.25 + terms.sum()
        bound = (k + 8 + G + extra) * U24 * (float(terms.abs().sum()) + 3.25)
        err = abs(float(out.cpu().double()) - float(ref))
        print(name, n, "error", err, "bound", bound)
        assert err <= bound


# ------------------------------------------------------------------------------------------
# BERTgrid: owner map, scatter and the accumulating backward kernels
# ------------------------------------------------------------------------------------------
def _pack_boxes(boxes):
    off = [0]
    for b in boxes:
        off.append(off[-1] + b.shape[0])
    allb = torch.cat([b.int() for b in boxes], 0) if off[-1] else torch.zeros((0, 4), dtype=torch.int32)
    doc = torch.cat([torch.full((b.shape[0],), i, dtype=torch.int32) for i, b in enumerate(boxes)]) if off[-1] else torch.zeros((0,), dtype=torch.int32)
    return allb.contiguous(), torch.tensor(off, dtype=torch.int32), doc


def _random_boxes(n, extent, g):
    """as test_owner_map_random_large: overlapping, border-crossing and zero-area boxes on an extent x extent pixel page"""
    x1 = torch.randint(-10, extent - 12, (n,), generator=g)
    y1 = torch.randint(-10, extent - 12, (n,), generator=g)
    w = torch.randint(0, 73, (n,), generator=g)
    h = torch.randint(0, 25, (n,), generator=g)
    return torch.stack([x1, y1, x1 + w, y1 + h], 1).int()


def _owner_case(stride, n):
    """documents of 700, 0 and 257 boxes (the kernel stages 256 rectangles at a time through LDS); the first box of the last document
    covers the page, so it -- the only box of that document's second chunk -- owns whatever the other 256 leave free"""
    g = gen(100 + stride)
    boxes = [_random_boxes(700, n * stride, g), torch.zeros((0, 4), dtype=torch.int32), _random_boxes(257, n * stride, g)]
    boxes[2][0] = torch.tensor([0, 0, n * stride, n * stride], dtype=torch.int32)
    refs, base = [], 0
    for b in boxes:
        r = O.owner_map(b.numpy(), n, n, stride)
        refs.append(np.where(r >= 0, r + base, -1))
        base += b.shape[0]
    return boxes, np.stack(refs)


@pytest.mark.parametrize("stride,n", [(8, 64), (1, 96)])
def test_owner_map_lds_chunks_and_empty_document(ops, stride, n):
    d = dev()
    boxes, ref = _owner_case(stride, n)
    allb, off, _ = _pack_boxes(boxes)
    own = ops.owner_map(allb.to(d), off.to(d), 3, n, n, stride).cpu().numpy()
    assert np.array_equal(own, ref)
    assert (own[1] == -1).all() and (own[2] == 700).any()
    if stride == 8:
        assert (own[0] == -1).any() and ((own[0] >= 0) & (own[0] < 700 - 512)).any()          # owners in the third chunk of document 0


def test_owner_map_and_scatter_without_boxes(ops):
    d = dev()
    allb, off, _ = _pack_boxes([torch.zeros((0, 4), dtype=torch.int32)] * 2)
    own = ops.owner_map(allb.to(d), off.to(d), 2, 16, 24, 8)
    assert bool((own == -1).all())
    emb = torch.zeros((0, 8), device=d)
    for layout, shape in ((0, (2, 16, 24, 8)), (1, (2, 8, 16, 24))):
        assert torch.equal(ops.grid_scatter_fwd(emb, own, 8, layout=layout), torch.zeros(shape, device=d))
        grid = torch.full(shape, NAN, device=d)
        call(ops, "vbg_grid_scatter_fwd", None, ops.P(own), 2, 16, 24, 8, layout, ops.P(grid))
        assert not bool(grid.any())


def test_grid_scatter_fwd_nhwc_loop_shape(ops):
    d = dev()
    C, n = 116, 96
    assert 3 * n * n * (C // 4) > LOOP
    boxes, ref = _owner_case(1, n)
    emb = rnd(957, C, seed=101)
    own = torch.from_numpy(ref).int()
    want = torch.where((own >= 0)[..., None], emb[own.clamp(min=0).long()], torch.zeros(()))
    assert torch.equal(ops.grid_scatter_fwd(emb.to(d), own.to(d), C, layout=0).cpu(), want)
    assert torch.equal(ops.grid_scatter_fwd(emb.to(d), own.to(d), C, layout=1).cpu(), nchw(want))


def test_grid_scatter_bwd_accumulates(ops, golden):
    """test_owner_scatter_bitexact's backward case onto a non-zero destination"""
    g = golden("scatter.npz")
    H, W = int(g["H"]), int(g["W"])
    boxes = [torch.from_numpy(g[f"box{b}"]) for b in range(3)]
    allb, off, doc = _pack_boxes(boxes)
    d = dev()
    own = ops.owner_map(allb.to(d), off.to(d), 3, H // 8, W // 8, 8)
    gout = torch.from_numpy(g["gout"]).permute(0, 2, 3, 1).contiguous()
    R = rnd(allb.shape[0], 6, seed=102)
    demb = R.to(d)
    ops.grid_scatter_bwd(gout.to(d), own, allb.to(d), doc.to(d), 8, demb)
    ref = torch.from_numpy(np.concatenate([g[f"gemb{b}"] for b in range(3)], 0)).double() + R.double()
    assert close(demb, ref, 1e-5, 1e-6)


def test_seg_reduce_bwd_accumulates(ops, golden):
    """test_seg_reduce_bitexact's backward case onto a non-zero destination"""
    g = golden("aggregate.npz")
    d = dev()
    for mode, mi in (("mean", 0), ("first", 1)):
        tok, mask = torch.from_numpy(g[f"{mode}_tok"]), torch.from_numpy(g[f"{mode}_mask"])
        B, T, Hd = tok.shape
        rows, starts, lens, base = [], [], [], 0
        for b in range(B):
            r = torch.nonzero(mask[b] == 1).flatten() + b * T
            st, ln = O.seg_runs(torch.from_numpy(g[f"{mode}_seg{b}"]))
            starts += list(st + base)
            lens += list(ln)
            base += r.numel()
            rows.append(r)
        rows = torch.cat(rows).int().to(d)
        starts, lens = torch.tensor(starts, dtype=torch.int32, device=d), torch.tensor(lens, dtype=torch.int32, device=d)
        gy = rnd(starts.numel(), Hd, seed=103)
        R = rnd(B * T, Hd, seed=104)
        dt = R.to(d)
        ops.seg_reduce_bwd(gy.to(d), rows, starts, lens, mi, dt)
        tk = tok.reshape(B * T, Hd).clone().requires_grad_(True)
        embs = [O.seg_aggregate(tk.view(B, T, Hd)[b], mask[b], torch.from_numpy(g[f"{mode}_seg{b}"]), mode) for b in range(B)]
        torch.cat(embs).backward(gy)
        assert close(dt, R.double() + tk.grad.double(), 1e-6, 1e-7)


@pytest.mark.parametrize("det", [False, True])
def test_roi_align_bwd_accumulates(ops, det):
    """test_roi_align's backward case onto a non-zero dfeat, atomic and fixed-order form"""
    B, C_, H, W = 2, 32, 24, 32
    feat = rnd(B, C_, H, W, seed=100).requires_grad_(True)
    boxes = [torch.tensor([[0, 0, 128, 96], [3, 5, 40, 22], [100, 80, 140, 120], [10, 10, 11, 11], [60, 40, 61, 90]], dtype=torch.int32),
             torch.tensor([[5, 7, 77, 30], [120, 90, 128, 96], [0, 50, 30, 52]], dtype=torch.int32)]
    ref = O.roi_align(feat, [b.float() for b in boxes], 7, 0.25)
    gy = rnd(*ref.shape, seed=101)
    ref.backward(gy)
    allb, off, doc = _pack_boxes(boxes)
    d = dev()
    R = rnd(B, H, W, C_, seed=105)
    df = R.to(d)
    with ops.deterministic_scope(det):
        ops.roi_align_bwd(nhwc(gy).to(d), (B, H, W, C_), allb.to(d), doc.to(d), 7, 0.25, df)
    assert close(df, R.double() + nhwc(feat.grad).double(), 1e-4, 1e-5)


# ------------------------------------------------------------------------------------------
# optimizers
# ------------------------------------------------------------------------------------------
OPT_N = [1, 3, 4, 5, 1023, 2097152 + 1203]
PAD = 8


def f32(v):
    """the value a `float` argument of the C entries has"""
    return float(np.float32(v))


def _views(ops, tensors, unaligned):
    """device copies of `tensors` inside larger buffers filled with a sentinel: at float offset 1 (not 16-byte aligned) or 4 (aligned);
    -> (views, check) where check() asserts that nothing outside the views changed"""
    bufs, views = [], []
    for t, un in zip(tensors, unaligned):
        off = 1 if un else 4
        buf = torch.full((t.numel() + PAD,), 123.5, device=dev())
        buf[off:off + t.numel()] = t.to(dev())
        v = buf[off:off + t.numel()]
        assert (v.data_ptr() % 16 != 0) == un
        bufs.append((buf, off, t.numel()))
        views.append(v)

    def check():
        for buf, off, n in bufs:
            assert bool((buf[:off] == 123.5).all()) and bool((buf[off + n:] == 123.5).all())
    return views, check


def _opt_inputs(n, steps=3):
    """parameters ~ N(0, 1); each element's gradients keep one sign over the steps (magnitudes 0.25 ... 3, independent per step), so the
    momentum / first-moment sums do not cancel and the relative tolerance below holds for any correct fp32 evaluation of the rule"""
    g = gen(110 + n % 1000)
    p = rnd(n, seed=111 + n % 1000)
    s = (torch.randint(0, 2, (n,), generator=g).float() * 2 - 1) * (0.5 + 1.5 * torch.rand(n, generator=g))
    return p, [s * (0.5 + torch.rand(n, generator=g)) for _ in range(steps)]


CONFIGS = {"aligned": (False, False, False, False), "views": (True, True, True, True), "grad_unaligned": (False, True, False, False)}


def sgd_ref(p, g, mom, lr, momentum, wd, first, gs):
    """torch.optim.SGD (dampening 0, no nesterov) with the gradient scaled by gs, in fp64"""
    d = g * gs + wd * p
    mom = d if first else momentum * mom + d
    return p - lr * mom, mom


def adamw_ref(p, g, m, v, lr, b1, b2, eps, wd, step, gs):
    """torch.optim.AdamW (amsgrad off) with the gradient scaled by gs, in fp64"""
    g = g * gs
    p = p * (1 - lr * wd)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    denom = v.sqrt() / (1 - b2 ** step) ** 0.5 + eps
    return p - lr / (1 - b1 ** step) * (m / denom), m, v


def test_adamw_restatement_is_torch_adamw():
    p0, gs_ = _opt_inputs(1023)
    lr, b1, b2, eps, wd = f32(1e-3), f32(0.9), f32(0.999), f32(1e-8), f32(0.01)
    pt = p0.double().clone().requires_grad_(True)
    opt = torch.optim.AdamW([pt], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    p, m, v = p0.double(), torch.zeros(1023, dtype=torch.float64), torch.zeros(1023, dtype=torch.float64)
    for i, g in enumerate(gs_):
        pt.grad = g.double()
        opt.step()
        p, m, v = adamw_ref(p, g.double(), m, v, lr, b1, b2, eps, wd, i + 1, 1.0)
    assert torch.allclose(p, pt.detach(), rtol=1e-12, atol=1e-14)
    assert torch.allclose(m, opt.state[pt]["exp_avg"], rtol=1e-12, atol=1e-14) and torch.allclose(v, opt.state[pt]["exp_avg_sq"], rtol=1e-12, atol=1e-14)


def _opt_cases(base, variants):
    """every size in every alignment configuration with the base hyper-parameters; the variants of the rule aligned, at one tail shape
    and at the loop shape"""
    return [(n, c) + base for n in OPT_N for c in CONFIGS] + [(n, "aligned") + v for n in (5, OPT_N[-1]) for v in variants]


@pytest.mark.parametrize("n,config,momentum,wd", _opt_cases((0.9, 0.005), [(0.0, 0.005), (0.9, 0.0)]))
def test_sgd_step(ops, n, config, momentum, wd):
    lr, momentum, wd = f32(0.005), f32(momentum), f32(wd)
    p0, grads = _opt_inputs(n)
    for gs in (1.0, 0.125):
        un = CONFIGS[config]
        mom0 = rnd(n, seed=112)                   # (first step: whatever the buffer holds is overwritten)
        (p, mom), check = _views(ops, (p0, mom0), (un[0], un[2]))
        pr, mr = p0.double(), mom0.double()
        for i, g in enumerate(grads):
            (gd,), gcheck = _views(ops, (g,), (un[1],))
            ops.sgd_step(p, gd, mom, lr, momentum, wd, i == 0, gs)
            pr, mr = sgd_ref(pr, g.double(), mr, lr, momentum, wd, i == 0, gs)
            assert torch.equal(gd.cpu(), g)
            gcheck()
        assert close(p, pr, 1e-6, 1e-7), (n, config, gs)
        assert close(mom, mr, 1e-6, 1e-7), (n, config, gs)
        check()


@pytest.mark.parametrize("n,config,wd,step0", _opt_cases((0.01, 1), [(0.0, 1), (0.01, 1000)]))
def test_adamw_step(ops, n, config, wd, step0):
    lr, b1, b2, eps, wd = f32(1e-3), f32(0.9), f32(0.999), f32(1e-8), f32(wd)
    p0, grads = _opt_inputs(n)
    m0, v0 = torch.zeros(n), torch.zeros(n)
    if step0 > 1:                                 # a late step on given moments: bias corrections 1 - b^step far from their first values
        m0, v0 = grads[0] * 0.1 * (0.5 + torch.rand(n, generator=gen(113))), 1e-3 * (0.1 + torch.rand(n, generator=gen(114)))
    for gs in (1.0, 0.125):
        un = CONFIGS[config]
        (p, m, v), check = _views(ops, (p0, m0, v0), (un[0], un[2], un[3]))
        pr, mr, vr = p0.double(), m0.double(), v0.double()
        for i, g in enumerate(grads):
            (gd,), gcheck = _views(ops, (g,), (un[1],))
            ops.adamw_step(p, gd, m, v, lr, b1, b2, eps, wd, step0 + i, gs)
            pr, mr, vr = adamw_ref(pr, g.double(), mr, vr, lr, b1, b2, eps, wd, step0 + i, gs)
            assert torch.equal(gd.cpu(), g)
            gcheck()
        assert close(p, pr, 1e-6, 1e-7), (n, config, gs)
        assert close(m, mr, 1e-6, 1e-7), (n, config, gs)
        assert close(v, vr, 1e-6, 1e-7), (n, config, gs)
        check()


def test_clip_grad_norm(ops):
    from vbg import optim as vopt
    d = dev()
    shapes = {"a.weight": (37, 5), "a.bias": (13,), "b.weight": (3, 64), "b.bias": (1,)}
    params = {k: torch.nn.Parameter(rnd(*s, seed=120 + i).to(d)) for i, (k, s) in enumerate(shapes.items())}
    grads = {k: rnd(*s, seed=130 + i) for i, (k, s) in enumerate(shapes.items())}
    opts = [vopt.FusedSGD([(k, params[k]) for k in ("a.weight", "a.bias")], d, lr=0.01, momentum=0.9),
            vopt.FusedAdamW([(k, params[k]) for k in ("b.weight", "b.bias")], d, lr=1e-3)]
    norm = float(torch.cat([g.double().flatten() for g in grads.values()]).norm())
    for max_norm in (0.5 * norm, 2.0 * norm):          # above the threshold (scaled) and below it (untouched)
        copies = [torch.nn.Parameter(torch.zeros(s, dtype=torch.float64)) for s in shapes.values()]
        for c, k in zip(copies, shapes):
            c.grad = grads[k].double().clone()
            params[k].grad.copy_(grads[k].to(d))
        ref = float(torch.nn.utils.clip_grad_norm_(copies, max_norm))
        got = vopt.clip_grad_norm_(opts, max_norm)
        assert abs(got - ref) <= 1e-6 * ref
        for c, k in zip(copies, shapes):
            assert close(params[k].grad, c.grad, 1e-6, 1e-7), k
            if max_norm > norm:
                assert torch.equal(params[k].grad.cpu(), grads[k])
