"""Frozen BatchNorm as the epilogue of the convolution in front of it (include/vbg.h vbg_bn_epilogue): every kernel variant that
carries it, on the smallest shape that reaches the variant.

Ground truth: z from the SAME convolution launched without the epilogue (same instance, same accumulators), then in fp64 on the host
    y64 = relu?((z - mean) * invstd * gamma + beta + res).
Gate, elementwise:  |y - y64| <= 6 * 2^-24 * (|z - mean| * invstd * |gamma| + |beta| + |res|).
Derived, not measured: the expression is at most five fp32 roundings (subtract, two multiplies, two adds -- fewer where the compiler
contracts a multiply-add), each at most 2^-24 of a partial result that the bracket bounds; ReLU is 1-Lipschitz; one more 2^-24 covers the
second-order terms.  The two-launch route (convolution + vbg_bn_apply) is held to the same gate in the same test: one yardstick for both.
Whether the two routes agree bit for bit is printed, not asserted (the compiler may contract differently in the two kernels)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 1e-5
U = 2.0 ** -24


def _params(C, dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    sign = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    gamma = (0.5 + torch.rand(C, generator=g)) * sign                      # both signs
    beta = torch.randn(C, generator=g)
    mean = 0.3 * torch.randn(C, generator=g)
    var = 1e-3 + (4.0 - 1e-3) * torch.rand(C, generator=g)                # running_var in [1e-3, 4]
    var[0], var[1] = 1e-3, 4.0
    mean, var, gamma, beta = (t.to(dev) for t in (mean, var, gamma, beta))
    return mean, torch.rsqrt(var + EPS), gamma, beta


def _slot_value(slot):
    from vbg import ops
    return int(slot.view(ops.AMAX_WORDS, ops.AMAX_STRIDE)[:, 0].max())


def _gate(tag, y, z, mean, invstd, gamma, beta, res, relu):
    z64 = z.double().reshape(-1, z.shape[-1]).cpu()
    mu, is_, ga, be = (t.double().cpu() for t in (mean, invstd, gamma, beta))
    r64 = None if res is None else res.double().reshape(-1, z.shape[-1]).cpu()
    y64 = (z64 - mu) * is_ * ga + be
    bound = (z64 - mu).abs() * is_ * ga.abs() + be.abs()
    if r64 is not None:
        y64 = y64 + r64
        bound = bound + r64.abs()
    if relu:
        y64 = y64.clamp(min=0)
    err = (y.double().reshape(-1, z.shape[-1]).cpu() - y64).abs()
    ratio = float((err / (6 * U * bound).clamp(min=1e-300)).max())
    print(f"{tag}: max |y - y64| / bound = {ratio:.3f}")
    assert torch.isfinite(y).all()
    assert ratio <= 1.0, (tag, ratio)


def _check(tag, launch, C, res_shape, dev, seed):
    """launch(bn) -> the convolution's output, bn = None (plain store) or an ops.BnEpi; residual / ReLU on and off"""
    from vbg import ops
    mean, invstd, gamma, beta = _params(C, dev, seed)
    with torch.no_grad():
        z = launch(None)
        for has_res, relu in ((True, True), (False, False), (True, False), (False, True)):
            res = torch.randn(res_shape, device=dev) if has_res else None
            slot_f, slot_a = ops.amax_slot(dev), ops.amax_slot(dev)
            y = launch(ops.BnEpi(mean, invstd, gamma, beta, res, relu, slot_f))
            assert y.shape == z.shape and y.data_ptr() != z.data_ptr()
            ya = ops.bn_apply(z.view(-1, C), None if res is None else res.view(-1, C), mean, invstd, gamma, beta, relu, y_amax=slot_a).view(z.shape)
            t = f"{tag} res={int(has_res)} relu={int(relu)}"
            _gate(t + " fused", y, z, mean, invstd, gamma, beta, res, relu)
            _gate(t + " bn_apply", ya, z, mean, invstd, gamma, beta, res, relu)
            print(f"{t}: fused torch.equal two-launch: {torch.equal(y, ya)}")
            # the amax word: the slot's maximum is the bit pattern of max |y|, exactly
            assert _slot_value(slot_f) == int(y.abs().max().view(torch.int32)), t
            assert _slot_value(slot_a) == int(ya.abs().max().view(torch.int32)), t
    return z


def _conv3_inputs(shape, N, dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    B, H, W, Cs = shape
    x = torch.randn(shape, generator=g).to(dev)
    w = (torch.randn((N, 3, 3, Cs), generator=g) / (9 * Cs) ** 0.5).to(dev)
    return x, w


def _conv3_launch(x, w, *, f16x2, planes_bn=None, nsplit=1):
    from vbg import ops
    wp = None if planes_bn is None else ops.conv3_planes(w, w, False, bn=planes_bn)
    assert planes_bn is None or wp is not None

    def launch(bn):
        return ops.conv3x3(x, w, f16x2=f16x2, w_planes=wp, nsplit=nsplit, bn=planes_bn or 0, bn_epi=bn)
    return launch


CONV3 = [
    # (id, x shape, filters, f16x2, plane image's filters per tile (None: the fp32 filter), nsplit)
    ("n64_planes_two_tiles", (1, 16, 16, 64), 64, True, 64, 1),            # <128, 64, F16, PW>, two pixel tiles
    ("n64_f16", (1, 16, 16, 64), 64, True, None, 1),                      # the fp32 filter, fp16-pair form (64-pixel tiles)
    ("n64_bf16x3", (1, 16, 16, 64), 64, False, None, 1),                  # the fp32 filter, three bf16 pieces
    ("n128_f16", (2, 8, 16, 128), 128, True, None, 1),                    # vbg_conv3x3, F16
    ("n128_planes", (2, 8, 16, 128), 128, True, 128, 1),                  # <128, 128, F16, PW>
    ("wide_row_f16", (1, 2, 128, 32), 128, True, None, 1),                # W = 128: <128, 128, F16> from the fp32 filter
    ("wide_row_bf16x3", (1, 2, 128, 32), 128, False, None, 1),            # <128, 128> three bf16 pieces
    ("roi_f16", (3, 7, 7, 256), 256, True, None, 1),                      # region form, partial last slot grid (3 images, 2 per tile)
    ("roi_planes", (3, 7, 7, 256), 256, True, 128, 1),
    ("roi_bf16x3", (3, 7, 7, 256), 256, False, None, 1),
]


@pytest.mark.parametrize("tag,shape,N,f16x2,planes_bn,nsplit", CONV3, ids=[c[0] for c in CONV3])
def test_conv3_epilogue(tag, shape, N, f16x2, planes_bn, nsplit):
    dev = torch.device("cuda")
    x, w = _conv3_inputs(shape, N, dev, 11)
    B, H, W, _ = shape
    _check(tag, _conv3_launch(x, w, f16x2=f16x2, planes_bn=planes_bn, nsplit=nsplit), N, (B, H, W, N), dev, 5)


def test_conv3_epilogue_split_finisher_is_deterministic():
    """512 -> 512 at 16 x 16 with conv3_late_choice: 64-filter tiles, four workgroups per tile -- only the finishing workgroup applies the
    epilogue, after adding the slabs in block order; twice the same bits"""
    from vbg import ops
    dev = torch.device("cuda")
    shape, N = (1, 16, 16, 512), 512
    late = ops.conv3_late_choice(*shape, N)
    assert late == (64, 4), late
    x, w = _conv3_inputs(shape, N, dev, 12)
    launch = _conv3_launch(x, w, f16x2=True, planes_bn=late[0], nsplit=late[1])
    log = ops.dispatch_log(True)
    try:
        _check("late_split", launch, N, (1, 16, 16, N), dev, 6)
        assert log.get("conv3:split", 0) > 0 and log.get("conv3:bn64", 0) > 0 and log.get("bn:epilogue_conv3", 0) == 4, log
    finally:
        ops.dispatch_log(False)
    mean, invstd, gamma, beta = _params(N, dev, 6)
    res = torch.randn((1, 16, 16, N), device=dev)
    outs = []
    for _ in range(2):
        slot = ops.amax_slot(dev)
        y = launch(ops.BnEpi(mean, invstd, gamma, beta, res, True, slot))
        outs.append((y, _slot_value(slot)))
    assert torch.equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1]


def test_conv3_epilogue_one_product_form():
    """a plane-image launch inside an autocast region: the one-product (ONEP) instance"""
    from vbg import ops
    dev = torch.device("cuda")
    shape, N = (2, 8, 16, 128), 128
    x, w = _conv3_inputs(shape, N, dev, 13)
    ops.set_amp(True)
    log = ops.dispatch_log(True)
    try:
        _check("onep", _conv3_launch(x, w, f16x2=True, planes_bn=128), N, (2, 8, 16, N), dev, 7)
        assert log.get("conv3:onep", 0) > 0, log
    finally:
        ops.dispatch_log(False)
        ops.set_amp(False)


def _conv_inputs(shape, N, k, dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(shape, generator=g).to(dev)
    w = (torch.randn((N, k, k, shape[3]), generator=g) / (k * k * shape[3]) ** 0.5).to(dev)
    return x, w


GEMM = [
    # (id, x shape, filters, kernel, stride, pad)
    ("dense_1x1", (1, 8, 8, 64), 256, 1, 1, 0),                           # DENSE_K, 64 x 64 tiles
    ("conv_3x3_s2", (1, 16, 16, 64), 128, 3, 2, 1),                       # CONV_K
    ("shortcut_1x1_s2", (1, 16, 16, 64), 128, 1, 2, 0),                   # the strided 1x1 shortcut
]
FORMS = ["f16x2", "bf16x3", "amp", "fp32", "tile128128"]


class _form:
    """the arithmetic form / tile of the generic kernel for the launches inside"""

    def __init__(self, form):
        self.form = form

    def __enter__(self):
        from vbg import ops
        f = self.form
        if f == "bf16x3":
            ops.set_gemm_f16(False)
        elif f == "amp":
            ops.set_amp(True)
        elif f == "fp32":
            ops.set_precision("fp32")
        elif f == "tile128128":
            ops._FORCE[0] = 128128
        return self

    def __exit__(self, *exc):
        from vbg import ops
        ops.set_gemm_f16(True)
        ops.set_amp(False)
        ops.set_precision("split")
        ops._FORCE[0] = 0


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("tag,shape,N,k,stride,pad", GEMM, ids=[c[0] for c in GEMM])
def test_gemm_epilogue(tag, shape, N, k, stride, pad, form):
    """the generic kernel's kinds x every arithmetic form (vbg_gemm_desc.bf16 = 2, 3, 1, 0) and the forced 128 x 128 tile"""
    from vbg import ops
    dev = torch.device("cuda")
    x, w = _conv_inputs(shape, N, k, dev, 21)
    Ho, Wo = ops.conv_out_hw(shape[1], shape[2], k, stride, pad)
    with _form(form):
        log = ops.dispatch_log(True)
        try:
            _check(f"{tag}/{form}", lambda bn: ops.conv2d_fwd(x, w, stride, pad, bn=bn), N, (shape[0], Ho, Wo, N), dev, 8)
            assert log.get("bn:epilogue_gemm", 0) == 4 and "conv3:fwd" not in log, log
            if form in ("f16x2", "bf16x3"):
                assert log.get("gemm:" + form, 0) > 0, log
        finally:
            ops.dispatch_log(False)


@pytest.mark.parametrize("form", ["split", "fp32"])
def test_gemm_epilogue_stem_im2col(form):
    """the stem: 7 x 7 / s2 over 3 channels through im2col (Kp = 148), M = 81 rows: the row guard of a 64-row tile"""
    from vbg import functions as Fn
    dev = torch.device("cuda")
    x, w = _conv_inputs((1, 18, 18, 3), 64, 7, dev, 22)
    with _form(form):
        z = _check(f"stem/{form}", lambda bn: Fn._conv_any(x, w, 2, 3, bn=bn)[0], 64, (1, 9, 9, 64), dev, 9)
    assert z.shape == (1, 9, 9, 64)


def test_gemm_epilogue_never_skipped_on_the_per_lane_store_path():
    """the fp32 form's 16-deep k-tiles under a 128-row tile store per lane, where the epilogue does not exist: the library refuses the
    launch instead of storing the unnormalised product"""
    from vbg import ops
    from vbg.lib import VbgError
    dev = torch.device("cuda")
    x, w = _conv_inputs((1, 16, 16, 64), 128, 1, dev, 23)
    mean, invstd, gamma, beta = _params(128, dev, 3)
    with _form("fp32"), torch.no_grad():
        ops._FORCE[0] = 128128
        ops.conv2d_fwd(x, w, 1, 0)                                                      # (K = 64: 16-deep k-tiles) fine without
        with pytest.raises(VbgError):
            ops.conv2d_fwd(x, w, 1, 0, bn=ops.BnEpi(mean, invstd, gamma, beta))


def test_argument_errors():
    """every combination the epilogue does not go with is an argument error (< 0), returned before any launch"""
    import ctypes as C
    from vbg import ops
    from vbg.lib import BnEpilogue, VbgError, lib
    from vbg.lib import EPI_RELU, OP_DENSE_K
    dev = torch.device("cuda")
    M, N, K = 64, 64, 256
    a, b = torch.randn(M, K, device=dev), torch.randn(N, K, device=dev)
    out, out2 = torch.empty(M, N, device=dev), torch.empty(M, N, device=dev)
    mean, invstd, gamma, beta = _params(N, dev, 1)
    res = torch.randn(M * N + 4, device=dev)
    bn = lambda **kw: ops.BnEpi(mean, invstd, gamma, beta, **kw)

    def gemm(bn_, n=N, c=out, **kw):
        ops.gemm_raw(M, n, K, a, K, OP_DENSE_K, b, K, OP_DENSE_K, c, n, bn=bn_, **kw)

    with torch.no_grad():
        gemm(bn(res=res[: M * N].view(M, N), relu=True, amax=ops.amax_slot(dev)))      # the legal launch
        bad = [
            dict(stats=ops._bn_workspace(dev, N)),
            dict(accumulate=True),
            dict(splitk=0),
            dict(splitk=2, accumulate=True),
            dict(splitk=2, slab_stride=M * N, c=torch.empty(2, M, N, device=dev)),
            dict(grp=torch.tensor([[M, N, K, 0, 0, 0, 0, 0]], device=dev, dtype=torch.int64), ngroups=1, grp_max=(M, N)),
            dict(C2=out2),
            dict(epi=EPI_RELU),
            dict(bias=beta),
            dict(n=N - 2),                                                              # N % 4 != 0
            dict(c_ptr_off=1, c=torch.empty(M * N + 4, device=dev)),                    # output not 16-byte aligned
        ]
        for kw in bad:
            with pytest.raises(VbgError):
                gemm(bn(), **kw)
        with pytest.raises(VbgError):
            gemm(bn(res=res[1: M * N + 1].view(M, N)))                                  # residual not 16-byte aligned
        with pytest.raises(VbgError):
            gemm(bn(res=out))                                                           # residual aliasing the output

        # vbg_conv3x3_bn
        x, w = _conv3_inputs((2, 8, 16, 128), 128, dev, 2)
        mean, invstd, gamma, beta = _params(128, dev, 1)
        y = torch.empty(2, 8, 16, 128, device=dev)
        wp = ops.conv3_planes(w, w, False, bn=128)
        P = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        s = ops._stream()

        def conv3(e, w_=w, wp_=None, y_=y, n=128, form=1, bn_tile=0):
            return lib.vbg_conv3x3_bn(P(x), P(w_), P(wp_), P(y_), 2, 8, 16, 128, n, form, None, None, None, 1, bn_tile,
                                      None if e is None else C.byref(e), s)
        ok = ops.BnEpi(mean, invstd, gamma, beta).fill(BnEpilogue())
        assert conv3(ok) == 0 and conv3(ok, None, wp, bn_tile=128) == 0
        assert conv3(None) < 0                                                          # no epilogue given
        assert conv3(BnEpilogue()) < 0                                                  # a zeroed epilogue
        assert conv3(ok, w, wp) < 0 and conv3(ok, None, None) < 0                       # exactly one filter form
        assert conv3(ok, form=2) < 0 and conv3(ok, None, wp, form=0) < 0                # forms of the other filter form
        assert conv3(ok, n=126) < 0                                                     # N % 4 != 0
        assert conv3(ok, y_=y.view(-1)[1:]) < 0                                         # output not 16-byte aligned
        assert conv3(ops.BnEpi(mean, invstd, gamma, beta, res=torch.empty(y.numel() + 4, device=dev)[1:]).fill(BnEpilogue())) < 0
        assert conv3(ops.BnEpi(mean, invstd, gamma, beta, res=y).fill(BnEpilogue())) < 0   # residual aliasing the output
        with pytest.raises(VbgError):                                                   # bias / stats / accumulate have no place in the entry point
            ops.conv3x3(x, w, bias=beta, f16x2=True, nsplit=1, bn_epi=ops.BnEpi(mean, invstd, gamma, beta))
        torch.cuda.synchronize()
