"""Every instance of the generic GEMM / implicit-GEMM convolution kernel (csrc/gemm.hip gemm_kernel<BM, BN, BK, NT, AK, BKD, VEC, PREC>) against
an fp64 CPU reference at its edges: the cases of tests/gemm_cases.py (ragged M / N for the instance's own tile, reductions off the k-tile
depth, NaN operand padding, sentinel around C, every epilogue on both store paths, alpha, accumulate, splits that leave a split empty or
start inside a filter tap / an image, the automatic and the slab split, fused statistics, the A prologue, K segments, groups, and the
convolution forward / data-gradient / weight-gradient gathers on odd maps).

Reference: torch matmul / F.conv2d in double (autograd for the two convolution gradients) on the operands as the form that RUNS sees
them -- ops.gemm_variant's prec: 1 rounds them to bf16 after the prologue, 0 / 2 / 3 leave them as they are.
Error unit: |got - ref| / (|a| @ |b|), as tests/test_gpu_kernels.py::test_split_form_is_fp32_grade; the bound is that test's 2e-6 up to
K = 640 and 2e-6 sqrt(K / 640) beyond.  alpha, the bias and the accumulate start enter the unit with their own magnitude
(|alpha| (|a| @ |b|) + |bias| + |c0|: each adds one fp32 rounding of a term that size); ReLU is 1-Lipschitz and keeps the bound.  Where the
unit is zero (the dx pixels a strided 1x1 convolution never reads) the result must be exactly the reference.
A split product is compared once, against fp64 only: the order of its atomics is free.

Each case first asserts that the library reports the instance the table names for it (vbg_gemm_variant), so the test cannot thin out
when the dispatch heuristic moves.  tools/gemm_variants_profile.py writes the largest error seen per instance to profiles/gemm_variants.txt."""
import pytest
import torch

import gemm_cases as G

pytestmark = pytest.mark.gpu

f64 = torch.float64


@pytest.fixture(scope="module")
def ops():
    from vbg import ops as _ops
    return _ops


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752440))


def run_case(c, ops, dev=None):
    """runs one case; returns its largest error in the unit above.  Raises AssertionError on a wrong instance, a touched sentinel, an
    error above the bound (a NaN is one), a wrong GELU image or wrong statistics"""
    from vbg.lib import lib
    dev = dev or torch.device("cuda")
    p = G.Problem(c, dev, ops)
    with G.form_state(ops, p.form):
        got_v = tuple(ops.gemm_variant(*p.args, **p.kw))
        assert got_v == c.expect, (c.name, "instance", c.expect, got_v)
        ops.gemm_raw(*p.args, **p.kw)
        if c.slab:
            ops.check(lib.vbg_slab_reduce(ops.P(p.slabs), c.splitk, p.M * p.N, p.M, p.N, p.N, ops.P(p.bias_dev), 1, ops.P(p.c_buf), p.ldc, ops._stream()),
                      "vbg_slab_reduce")
    torch.cuda.synchronize()
    return check_case(p, got_v)


def check_case(p, got_v):
    """the output of a finished launch against the sentinel and the fp64 reference"""
    c = p.case
    out = p.c_buf.cpu()
    # ---- nothing outside [M, N] was written: bit for bit the prefill (sentinel, or NaN for the automatic split) -------------------------
    outside = torch.ones(out.numel(), dtype=torch.bool)
    outside[p.valid] = False
    touched = (out.view(torch.int32) != p.c_host0.view(torch.int32)) & outside
    assert not bool(touched.any()), (c.name, "wrote outside C[M, N] at flat offsets", touched.nonzero().reshape(-1)[:8].tolist())
    # ---- values ---------------------------------------------------------------------------------------------------------------------
    prec = got_v[4]
    ref, mag = p.reference(prec)
    bound = G.bound_for(p.K)
    got = out[p.valid].double()
    if c.epi == "bias_relu":
        ref = torch.clamp(ref, min=0)
    err = (got - ref).abs()
    ok = err <= bound * mag          # (NaN compares false)
    worst = float((err / mag.clamp_min(1e-300))[mag > 0].max()) if bool((mag > 0).any()) else 0.0
    print(f"{c.name}: instance {got_v[:5]} max error {worst:.3e} (bound {bound:.3e})")
    assert bool(ok.all()), (c.name, "error", worst, "bound", bound, "first bad", (~ok).nonzero().reshape(-1)[:8].tolist(),
                            got[~ok][:4].tolist(), ref[~ok][:4].tolist())
    if c.conv is not None and c.pair == "CW" and c.conv[5:8] == (1, 2, 0) and not c.accumulate:
        unread = p.dgrad_unread()
        assert bool(unread.any()) and bool((out[p.valid][unread] == 0).all()), (c.name, "dx pixels no output pixel reads must be exact zeros")
    if c.epi == "gelu":
        # C2 = gelu_erf(C) of the very value stored to C.  The evaluation in fp32: erf to ~1 ulp of 1 (2^-24 relative to 1 + erf <= 2), the
        # product 0.5 x (1 + erf) with two more roundings -- an absolute error <= 0.5 |x| 2^-23 + 2 * 2^-24 |x| < 2^-22 |x|
        out2 = p.c2_buf.cpu()
        touched2 = (out2.view(torch.int32) != p.c_host0.view(torch.int32)) & outside
        assert not bool(touched2.any()), (c.name, "wrote outside C2[M, N]")
        want2 = _gelu(got)
        e2 = (out2[p.valid].double() - want2).abs()
        assert bool((e2 <= 2.0 ** -22 * got.abs() + 1e-30).all()), (c.name, "C2 != gelu(C)", float(e2.max()))
    if c.stats:
        # sums and sums of squares of the STORED values over the M rows of the problem (tail rows of the last tile not counted): a thread
        # adds at most 16 rows in fp32 (128 x 128 tile: 128 * 32 float4 / 256 threads) before the fp64 reduction -- 16 roundings, one more
        # for the square: 18 * 2^-24 of the sum of magnitudes
        st = p.stats.cpu().view(-1, 2, p.N).sum(0)
        v = got.view(p.M, p.N)
        tol = 18 * 2.0 ** -24
        assert bool(((st[0] - v.sum(0)).abs() <= tol * v.abs().sum(0)).all()), (c.name, "column sums", float((st[0] - v.sum(0)).abs().max()))
        assert bool(((st[1] - (v * v).sum(0)).abs() <= tol * (v * v).sum(0)).all()), (c.name, "column sums of squares")
    return worst


def _ids(cases):
    return [c.name for c in cases]


@pytest.mark.parametrize("case", G.BY_PAIR["KK"], ids=_ids(G.BY_PAIR["KK"]))
def test_dense_forward(ops, case):
    run_case(case, ops)


@pytest.mark.parametrize("case", G.BY_PAIR["KR"], ids=_ids(G.BY_PAIR["KR"]))
def test_dense_dgrad(ops, case):
    run_case(case, ops)


@pytest.mark.parametrize("case", G.BY_PAIR["RR"], ids=_ids(G.BY_PAIR["RR"]))
def test_dense_wgrad(ops, case):
    run_case(case, ops)


@pytest.mark.parametrize("case", G.BY_PAIR["CK"], ids=_ids(G.BY_PAIR["CK"]))
def test_conv_forward(ops, case):
    run_case(case, ops)


@pytest.mark.parametrize("case", G.BY_PAIR["CW"], ids=_ids(G.BY_PAIR["CW"]))
def test_conv_dgrad(ops, case):
    run_case(case, ops)


@pytest.mark.parametrize("case", G.BY_PAIR["RC"], ids=_ids(G.BY_PAIR["RC"]))
def test_conv_wgrad(ops, case):
    run_case(case, ops)
