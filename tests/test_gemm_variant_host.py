"""vbg_gemm_variant (include/vbg.h) without a GPU: the host-only query of the dispatch decision vbg_gemm itself launches from.

Every case of tests/gemm_cases.py must reach the kernel instance it names; the instances the table reaches, per operand-kind pair, must
be the whole instantiation list of launch_pair (csrc/gemm.hip), written out in gemm_cases.INSTANCES and compared with the source here;
what no descriptor can reach is named with its reason (gemm_cases.UNREACHABLE)."""
import os
import re

import pytest
import torch

import gemm_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    from vbg import ops as _ops
    return _ops


def test_kind_constants_are_the_headers():
    from vbg import lib as L
    assert (G.DENSE_K, G.DENSE_R, G.CONV_K, G.CONV_R, G.WT_R) == (L.OP_DENSE_K, L.OP_DENSE_R, L.OP_CONV_K, L.OP_CONV_R, L.OP_WT_R)
    assert (G.EPI_NONE, G.EPI_RELU, G.EPI_GELU_DUAL) == (L.EPI_NONE, L.EPI_RELU, L.EPI_GELU_DUAL)


def test_written_instance_list_is_the_sources():
    """launch_pair's switch: one VBG_GEMM_CASE(BM, BN, BK, VEC, PREC) per instance of every pair, plus the fp16-pair case that exists for the
    two forward pairs only -- the list gemm_cases.INSTANCES writes out"""
    src = open(os.path.join(ROOT, "vibertgrid-pytorch_amd", "csrc", "gemm.hip")).read()
    body = src[src.index("static int launch_pair("):src.index("#undef VBG_GEMM_CASE")]
    every = [tuple(int(x) for x in m) for m in re.findall(r"^\s*VBG_GEMM_CASE\((\d+), (\d+), (\d+), (\d+), (\d+)\)", body, flags=re.M)]
    fwd_only = [tuple(int(x) for x in m) for m in re.findall(r"case variant_key\((\d+), (\d+), (\d+), (\d+), (\d+)\):\s*\n\s*if constexpr \(\(AK == VBG_OP_DENSE_K \|\| "
                                                              r"AK == VBG_OP_CONV_K\) && BKD == VBG_OP_DENSE_K\)", body)]
    assert len(every) == 12 and len(set(every)) == 12 and fwd_only == [G.F16_TILE]
    assert len(re.findall(r"launch_one<", body)) == 2          # the macro's and the fp16-pair's: no instance outside the two lists
    for pair, inst in G.INSTANCES.items():
        assert sorted(inst) == sorted(every + (fwd_only if pair in ("KK", "CK") else [])), pair
    assert sum(len(v) for v in G.INSTANCES.values()) == 74


def test_table_reaches_every_instance():
    reached = {(c.pair, c.expect[:5]) for c in G.CASES}
    every = {(p, v) for p, inst in G.INSTANCES.items() for v in inst}
    assert set(G.UNREACHABLE) <= every
    assert reached == every - set(G.UNREACHABLE), (sorted(every - set(G.UNREACHABLE) - reached), sorted(reached - every))


@pytest.mark.parametrize("pair", list(G.PAIRS))
def test_every_case_runs_the_instance_it_names(ops, pair):
    bad = []
    for c in G.BY_PAIR[pair]:
        p = G.Problem(c, torch.device("cpu"), ops)
        with G.form_state(ops, p.form):
            got = tuple(ops.gemm_variant(*p.args, **p.kw))
        if got != c.expect:
            bad.append((c.name, c.expect, got))
    assert not bad, bad[:20]


def test_unreachable_instance_is_unreachable(ops):
    """CONV_K x WT_R never takes the scalar-load path: a misaligned filter or a row length off 4 is an argument error, and an aligned
    one runs vector loads whatever a_vec / b_vec the caller computed (here: dy one float off is an argument error too)"""
    from vbg.lib import VbgError
    c = next(c for c in G.CASES if c.pair == "CW")
    p = G.Problem(c, torch.device("cpu"), ops)
    with G.form_state(ops, p.form):
        assert ops.gemm_variant(*p.args, **p.kw).vec == 1
        for off in ({"a_ptr_off": 1}, {"b_ptr_off": 1}):
            with pytest.raises(VbgError):
                ops.gemm_variant(*p.args, **{**p.kw, **off})
        a = list(p.args)
        a[7] = 21          # ldb = 21: gemm_raw computes b_vec = 0 from it, the dispatch sets it back to 1
        assert ops.gemm_variant(*a, **p.kw).vec == 1


def test_query_is_host_only_and_dereferences_nothing(ops):
    """operand, output, bias, group-table and statistics pointers that point nowhere: the query answers from the numbers alone"""
    import ctypes as C
    from vbg import lib as L
    d = L.GemmDesc()
    d.M, d.N, d.K, d.lda, d.ldb, d.ldc = 130, 132, 1536, 1536, 1536, 132
    d.A, d.B, d.C, d.bias = 0x1000, 0x2000, 0x3000, 0x10
    d.a_vec = d.b_vec = 1
    d.a_kind, d.b_kind, d.alpha, d.splitk, d.bf16 = G.DENSE_K, G.DENSE_K, 1.0, 0, 3
    out = (C.c_int * 8)()
    assert L.lib.vbg_gemm_variant(C.byref(d), C.byref(out)) == 0
    assert tuple(out) == (64, 64, 32, 1, 3, 4, 0, 1)          # 3 x 3 tiles, 48 k-tiles: the automatic split takes 4, nothing was zeroed
    d.grp, d.ngroups, d.grp_maxM, d.grp_maxN, d.splitk = 0x4000, 3, 64, 64, 1
    assert L.lib.vbg_gemm_variant(C.byref(d), C.byref(out)) == 0 and tuple(out)[:5] == (64, 64, 32, 1, 3)
    assert L.lib.vbg_gemm_variant(None, C.byref(out)) == -1 and L.lib.vbg_gemm_variant(C.byref(d), None) == -1
    d.M = 0
    d.grp = None
    assert L.lib.vbg_gemm_variant(C.byref(d), C.byref(out)) == 0 and tuple(out) == (0,) * 8          # empty problem: no launch


def test_argument_errors_of_the_query(ops):
    """the codes of vbg_gemm: a split without accumulate, slab_stride with K < 64 splitk^2, statistics with N % 4 != 0, Cs % 16 != 0,
    CONV_R with N != kh kw Cs"""
    from vbg.lib import VbgError
    cpu = torch.device("cpu")

    def problem(name):
        return G.Problem(next(c for c in G.CASES if c.name == name), cpu, ops)

    def rejected(p, args=None, **over):
        with G.form_state(ops, p.form):
            assert tuple(ops.gemm_variant(*p.args, **p.kw))[0] > 0          # the case itself is fine
            with pytest.raises(VbgError) as e:
                ops.gemm_variant(*(args or p.args), **{**p.kw, **over})
            assert "argument error" in str(e.value)          # (a negative code: vbg.lib.check)

    p = problem("KK-64x64x32-v1p2-K200")
    rejected(p, splitk=3)                                                   # a split without accumulate
    p = problem("KK-slab2-p2-64")
    a = list(p.args)
    a[2] = 255                                                              # K = 255 < 64 * 2^2
    rejected(p, args=a)
    p3 = problem("KK-slab3-p2-64")
    a = list(p3.args)
    a[2] = 575                                                              # K = 575 < 64 * 3^2
    rejected(p3, args=a)
    p = problem("KK-stats-64x64x32-p2")
    a = list(p.args)
    a[1] = p.N - 1                                                          # statistics with N % 4 != 0
    rejected(p, args=a)
    p = problem("CK-64x64x16-v1p0-k3s1-c16")
    g = p.kw["geo"]
    rejected(p, geo=ops.conv_geo(g.Hs, g.Ws, 24, g.Hr, g.Wr, g.kh, g.kw, g.stride, g.pad, 0))          # Cs % 16 != 0
    p = problem("RC-64x64x32-v1p0-7x9")
    a = list(p.args)
    a[1] = p.N - 32                                                         # CONV_R: N != kh kw Cs
    rejected(p, args=a)
