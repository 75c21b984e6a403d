"""vbg_sample_select (csrc/sample.hip) against its numpy statement (tests/sample_restate.py): the lists -- order included --, the
keeps and the category sizes are EQUAL, for every input.  Needs a real MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

import sample_restate as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from vbg import ops as _ops
    return _ops


def dev():
    return torch.device("cuda")


def run(ops, labels, cats, seed, stream0=S.STREAM0):
    """-> (lists, keep, n) as python lists, from one ops.sample_select call (cats: [(value, eq, k)], taken in key order)"""
    lab = torch.as_tensor(np.asarray(labels, np.int32)).to(dev())
    idx, keep, n = ops.sample_select(lab, [(v, eq, k, 1) for v, eq, k in cats], seed, stream0)
    idx, keep, n = idx.cpu().numpy(), keep.cpu().tolist(), n.cpu().tolist()
    lists, o = [], 0
    for (_, _, k), kp in zip(cats, keep):
        lists.append(idx[o:o + kp].tolist())
        o += k
    return lists, keep, n


def check(ops, labels, cats, seed, stream0=S.STREAM0):
    got = run(ops, labels, cats, seed, stream0)
    wl, wk, wn = S.sample_select(labels, cats, seed, stream0)
    assert got[1] == wk and got[2] == wn, (got[1], wk, got[2], wn)
    for c, (a, b) in enumerate(zip(got[0], wl)):
        assert a == b.tolist(), (c, a[:8], b[:8].tolist())
    return got


@pytest.mark.parametrize("N", [1, 255, 256, 257, 100_003])
@pytest.mark.parametrize("k", [1, 32, 512, 4096])
def test_sizes_and_ks(ops, N, k):
    """three classes and a foreign value; category 0 = class 1, category 1 = everything but class 0"""
    rng = np.random.default_rng(N + k)
    labels = rng.integers(0, 3, N).astype(np.int32)
    labels[rng.integers(0, N, max(N // 50, 1))] = 77
    check(ops, labels, [(1, 1, k), (0, 0, k)], seed=S.step_seed(N, 1234))


def test_past_one_grid_sweep(ops):
    """600 001 elements: the sweeps launch one block of 512 threads per 8192 elements (at most 256) and loop with the grid's stride, so
    every thread makes 16 trips here with a ragged last one"""
    labels = (np.arange(600_001) % 5).astype(np.int32)
    check(ops, labels, [(3, 1, 512), (0, 0, 4096), (9, 1, 32)], seed=0xABCDEF0123)


@pytest.mark.parametrize("k", [1, 32, 512, 4096])
@pytest.mark.parametrize("delta", ["empty", -1, 0, 1])
def test_category_sizes_around_k(ops, k, delta):
    nc = 0 if delta == "empty" else k + delta
    N = 9001
    rng = np.random.default_rng(7 * k + nc)
    labels = np.zeros(N, np.int32)
    labels[rng.choice(N, nc, replace=False)] = 4
    lists, keep, n = check(ops, labels, [(4, 1, k)], seed=k)
    assert n == [nc] and keep == [min(k, nc)]
    if 1 < nc <= k:
        assert lists[0] == sorted(lists[0])          # everything kept: ascending element index


def test_four_categories_eq0_and_foreign_values(ops):
    N = 70_001
    rng = np.random.default_rng(3)
    labels = rng.integers(-2, 6, N).astype(np.int32)          # -2, -1, 4, 5 belong to no `==` category below
    cats = [(0, 1, 16), (1, 1, 4096), (2, 0, 333), (3, 1, 1)]
    lists, keep, n = check(ops, labels, cats, seed=S.step_seed(5, 42, rank=2))
    for (v, eq, _), l in zip(cats, lists):
        assert all((labels[i] == v) == bool(eq) for i in l)


def test_one_bin_holds_more_than_the_selection(ops):
    """4 200 000 elements, all in the category, k = 512: the 512th key lies in the first of the 2048 leading-digit bins, which holds
    about 2051 elements -- four times the selection -- so the finishing workgroup has to narrow the key over further digits instead of
    sorting what it was handed.  The count is asserted from the statement's keys."""
    N, k, seed = 4_200_000, 512, 2024
    labels = np.ones(N, np.int32)
    key = S.keys_of(seed, S.STREAM0, np.arange(N))
    kth = np.partition(key, k - 1)[k - 1]
    in_bin = int(((key >> np.uint64(53)) == (kth >> np.uint64(53))).sum())
    print("elements sharing the k-th key's leading digit:", in_bin)
    assert in_bin > 3 * k
    got = run(ops, labels, [(1, 1, k)], seed)
    want = np.argsort(key, kind="stable")[:k]
    assert got[1] == [k] and got[2] == [N] and got[0][0] == want.tolist()


def test_repeatable_and_independent_of_the_stream(ops):
    N = 300_007
    labels = (np.random.default_rng(8).integers(0, 4, N)).astype(np.int32)
    cats = [(1, 1, 512), (0, 0, 4096)]
    a = run(ops, labels, cats, seed=99)
    b = run(ops, labels, cats, seed=99)
    assert a == b
    s = torch.cuda.Stream()
    x = torch.randn(1024, 1024, device=dev())
    with torch.cuda.stream(s):
        for _ in range(3):
            x = x @ x * 1e-3          # unrelated launches in front
        c = run(ops, labels, cats, seed=99)
    s.synchronize()
    assert a == c
    assert run(ops, labels, cats, seed=100) != a


def test_argument_errors_before_any_launch(ops):
    from vbg import lib as L
    lab = torch.zeros(64, dtype=torch.int32, device=dev())
    with pytest.raises(Exception):
        ops.sample_select(lab, [(0, 1, 4, 0)] * 5, 1)                                  # more than 4 categories
    for k in (0, -3, 4097):
        with pytest.raises(L.VbgError):
            ops.sample_select(lab, [(0, 1, k, 0)], 1)
    sc = L.SampleCats()
    sc.c[0].value, sc.c[0].eq, sc.c[0].k = 0, 1, 4
    out = torch.zeros(16, dtype=torch.int32, device=dev())
    ws = torch.zeros(int(L.lib.vbg_sample_ws_bytes(64, 1, 4)), dtype=torch.uint8, device=dev())
    P = lambda t: C.c_void_p(t.data_ptr())
    f = L.lib.vbg_sample_select
    assert f(P(lab), 64, 1, sc, 1, 0, P(out), P(out[8:]), P(out[12:]), P(ws), ws.numel(), None) == 0
    assert f(P(lab), 64, 1, sc, 1, 0, P(out), P(out[8:]), P(out[12:]), P(ws), ws.numel() - 1, None) == -1          # workspace too small
    assert f(P(lab), 2 ** 31, 1, sc, 1, 0, P(out), P(out[8:]), P(out[12:]), P(ws), 2 ** 40, None) == -1              # N >= 2^31
    assert f(P(lab), 64, 5, sc, 1, 0, P(out), P(out[8:]), P(out[12:]), P(ws), ws.numel(), None) == -1
    assert f(P(lab), 64, 0, sc, 1, 0, P(out), P(out[8:]), P(out[12:]), P(ws), ws.numel(), None) == -1
    assert L.lib.vbg_sample_ws_bytes(10, 5, 4) < 0
    torch.cuda.synchronize()
