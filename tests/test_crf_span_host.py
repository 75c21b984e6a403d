"""The restatement the GPU tests of vbg_crf_path_logp / vbg_field_runs lean on (tests/crf_span_restate.py), checked without a GPU:
against brute-force enumeration of every path (spans, whole paths, a path that is not the best one), against the winners of
tests/crf_posterior_restate.py, and the new entries' argument checks, which run before any launch."""
import numpy as np
import pytest

import crf_posterior_restate as R
import crf_span_restate as S


def tiny(T, n, seed):
    rng = np.random.default_rng(seed)
    start, stop = T - 2, T - 1
    em = rng.standard_normal((n, T))
    trans = 2 * rng.standard_normal((T, T))
    trans[start, :] = -10000
    trans[:, stop] = -10000
    return em, trans, start, stop, rng


@pytest.mark.parametrize("T,n", [(3, 1), (3, 6), (4, 2), (4, 5), (5, 3), (5, 5)])
def test_spans_and_whole_paths_against_brute_force(T, n):
    em, trans, start, stop, rng = tiny(T, n, 70 + 10 * T + n)
    logz, _, best, _ = R.brute_force(em, trans, start, stop)
    other = [int(v) for v in rng.integers(0, T - 2, n)]
    if other == best:                                    # (three tags leave one ordinary tag: there the best path is the only one)
        other[0] = (other[0] + 1) % (T - 2)
    assert T == 3 or other != best
    for y in (best, other):
        lm, lc = S.path_logp(em, trans, start, stop, y)
        assert lc[0] == lm[0]
        worst = 0.0
        for s in range(n):
            for e in range(s, n):
                err = abs(S.span_logp(lm, lc, s, e) - S.brute_span(em, trans, start, stop, y, s, e))
                worst = max(worst, err)
                assert err <= 1e-12, (y, s, e, err)
        whole = abs(float(np.sum(lc)) - (R.path_score(em, trans, start, stop, y) - logz))
        print(f"T {T} n {n} path {y}: worst span error {worst:.2e}, |sum(lc) - (score - logz)| {whole:.2e}")
        assert whole <= 1e-12


def test_marginals_are_the_posteriors():
    em, trans, start, stop, _ = tiny(5, 4, 3)
    _, marg = R.forward_backward(em, trans, start, stop)
    y = [0, 2, 1, 2]
    lm, _ = S.path_logp(em, trans, start, stop, y)
    assert np.allclose(np.exp(lm), marg[np.arange(4), y], rtol=1e-12, atol=0)


def test_out_of_range_tags_and_the_empty_document():
    em, trans, start, stop, _ = tiny(4, 5, 9)
    lm, lc = S.path_logp(em, trans, start, stop, [0, -1, 1, 4, 0])
    assert np.isinf(lm[[1, 3]]).all() and np.isfinite(lm[[0, 2, 4]]).all()
    assert np.isinf(lc[[1, 2, 3, 4]]).all() and lc[0] == lm[0]
    ok_lm, _ = S.path_logp(em, trans, start, stop, [0, 0, 1, 1, 0])
    assert lm[0] == ok_lm[0] and lm[2] == ok_lm[2] and lm[4] == ok_lm[4]                 # a marginal does not see the other rows' tags
    lm, lc = S.path_logp(np.zeros((0, 4)), trans, start, stop, [])
    assert lm.shape == lc.shape == (0,)


# tags: 0 "O", 1 "B-a", 2 "I-a", 3 "B-b" (classes 0, 1, 1, 2), as in test_crf_posterior_host.py
TC, TB = [0, 1, 1, 2], [0, 1, 0, 0]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_best_of_the_list_is_the_winner_table(seed):
    rng = np.random.default_rng(seed)
    n = 60
    path = []
    while len(path) < n:
        path += [int(rng.integers(0, 4))] * int(rng.integers(1, 5))
    path = path[:n]
    m = rng.random((n, 4)).astype(np.float32)
    m[5:9] = 0                                                                           # runs whose scores are all 0
    m /= np.maximum(m.sum(1, keepdims=True), 1e-30)
    for thresh in (None, 0.5):
        cls, score, win = R.decode_tags(m, path, TC, TB, 3, thresh)
        begin_rows = [bool(TB[t]) for t in path]
        lm = np.log(np.maximum(m[np.arange(n), path].astype(np.float64), 1e-300))
        runs = S.list_runs(cls, score, begin_rows, lm, lm, True)
        assert sum(r[1] for r in runs) == n and [r[0] for r in runs] == sorted(r[0] for r in runs)
        assert all(cls[r[0]] == r[2] for r in runs)
        assert S.best_of(runs, 3) == win


def test_list_runs_on_known_cases():
    # B-a I-a | B-a I-a I-a, then O: three runs, the begin tag splits the class
    path = [1, 2, 1, 2, 2, 0]
    score = [np.float32(v) for v in (0.5, 0.5, 0.75, 0.75, 0.75, 1.0)]
    lm = np.log([0.5, 0.5, 0.75, 0.75, 0.75, 1.0])
    lc = np.log([0.5, 0.25, 0.5, 0.5, 0.5, 0.125])
    runs = S.list_runs([1, 1, 1, 1, 1, 0], score, [True, False, True, False, False, False], lm, lc, True)
    assert [(r[0], r[1], r[2], r[3]) for r in runs] == [(0, 2, 1, 0.5), (2, 3, 1, 0.75), (5, 1, 0, 1.0)]
    assert np.allclose([r[4] for r in runs], np.log([0.5 * 0.25, 0.75 * 0.5 * 0.5, 1.0]), rtol=1e-15)
    # the score form: runs of equal class only, every run under its own class (the last one too), logp 0
    runs = S.list_runs([2, 2, 1], [0.5, 0.25, 0.75], None, None, None, False)
    assert runs == [(0, 2, 2, 0.375, 0.0), (2, 1, 1, 0.75, 0.0)]
    assert S.list_runs([], [], [], [], [], True) == []


def test_new_entries_reject_their_argument_errors_without_a_gpu():
    import ctypes as C
    from vbg import lib as L
    ints = lambda *v: (C.c_int * len(v))(*v)                                           # noqa: E731
    one = C.c_void_p(64)                                                               # a non-NULL pointer that is never followed
    f = L.lib.vbg_crf_path_logp
    assert f(None, one, 0, one, 7, 5, 6, None, None, None, None, None) == 0            # no document: a no-op
    assert f(one, None, 1, one, 7, 5, 6, one, one, one, one, None) == -1               # NULL doc_off
    assert f(one, one, 1, None, 7, 5, 6, one, one, one, one, None) == -1               # NULL trans
    assert f(one, one, 1, one, 0, 0, 0, one, one, one, one, None) == -1                # no tag
    assert f(one, one, 1, one, 65, 63, 64, one, one, one, one, None) == -1             # more than 64 tags
    assert f(one, one, -1, one, 7, 5, 6, one, one, one, one, None) == -1               # ndoc < 0
    for s, e in ((-1, 6), (7, 6), (5, -1), (5, 7)):
        assert f(one, one, 1, one, 7, s, e, one, one, one, one, None) == -1            # START / STOP out of range
    for k in range(4):                                                                 # NULL path / ws / lm / lc with documents
        args = [one, one, one, one]
        args[k] = None
        assert f(one, one, 1, one, 7, 5, 6, *args, None) == -1
    assert f(None, one, 1, one, 7, 5, 6, one, one, one, one, None) == -1               # NULL emissions

    g = L.lib.vbg_field_runs
    assert g(None, ints(0, 0), 0, 5, 0, 0.0, None, None, None, None) == 0              # no document: a no-op
    assert g(None, ints(0, 0, 0), 2, 5, 0, 0.0, None, None, None, None) == 0           # empty documents only: no row, no buffer
    assert g(None, None, 0, 5, 0, 0.0, None, None, None, None) == -1                   # NULL row ranges
    assert g(None, ints(0, 0), -1, 5, 0, 0.0, None, None, None, None) == -1
    assert g(None, ints(0, 0), 1, 0, 0, 0.0, None, None, None, None) == -1             # C outside [1, 64]
    assert g(None, ints(0, 0), 1, 65, 0, 0.0, None, None, None, None) == -1
    assert g(None, ints(0, 1 << 20), 1, 5, 0, 0.0, None, None, None, None) == -1       # 2^20 rows
    assert g(None, ints(3, 2), 1, 5, 0, 0.0, None, None, None, None) == -1             # decreasing row ranges
    assert g(None, ints(-1, 2), 1, 5, 0, 0.0, None, None, None, None) == -1
    assert g(one, ints(0, 5), 1, 5, 0, 0.0, one, one, None, None) == -1                # rows without a record array
    assert g(None, ints(0, 5), 1, 5, 0, 0.0, one, one, one, None) == -1

    h = L.lib.vbg_field_runs_tags
    ok_cls, ok_beg = ints(0, 1, 1, 2), ints(0, 1, 0, 0)
    assert h(None, None, None, None, ints(0, 0), 0, 4, 3, ok_cls, ok_beg, 0, 0.0, None, None, None, None) == 0
    assert h(None, None, None, None, ints(0, 0), 1, 4, 3, ints(0, 1, 3, 2), ok_beg, 0, 0.0, None, None, None, None) == -1   # class out of range
    assert h(None, None, None, None, ints(0, 0), 1, 4, 3, ok_cls, ints(0, 2, 0, 0), 0, 0.0, None, None, None, None) == -1   # a begin flag of 2
    assert h(None, None, None, None, ints(0, 0), 1, 65, 3, ints(*([0] * 65)), ints(*([0] * 65)), 0, 0.0, None, None, None, None) == -1
    assert h(None, None, None, None, ints(0, 0), 1, 4, 65, ok_cls, ok_beg, 0, 0.0, None, None, None, None) == -1
    assert h(None, None, None, None, ints(0, 0), 1, 4, 3, None, ok_beg, 0, 0.0, None, None, None, None) == -1               # NULL tables
    assert h(None, None, None, None, ints(0, 1 << 20), 1, 4, 3, ok_cls, ok_beg, 0, 0.0, None, None, None, None) == -1
    for k in range(4):                                                                 # rows without marginals / path / lm / lc
        args = [one, one, one, one]
        args[k] = None
        assert h(*args, ints(0, 5), 1, 4, 3, ok_cls, ok_beg, 0, 0.0, one, one, one, None) == -1
