"""The restatement the GPU tests of vbg_crf_posterior / vbg_field_decode_tags lean on (tests/crf_posterior_restate.py), checked
without a GPU: against the reference CRF's own numbers (tests/golden/crf_posterior.npz: log Z, d log Z / d emissions and the
Viterbi path of the real model/crf.py in double), against brute-force enumeration, and on hand-built decode cases whose answers are
known.  vbg.decode.tag_table is host code and is checked here too."""
import os

import numpy as np
import pytest

import crf_posterior_restate as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "crf_posterior.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN, allow_pickle=False)


def test_fixture_cases(golden):
    assert [str(n) for n in golden["names"]] == ["t9_n15", "t27_n300", "t27_n700"]
    for name, shape in zip(golden["names"], [(15, 9), (300, 27), (700, 27)]):
        assert golden[f"em_{name}"].shape == shape and golden[f"marg_{name}"].dtype == np.float64


@pytest.mark.parametrize("name", ["t9_n15", "t27_n300", "t27_n700"])
def test_restatement_against_the_reference(golden, name):
    em, trans = golden[f"em_{name}"], golden[f"trans_{name}"]
    start, stop = (int(v) for v in golden[f"ends_{name}"])
    logz, marg = R.forward_backward(em, trans, start, stop)
    want = golden[f"marg_{name}"]
    rel = np.abs(marg - want) / np.maximum(np.abs(want), 1e-300)
    rel[want == 0] = np.abs(marg[want == 0])
    print(name, "max relative error of the marginals", float(rel.max()), "of log Z", abs(logz - float(golden[f"logz_{name}"])) / abs(logz))
    assert float(rel.max()) <= 1e-10
    assert abs(logz - float(golden[f"logz_{name}"])) <= 1e-10 * abs(float(golden[f"logz_{name}"]))
    assert bool((marg[:, [start, stop]] == 0).all())
    path, score = R.viterbi(em, trans, start, stop)
    assert path == golden[f"path_{name}"].tolist()
    assert abs(score - float(golden[f"score_{name}"])) <= 1e-10 * abs(score)


@pytest.mark.parametrize("rows", [1, 2, 3, 4, 5])
def test_restatement_against_brute_force(rows):
    T, start, stop = 4, 2, 3
    rng = np.random.default_rng(40 + rows)
    em = rng.standard_normal((rows, T))
    trans = 2 * rng.standard_normal((T, T))
    trans[start, :] = -10000
    trans[:, stop] = -10000
    logz, marg = R.forward_backward(em, trans, start, stop)
    bz, bm, bpath, bscore = R.brute_force(em, trans, start, stop)
    assert abs(logz - bz) <= 1e-12 * max(1.0, abs(bz))
    assert np.allclose(marg, bm, rtol=1e-10, atol=1e-300)
    path, score = R.viterbi(em, trans, start, stop)
    assert path == bpath and abs(score - bscore) <= 1e-12 * max(1.0, abs(bscore))


def test_empty_document():
    trans = np.array([[0.5, 1.0, -10000.0], [-10000.0] * 3, [0.25, 2.0, -10000.0]])
    logz, marg = R.forward_backward(np.zeros((0, 3)), trans, 1, 2)
    assert logz == 2.0 and marg.shape == (0, 3)


# ---- tag_table
PLAIN = {"O": 0, "B-company": 1, "B-date": 2, "B-address": 3, "B-total": 4}
BIO = {"O": 0, "B-company": 1, "I-company": 2, "B-date": 3, "I-date": 4, "B-total": 5}
CATS = ["others", "company", "date", "address", "total"]


def with_ends(d):
    d = dict(d)
    d["<START>"], d["<STOP>"] = len(d), len(d) + 1
    return d


def test_tag_table_plain_and_bio():
    from vbg import decode as D
    t = D.tag_table(with_ends(PLAIN), CATS)
    assert t.tag_class == [0, 1, 2, 3, 4, 0, 0] and t.tag_begin == [0] * 7          # every segment of a field is "B-x": no begin tags
    t = D.tag_table(with_ends(BIO), CATS)
    assert t.tag_class == [0, 1, 1, 2, 2, 4, 0, 0]
    assert t.tag_begin == [0, 1, 0, 1, 0, 0, 0, 0]                                   # B-total has no I-total: not a begin tag
    for d in (with_ends(PLAIN), with_ends(BIO), PLAIN):
        got = D.tag_table(d, CATS)
        assert (got.tag_class, got.tag_begin) == R.tag_table(d, CATS)


def test_tag_table_errors():
    from vbg import decode as D
    for bad in ({"O": 0, "B-vendor": 1}, {"O": 0, "company": 1}, {"O": 0, "E-company": 1}, {"O": 0, "B-date": 2}, {"O": 0, "B-date": 0}):
        with pytest.raises(ValueError):
            D.tag_table(bad, CATS)
        with pytest.raises(ValueError):
            R.tag_table(bad, CATS)


def test_entry_argument_errors_do_not_need_a_gpu():
    import ctypes as C
    from vbg import lib as L
    ints = lambda *v: (C.c_int * len(v))(*v)                                           # noqa: E731
    f = L.lib.vbg_field_decode_tags
    ok_cls, ok_beg = ints(0, 1, 1, 2), ints(0, 1, 0, 0)
    assert f(None, None, ints(0, 0), 0, 4, 3, ok_cls, ok_beg, 0, 0.0, None, None, None, None) == 0          # no document: a no-op
    assert f(None, None, ints(0, 0), 1, 4, 3, ints(0, 1, 3, 2), ok_beg, 0, 0.0, None, None, None, None) == -1  # class out of range
    assert f(None, None, ints(0, 0), 1, 4, 3, ok_cls, ints(0, 2, 0, 0), 0, 0.0, None, None, None, None) == -1  # a begin flag of 2
    assert f(None, None, ints(0, 0), 1, 65, 3, ints(*([0] * 65)), ints(*([0] * 65)), 0, 0.0, None, None, None, None) == -1
    assert f(None, None, ints(0, 0), 1, 4, 65, ok_cls, ok_beg, 0, 0.0, None, None, None, None) == -1
    assert f(None, None, ints(0, 1 << 20), 1, 4, 3, ok_cls, ok_beg, 0, 0.0, None, None, None, None) == -1   # 2^20 rows
    assert f(None, None, ints(0, 5), 1, 4, 3, ok_cls, ok_beg, 0, 0.0, None, None, None, None) == -1         # rows without buffers
    g = L.lib.vbg_crf_posterior
    assert g(None, None, 1, None, 7, 5, 6, None, None, None, None, None, None) == -1


# ---- the decode over tags, on cases whose answers are known.  Tags: 0 "O", 1 "B-a", 2 "I-a", 3 "B-b" (classes 0, 1, 1, 2)
TC, TB = [0, 1, 1, 2], [0, 1, 0, 0]


def rows_for(path, conf):
    """marginals whose row r gives `conf[r]` to the tag path[r] and the rest to a tag of another class"""
    m = np.zeros((len(path), 4), dtype=np.float32)
    for r, (t, c) in enumerate(zip(path, conf)):
        m[r, t] = c
        m[r, 3 if TC[t] != 2 else 0] = np.float32(1.0) - np.float32(c)
    return m


def test_decode_begin_tag_splits_a_run():
    path = [1, 2, 1, 2, 2]                                   # B-a I-a | B-a I-a I-a: one class, two runs
    conf = [0.5, 0.5, 0.75, 0.75, 0.75]
    cls, score, win = R.decode_tags(rows_for(path, conf), path, TC, TB, 3)
    assert cls == [1] * 5 and [float(s) for s in score] == conf
    assert win == [None, (2, 3, 0.75), None]
    assert R.runs(cls, [True, False, True, False, False]) == [(0, 2), (2, 3)]
    # without the begin flag the five rows are one run
    assert R.decode_tags(rows_for(path, conf), path, TC, [0] * 4, 3)[2][1] == (0, 5, 0.65)


def test_decode_class_posterior_adds_the_tags_of_the_class():
    m = np.array([[0.125, 0.5, 0.25, 0.125]], dtype=np.float32)
    cls, score, win = R.decode_tags(m, [2], TC, TB, 3)
    assert cls == [1] and float(score[0]) == 0.75 and win == [None, (0, 1, 0.75), None]


def test_decode_threshold_zeroes_a_class():
    path = [3, 3, 1]
    conf = [0.5, 0.25, 0.75]
    m = rows_for(path, conf)
    assert R.decode_tags(m, path, TC, TB, 3)[2] == [None, (2, 1, 0.75), (0, 2, 0.375)]
    cls, score, win = R.decode_tags(m, path, TC, TB, 3, thresh=0.5)
    assert cls == [2, 0, 1] and [float(s) for s in score] == conf                   # the score stays
    assert win == [(1, 1, 0.25), (2, 1, 0.75), (0, 1, 0.5)]
    assert R.decode_tags(m, path, TC, TB, 3, thresh=0.500001)[0] == [0, 0, 1]


def test_decode_tie_takes_the_earlier_run():
    path = [3, 0, 3, 0, 3]
    conf = [0.5, 1.0, 0.5, 1.0, 0.25]
    win = R.decode_tags(rows_for(path, conf), path, TC, TB, 3)[2]
    assert win[2] == (0, 1, 0.5) and win[0] == (1, 1, 1.0)


def test_decode_single_row_and_zero_sum():
    assert R.decode_tags(rows_for([3], [0.5]), [3], TC, TB, 3)[2] == [None, None, (0, 1, 0.5)]     # under its OWN class
    m = np.zeros((2, 4), dtype=np.float32)
    m[:, 0] = 1.0
    assert R.decode_tags(m, [3, 0], TC, TB, 3)[2] == [(1, 1, 1.0), None, None]        # the run of class 2 sums to 0: no record
    assert R.decode_tags(np.zeros((0, 4), dtype=np.float32), [], TC, TB, 3)[2] == [None, None, None]


def test_decode_means_do_not_depend_on_grouping():
    rng = np.random.default_rng(5)
    score = rng.random(1000).astype(np.float32)
    q = [int(np.rint(float(v) * R.FIX)) for v in score]
    assert sum(q) == sum(q[::-1]) == sum(q[:333]) + sum(q[333:])
    win = R.winners([1] * 1000, list(score), [False] * 1000, 2)
    assert win[1] == (0, 1000, float(sum(q)) / R.FIX / 1000)
