"""Field decoding without a GPU: the restatement (tests/decode_restate.py) against the strings the REAL reference returned
(tests/golden/decode.npz, written by tests/golden/make_golden_decode.py), hand-written known answers for the filing quirk and the
double threshold, the argument checks of vbg_field_decode (they return before any launch), and the host side of vbg/decode.py."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import decode_restate as R
from vbg import decode as D
from vbg import lib as L

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode.npz")


def golden_cases():
    g = np.load(GOLDEN, allow_pickle=False)
    return [(str(n), g[f"x_{n}"], [str(t) for t in g[f"text_{n}"]], [str(s) for s in g[f"want_{n}"]]) for n in g["names"]]


def test_restatement_reproduces_every_golden_string():
    cases = golden_cases()
    assert {"n1", "n2_diff_second_wins", "last_single_after_long", "tie_first_wins", "random300"} <= {c[0] for c in cases}
    for name, x, texts, want in cases:
        got = R.decode(x, x.shape[1], texts, rule="concat")
        assert got[1:] == want, (name, got[1:], want)          # the reference function returns classes 1 .. C - 1


def test_filing_quirk_known_answers():
    # N == 1: prev_class == -1 files the only record under the LAST class
    assert R.stage2([3], [0.7], 5) == [None, None, None, None, (0, 1, 0.7)]
    # N == 2, two classes: both records land under the first row's class; the second row's class gets nothing
    assert R.stage2([1, 2], [0.6, 0.9], 4) == [None, (1, 1, 0.9), None, None]
    assert R.stage2([1, 2], [0.9, 0.6], 4) == [None, (0, 1, 0.9), None, None]
    assert R.stage2([1, 1], [0.5, 1.0], 4) == [None, (0, 2, 0.75), None, None]
    # a final one-segment run after a longer one is filed under the longer run's class, behind its record
    assert R.stage2([2, 2, 2, 3], [0.5, 0.5, 0.5, 0.75], 4) == [None, None, (3, 1, 0.75), None]
    assert R.stage2([2, 2, 2, 3], [0.5, 0.5, 0.5, 0.25], 4) == [None, None, (0, 3, 0.5), None]
    # ties: the first filed record wins; class 0 is a class like any other; nothing for an empty document
    assert R.stage2([1, 0, 1, 0, 0], [0.5, 0.25, 0.5, 0.5, 0.5], 2) == [(3, 2, 0.5), (0, 1, 0.5)]
    assert R.stage2([], [], 3) == [None, None, None]


def test_threshold_is_compared_in_double():
    cls, score = R.stage1([[0.0, 1.0]])
    assert cls == [1] and abs(score[0] - 0.7310585786300049) < 1e-15      # 1 / (1 + e^-1)
    s32 = np.float32(0.7310586)                                           # a device score: an fp32 value
    t = math.nextafter(float(s32), 1.0)                                   # the smallest double above it
    assert np.float32(t) == s32                                           # ... which an fp32 comparison cannot tell from the score
    assert R.threshold([1], [s32], float(s32)) == [1]                     # score < t is false at t == score
    assert R.threshold([1], [s32], t) == [0]                              # and true one double further
    assert R.threshold([1], [s32], None) == [1] and R.threshold([1], [s32], 0.0) == [1]


def _off(*v):
    return (C.c_int * len(v))(*v)


def test_argument_checks_return_before_any_launch():
    f = L.lib.vbg_field_decode
    host = (C.c_double * 2 * 130)()                                       # stands in for a pointer that is never dereferenced
    p = C.c_void_p(C.addressof(host))
    assert f(p, None, 1, 5, 0, 0.0, p, p, p, None) == -1                  # null row ranges
    assert f(p, _off(0, 4), 1, 5, 0, 0.0, p, p, None, None) == -1         # null table
    assert f(None, _off(0, 4), 1, 5, 0, 0.0, p, p, p, None) == -1         # null scores with rows to read
    assert f(p, _off(0, 4), 1, 5, 0, 0.0, None, p, p, None) == -1
    assert f(p, _off(0, 4), 1, 5, 0, 0.0, p, None, p, None) == -1
    assert f(p, _off(0, 4), 1, 0, 0, 0.0, p, p, p, None) == -1            # C outside 1 .. 64
    assert f(p, _off(0, 4), 1, 65, 0, 0.0, p, p, p, None) == -1
    assert f(p, _off(0, 5, 3), 2, 5, 0, 0.0, p, p, p, None) == -1         # decreasing row ranges
    assert f(p, _off(-1, 3), 1, 5, 0, 0.0, p, p, p, None) == -1
    assert f(p, _off(0, 2 ** 20), 1, 5, 0, 0.0, p, p, p, None) == -1      # 2^20 rows in one document
    assert f(p, _off(0), -1, 5, 0, 0.0, p, p, p, None) == -1
    assert f(None, _off(0), 0, 5, 0, 0.0, None, None, None, None) == 0    # no document: nothing to do


def test_record_layout_matches_the_header():
    assert D.REC.itemsize == 16 and [D.REC.fields[k][1] for k in ("start", "len", "mean")] == [0, 4, 8]
    src = open(os.path.join(os.path.dirname(GOLDEN), "..", "..", "include", "vbg.h")).read()
    assert "typedef struct vbg_decode_rec { int start; int len; double mean; } vbg_decode_rec;" in src


def _table(*recs):
    t = np.zeros(len(recs), dtype=D.REC)
    for i, (s, ln, m) in enumerate(recs):
        t[i] = (s, ln, m)
    return t


def test_host_joiner_rules():
    texts = ["A", "INV-", "001", "x", "B-", "C"]
    table = _table((-1, 0, 0.0), (1, 3, 0.9), (0, 1, 0.5), (4, 2, 0.7), (0, 6, 0.6))
    assert D.join_winners(table, texts, "space_before") == ["", "INV-001 x", "A", "B-C", "A INV-001 x B-C"]
    assert D.join_winners(table, texts, "concat") == ["", "INV-001x", "A", "B-C", "AINV-001xB-C"]
    # deployment/inference_SROIE appends `t + " "`: the first segment gets no space of its own, the last one does
    assert D.join_winners(table, texts, "space_after") == ["", "INV-001x ", "A", "B-C", "AINV- 001 x B- C "]
    for rule in D.JOIN:                                                   # the module's rules and the restatement's agree
        assert D.join_winners(table, texts, rule) == R.strings([None if r["start"] < 0 else (r["start"], r["len"], r["mean"]) for r in table], texts, rule)
    with pytest.raises(KeyError):
        D.join_winners(table, texts, "tabs")


def test_field_strings_makes_one_launch_call(monkeypatch):
    """the ops wrapper replaced by a recorder that answers from the restatement: one call per document, one table read"""
    name, x, texts, want = [c for c in golden_cases() if c[0] == "random300"][0]
    calls = []

    def recorder(pred, doc_off=None, thresh=None):
        calls.append((tuple(pred.shape), list(doc_off), thresh))
        cls, score = R.stage1(pred.tolist(), thresh)
        table = _table(*[(-1, 0, 0.0) if w is None else w for w in R.stage2(cls, score, pred.shape[1])])
        return torch.tensor(cls, dtype=torch.int32), torch.tensor(score, dtype=torch.float32), torch.from_numpy(table.view(np.float64).reshape(-1, 2))

    monkeypatch.setattr(D.ops, "field_decode", recorder)
    monkeypatch.setattr(D, "_check_pred_label", lambda t: None)           # (the recorder takes the host tensor the check would refuse)
    got = D.field_strings(torch.from_numpy(x), x.shape[1], (texts,), join="concat")
    assert calls == [((300, 12), [0, 300], None)]
    assert got[1:] == want
    assert D.field_strings(torch.from_numpy(x), x.shape[1], texts, thresh=0.25, join="concat")[1:] == want      # plain list of texts; every score is above 0.25
    assert len(calls) == 2 and calls[1][2] == 0.25


def test_wrong_inputs_raise():
    x = torch.zeros(4, 5)
    with pytest.raises(TypeError):
        D.decode_fields(x)                                                # not on the device
    with pytest.raises(TypeError):
        D.field_strings(torch.zeros(4, dtype=torch.int64), 5, ["a"] * 4)  # the crf mode's tag vector
    with pytest.raises(TypeError):
        D.field_strings(x.double(), 5, ["a"] * 4)
