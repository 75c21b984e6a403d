"""Validation metrics without a GPU: the restatement (tests/metrics_restate.py) against known answers of seqeval's default mode and
against the counts the REAL reference token_F1_criteria returned (tests/golden/metrics.npz, written by
tests/golden/make_golden_metrics.py); the tag table of vbg/metrics.py and its errors; SequenceMetrics' finishing arithmetic on a
hand-made table, zero divisions included; all_reduce without a process group; the input type errors; the argument checks of
vbg_seq_metrics (they return before any launch)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import metrics_restate as R
from vbg import lib as L
from vbg import metrics as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics.npz")

FUNSD_BIO = {"O": 0, "B-HEADER": 1, "I-HEADER": 2, "B-QUESTION": 3, "I-QUESTION": 4, "B-ANSWER": 5, "I-ANSWER": 6}


@pytest.mark.parametrize("tags, want", [
    (["B-PER", "I-PER", "O", "B-LOC"], [("PER", 0, 1), ("LOC", 3, 3)]),
    (["I-A", "I-A", "I-B", "O"], [("A", 0, 1), ("B", 2, 2)]),
    (["B-A", "B-A"], [("A", 0, 0), ("A", 1, 1)]),
    (["S-A", "E-A", "I-A"], [("A", 0, 0), ("A", 1, 1), ("A", 2, 2)]),
    (["O", "E-A"], [("A", 1, 1)]),
    (["B", "I", "O", "I-X"], [("_", 0, 1), ("X", 3, 3)]),
    ([], []),
    (["O", "O"], []),
])
def test_entity_lists_known_answers(tags, want):
    assert R.get_entities(tags) == want


README_TRUE = [["O", "O", "O", "B-MISC", "I-MISC", "I-MISC", "O"], ["B-PER", "I-PER", "O"]]
README_PRED = [["O", "O", "B-MISC", "I-MISC", "I-MISC", "I-MISC", "O"], ["B-PER", "I-PER", "O"]]


def test_seqeval_readme_pair():
    assert R.entity_counts(README_TRUE, README_PRED) == {"MISC": [1, 1, 0], "PER": [1, 1, 1]}
    m = M.SequenceMetrics(5, {"O": 0, "B-MISC": 1, "I-MISC": 2, "B-PER": 3, "I-PER": 4}, device="cpu")
    assert m.types == ["MISC", "PER", "_"]
    flat = np.zeros(3 * 3 + 25 + 20, dtype=np.int64)
    flat[:9] = [1, 1, 0, 1, 1, 1, 0, 0, 0]
    m.load_counts(flat)
    for avg in ("micro", "macro", "weighted"):
        assert m.entity_scores(avg) == (0.5, 0.5, 0.5), avg
    p, r, f = m.entity_scores(None)
    assert p.tolist() == [0.0, 1.0] and r.tolist() == [0.0, 1.0] and f.tolist() == [0.0, 1.0]          # MISC, PER: `_` does not occur
    d = m.report_dict()
    assert list(d) == ["MISC", "PER", "micro avg", "macro avg", "weighted avg"]
    assert d["MISC"]["support"] == 1 and d["PER"]["support"] == 1 and d["micro avg"]["support"] == 2
    text = m.report(digits=3)
    assert "MISC" in text and "weighted avg" in text and "0.500" in text and "1.000" in text


def golden_cases():
    g = np.load(GOLDEN, allow_pickle=False)
    return [(str(n), g[f"x_{n}"], g[f"gt_{n}"], g[f"counts_{n}"], g[f"prf_{n}"]) for n in g["names"]]


def test_restatement_reproduces_the_reference_token_counts():
    cases = golden_cases()
    assert {x.shape[1] for _, x, _, _, _ in cases} == {2, 5, 7} and len(cases) >= 6
    for name, x, gt, counts, prf in cases:
        got = R.token_counts(x.tolist(), gt.tolist(), x.shape[1])
        assert got == counts.tolist(), name
        d = R.token_f1(got)
        assert [[d[k][key] for key in ("precision", "recall", "F1")] for k in range(x.shape[1])] == prf.tolist(), name


def test_token_f1_dict_from_a_table_is_the_reference_dict():
    for name, x, gt, counts, prf in golden_cases():
        c = x.shape[1]
        m = M.SequenceMetrics(c, device="cpu")
        m.load_counts(np.concatenate([np.zeros(c * c, dtype=np.int64), counts.reshape(-1)]))
        d = m.token_f1()
        assert list(d) == list(range(c)) + ["num_classes"] and d["num_classes"] == c
        for k in range(c):
            assert list(d[k]) == ["TP", "TN", "FP", "FN", "precision", "recall", "F1"]
            assert [d[k][key] for key in ("TP", "TN", "FP", "FN")] == counts[k].tolist() and isinstance(d[k]["TP"], int)
            assert [d[k][key] for key in ("precision", "recall", "F1")] == prf[k].tolist(), (name, k)


def test_tag_table_parsing():
    types, prefix, type_id = M.parse_tags(FUNSD_BIO, 7)
    assert types == ["ANSWER", "HEADER", "QUESTION", "_"]
    assert prefix == [0, 1, 2, 1, 2, 1, 2] and type_id == [3, 1, 1, 2, 2, 0, 0]
    assert M.split_tag("B-A-B") == ("B", "A-B") and M.split_tag("I") == ("I", "_") and M.split_tag("O") == ("O", "_")
    iobes = {"O": 0, "B-X": 1, "I-X": 2, "E-X": 3, "S-X": 4, "S": 5}
    assert M.parse_tags(iobes, 6) == (["X", "_"], [0, 1, 2, 3, 4, 4], [1, 0, 0, 0, 0, 1])
    assert M.parse_tags(iobes, 3)[0] == ["X", "_"]                                  # tags beyond num_classes are not looked at
    m = M.SequenceMetrics(6, iobes, device="cpu")
    assert list(m._table.prefix[:6]) == [0, 1, 2, 3, 4, 4] and list(m._table.type[:6]) == [1, 0, 0, 0, 0, 1]


def test_tag_table_errors():
    with pytest.raises(ValueError, match="class index 2"):
        M.SequenceMetrics(3, {"O": 0, "B-A": 1}, device="cpu")
    with pytest.raises(ValueError, match="prefix"):
        M.SequenceMetrics(2, {"O": 0, "X-A": 1}, device="cpu")
    with pytest.raises(ValueError, match="prefix"):
        M.SequenceMetrics(2, {"O": 0, "": 1}, device="cpu")
    many = {"O": 0}
    many.update({f"B-T{k}": k + 1 for k in range(63)})
    assert len(M.SequenceMetrics(64, many, device="cpu").types) == 64                # 63 types and `_`
    many.pop("O")
    many["B-T63"] = 0
    assert len(M.SequenceMetrics(64, many, device="cpu").types) == 64
    with pytest.raises(ValueError, match="num_classes"):
        M.SequenceMetrics(65, device="cpu")
    with pytest.raises(ValueError, match="num_classes"):
        M.SequenceMetrics(0, device="cpu")
    with pytest.raises(ValueError, match="65 entity types"):
        M.parse_tags({f"B-T{k}": k for k in range(65)}, 65)


def test_finishing_arithmetic_on_a_hand_made_table():
    tags = {"O": 0, "B-A": 1, "I-A": 2, "B-B": 3, "I-B": 4, "B-C": 5, "B-D": 6}
    m = M.SequenceMetrics(7, tags, device="cpu")
    assert m.types == ["A", "B", "C", "D", "_"]
    flat = np.zeros(15 + 49 + 28, dtype=np.int64)
    #            A: true 4, pred 2, ok 1     B: 0, 3, 0     C: 2, 0, 0     D: never     _: never
    flat[:15] = [4, 2, 1, 0, 3, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0]
    conf = np.arange(49).reshape(7, 7)
    flat[15:64] = conf.reshape(-1)
    flat[64:68] = [3, 5, 1, 0]                                                     # class 0: TP 3, TN 5, FP 1, FN 0; the others all zero
    m.load_counts(flat)
    c = m.counts()
    assert c.entity.shape == (5, 3) and c.confusion.shape == (7, 7) and c.token.shape == (7, 4) and c.entity.dtype == np.int64
    p, r, f = m.entity_scores(None)                                                # A, B, C occur; D and _ do not
    pa, ra = 1 / 2, 1 / 4
    fa = 2 * pa * ra / (pa + ra)
    assert p.tolist() == [pa, 0.0, 0.0] and r.tolist() == [ra, 0.0, 0.0] and f.tolist() == [fa, 0.0, 0.0]      # 0 / 0 -> 0, both ways
    assert m.entity_scores("micro") == (1 / 5, 1 / 6, 2 * (1 / 5) * (1 / 6) / (1 / 5 + 1 / 6))
    assert m.entity_scores("macro") == (pa / 3, ra / 3, fa / 3)
    assert m.entity_scores("weighted") == (pa * 4 / 6, ra * 4 / 6, fa * 4 / 6)
    assert list(m.report_dict()) == ["A", "B", "C", "micro avg", "macro avg", "weighted avg"]
    assert np.array_equal(m.confusion(), conf)
    assert m.accuracy() == (float(np.trace(conf)), int(conf.sum())) and isinstance(m.accuracy()[0], float)
    d = m.token_f1()
    assert d[0]["precision"] == 3 / (4 + 1e-8) and d[0]["recall"] == 3 / (3 + 1e-8)
    assert d[1] == {"TP": 0, "TN": 0, "FP": 0, "FN": 0, "precision": 0.0, "recall": 0.0, "F1": 0.0}
    with pytest.raises(ValueError, match="average"):
        m.entity_scores("samples")
    with pytest.raises(ValueError, match="counts"):
        m.load_counts(np.zeros(5))
    # an empty table: every average is 0, nothing divides by zero
    m.reset()
    assert int(m.counts().entity.sum()) == 0
    for avg in ("micro", "macro", "weighted"):
        assert m.entity_scores(avg) == (0.0, 0.0, 0.0)
    assert [len(v) for v in m.entity_scores(None)] == [0, 0, 0]
    assert m.accuracy() == (0.0, 0) and list(m.report_dict()) == ["micro avg", "macro avg", "weighted avg"] and m.report()
    # true entities that were never predicted, and the other way round
    flat[:] = 0
    flat[:3] = [2, 0, 0]
    m.load_counts(flat)
    assert m.entity_scores("micro") == (0.0, 0.0, 0.0) and m.entity_scores("weighted") == (0.0, 0.0, 0.0)
    flat[:3] = [0, 2, 0]
    m.load_counts(flat)
    assert m.entity_scores("weighted") == (0.0, 0.0, 0.0) and m.entity_scores("macro") == (0.0, 0.0, 0.0)


def test_entity_calls_need_the_tag_table_token_calls_do_not():
    m = M.SequenceMetrics(3, device="cpu")
    assert m.types == [] and m.counts().entity.shape == (0, 3)
    assert m.token_f1()["num_classes"] == 3 and m.confusion().shape == (3, 3) and m.accuracy() == (0.0, 0)
    for call in (m.entity_scores, m.report, m.report_dict):
        with pytest.raises(ValueError, match="tag_to_idx"):
            call()


def test_all_reduce_without_a_process_group_changes_nothing():
    m = M.SequenceMetrics(2, device="cpu")
    flat = np.arange(12, dtype=np.int64)
    m.load_counts(flat)
    m.all_reduce()
    assert np.array_equal(np.concatenate([v.reshape(-1) for v in m.counts()]), flat)


def test_input_type_errors():
    m = M.SequenceMetrics(3, {"O": 0, "B-A": 1, "I-A": 2}, device="cpu")
    gt = torch.zeros(4, dtype=torch.int32)
    for bad in (torch.zeros(4, 3), [[0.0] * 3] * 4, np.zeros((4, 3), dtype=np.float32), torch.zeros(4, dtype=torch.int64)):
        with pytest.raises(TypeError, match="pred_label"):       # host tensors, lists, arrays: the scores must lie on the device
            m.update(bad, gt)
    assert int(m.counts().confusion.sum()) == 0


def test_wide_labels_do_not_wrap_into_a_class():
    """the kernel reads int32: a 64-bit label outside [0, C) must reach it as an out-of-range value, not as its low 32 bits"""
    m = M.SequenceMetrics(7, device="cpu")
    wide = torch.tensor([0, 6, 7, -1, 2 ** 32 + 1, -2 ** 32 + 2, 2 ** 40, 2 ** 31, 2 ** 63 - 1, -2 ** 63])
    got = m._labels_i32(wide)
    assert got.dtype == torch.int32 and got.tolist() == [0, 6, -1, -1, -1, -1, -1, -1, -1, -1]
    for dtype in (torch.int8, torch.uint8, torch.int16, torch.int32):
        narrow = torch.tensor([0, 6, 7, 100], dtype=dtype)
        assert m._labels_i32(narrow).tolist() == [0, 6, 7, 100] and m._labels_i32(narrow).dtype == torch.int32


def null_table():
    return L.TagTable()


def bio_table(c):
    t = L.TagTable()
    for k in range(c):
        t.prefix[k], t.type[k] = (0, 0) if k == 0 else (1 + (k - 1) % 2, 1)
    return t


def test_argument_errors_do_not_need_a_gpu():
    """every rejected call returns -1 before a launch (there is no device here to launch on); pointers are never dereferenced"""
    f = L.lib.vbg_seq_metrics
    off = lambda *v: (C.c_int * len(v))(*v)      # noqa: E731
    x, tags, gt, counts = C.c_void_p(0x1000), C.c_void_p(0x2000), C.c_void_p(0x3000), C.c_void_p(0x4000)
    assert f(x, None, gt, off(0), 0, 5, 2, bio_table(5), counts, None) == 0                   # ndoc == 0: valid, counts nothing
    assert f(x, None, gt, off(0), 0, 5, 2, bio_table(5), None, None) == 0
    assert f(None, tags, gt, off(3, 3, 3), 2, 5, 2, bio_table(5), counts, None) == 0          # empty sequences only
    assert f(x, None, gt, off(0, 4), 1, 0, 0, null_table(), counts, None) == -1               # C out of range
    assert f(x, None, gt, off(0, 4), 1, 65, 0, null_table(), counts, None) == -1
    assert f(x, None, gt, off(0, 4), 1, 5, -1, null_table(), counts, None) == -1              # T out of range
    assert f(x, None, gt, off(0, 4), 1, 5, 65, bio_table(5), counts, None) == -1
    assert f(x, tags, gt, off(0, 4), 1, 5, 2, bio_table(5), counts, None) == -1               # both inputs
    assert f(None, None, gt, off(0, 4), 1, 5, 2, bio_table(5), counts, None) == -1            # neither
    assert f(None, None, gt, off(0), 0, 5, 2, bio_table(5), counts, None) == -1
    assert f(x, None, gt, off(-1, 4), 1, 5, 2, bio_table(5), counts, None) == -1              # negative offset
    assert f(x, None, gt, off(0, 4, 3), 2, 5, 2, bio_table(5), counts, None) == -1            # decreasing offsets
    assert f(x, None, gt, None, 1, 5, 2, bio_table(5), counts, None) == -1
    assert f(x, None, gt, off(0, 4), -1, 5, 2, bio_table(5), counts, None) == -1
    assert f(x, None, gt, off(0, 4), 1, 5, 2, bio_table(5), None, None) == -1                 # no table to add to
    assert f(x, None, gt, off(0, 0), 1, 5, 2, bio_table(5), None, None) == -1
    assert f(x, None, None, off(0, 4), 1, 5, 2, bio_table(5), counts, None) == -1             # rows without gt
    assert f(x, None, gt, off(0, 4), 1, 5, 1, bio_table(5), counts, None) == -1               # a type id >= T
    bad = bio_table(5)
    bad.prefix[4] = 5
    assert f(x, None, gt, off(0, 4), 1, 5, 2, bad, counts, None) == -1                        # a prefix code that is no letter
    bad.prefix[4] = 1
    bad.prefix[5] = 9                                                                         # beyond C: not looked at
    assert f(x, None, gt, off(3, 3), 1, 5, 2, bad, counts, None) == 0
