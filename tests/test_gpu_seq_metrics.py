"""vbg_seq_metrics on the device (csrc/metrics.hip; vbg/metrics.py): entity, confusion and literal token counts of a forward from one
launch.  Needs a real MI355X.

Every table is held EXACTLY -- integer for integer -- to the restatement (tests/metrics_restate.py: seqeval's sequential loop, the set
intersection per type, token_F1_criteria's literal counts) fed the classes torch.argmax gives on scores built without ties, plus
dedicated tie rows whose class is written down by hand.  Shapes: every chunk edge of the 256-row walk (255 / 256 / 257 / 513 rows;
entities that span, end at, end behind and start at the edge; one entity over four chunks; 1000 one-row entities), the class counts
1, 2, 7 and the largest, 64, empty sequences, 513 sequences (the second launch), sequences cut inside an entity."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import metrics_restate as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics.npz")

BIO7 = {"O": 0, "B-HEADER": 1, "I-HEADER": 2, "B-QUESTION": 3, "I-QUESTION": 4, "B-ANSWER": 5, "I-ANSWER": 6}
IOBES = {"O": 0, "B-X": 1, "I-X": 2, "E-X": 3, "S-X": 4, "B-Y": 5, "I-Y": 6, "E-Y": 7, "S-Y": 8, "B": 9, "I": 10}


def tags_for(c):
    if c == 1:
        return {"O": 0}
    if c == 2:
        return {"O": 0, "B-A": 1}
    if c == 7:
        return BIO7
    assert c == 64
    out = {"O": 0}
    for ty in range(15):
        for p in "BIES":
            out[f"{p}-T{ty:02d}"] = len(out)
    for tag in ("B", "I", "S"):
        out[tag] = len(out)
    return out


@pytest.fixture(scope="module")
def M():
    from vbg import metrics
    return metrics


def dev():
    return torch.device("cuda")


def scored(classes, c, seed):
    """rows whose class is given and is the only maximum: [-2, 3) everywhere (both sides of -1, 0, 1 and 2: every token cell fills),
    [3.5, 4.5) on the row's class"""
    g = torch.Generator().manual_seed(seed)
    n = len(classes)
    x = torch.rand(n, c, generator=g) * 5.0 - 2.0
    if n:
        x[torch.arange(n), torch.tensor(classes, dtype=torch.long)] = 3.5 + torch.rand(n, generator=g)
    return x


def random_classes(n, c, seed, run=4):
    """gt classes in runs (so that entities of several rows occur) and a prediction that differs from it on about one row in five"""
    g = torch.Generator().manual_seed(seed)
    gt = []
    while len(gt) < n:
        k = int(torch.randint(0, c, (1,), generator=g))
        gt += [k] * int(torch.randint(1, run + 1, (1,), generator=g))
    gt = gt[:n]
    flip = torch.rand(n, generator=g) < 0.2
    other = torch.randint(0, c, (n,), generator=g).tolist()
    return [o if f else k for k, f, o in zip(gt, flip.tolist(), other)], gt


def want_flat(c, tag_to_idx, pred_cls, gt, off, rows=None):
    """the restatement's table in the layout of include/vbg.h; a row with gt or pred outside [0, c) counts nowhere and reads O, O"""
    ok = [0 <= g < c and 0 <= p < c for p, g in zip(pred_cls, gt)]
    conf = R.confusion([p for p, k in zip(pred_cls, ok) if k], [g for g, k in zip(gt, ok) if k], c)
    tok = [[0] * 4 for _ in range(c)]
    if rows is not None:
        tok = R.token_counts([r for r, k in zip(rows, ok) if k], [g for g, k in zip(gt, ok) if k], c)
    ent = []
    if tag_to_idx is not None:
        tag_of = {v: k for k, v in tag_to_idx.items()}
        types = sorted({R.split_tag(tag_of[k])[1] for k in range(c)})
        tr = [[tag_of[g] if k else "O" for g, k in zip(gt[a:b], ok[a:b])] for a, b in zip(off[:-1], off[1:])]
        pr = [[tag_of[p] if k else "O" for p, k in zip(pred_cls[a:b], ok[a:b])] for a, b in zip(off[:-1], off[1:])]
        got = R.entity_counts(tr, pr)
        ent = [got.get(ty, [0, 0, 0]) for ty in types]
    return np.array([v for row in ent for v in row] + [v for row in conf for v in row] + [v for row in tok for v in row], dtype=np.int64)


def flat_of(m):
    return np.concatenate([v.reshape(-1) for v in m.counts()])


def check(M, c, tag_to_idx, pred_cls, gt, doc_off=None, seed=0, as_tags=False):
    """one update on a fresh table against the restatement; -> (SequenceMetrics, expected flat table)"""
    n = len(gt)
    m = M.SequenceMetrics(c, tag_to_idx, device=dev())
    off = [0, n] if doc_off is None else list(doc_off)
    gtd = torch.tensor(gt, dtype=torch.int64).to(dev())
    if as_tags:
        m.update(torch.tensor(pred_cls, dtype=torch.int64).to(dev()), gtd, doc_off=doc_off)
        want = want_flat(c, tag_to_idx, pred_cls[off[0]:off[-1]], gt[off[0]:off[-1]], [o - off[0] for o in off])
    else:
        x = scored(pred_cls, c, seed)
        if n:
            top = x.topk(min(2, c), dim=1).values
            assert c == 1 or float((top[:, 0] - top[:, 1]).min()) > 0.0                   # no ties
            assert x.argmax(1).tolist() == pred_cls
        m.update(x.to(dev()), gtd, doc_off=doc_off)
        want = want_flat(c, tag_to_idx, x.argmax(1).tolist()[off[0]:off[-1]] if n else [], gt[off[0]:off[-1]], [o - off[0] for o in off],
                         rows=x.tolist()[off[0]:off[-1]])
    got = flat_of(m)
    assert got.dtype == np.int64 and got.shape == want.shape
    assert np.array_equal(got, want), (np.nonzero(got != want)[0][:8], got[got != want][:8], want[got != want][:8])
    return m, want


@pytest.mark.parametrize("c", [1, 2, 7, 64])
@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257, 513])
def test_random_rows(M, n, c):
    pred, gt = random_classes(n, c, seed=100 * c + n)
    m, want = check(M, c, tags_for(c), pred, gt, seed=7 * c + n)
    assert int(m.counts().confusion.sum()) == n
    if n >= 255 and c > 1:
        assert int(m.counts().entity.sum()) > 0 and int(m.counts().token.sum()) > 0


def bio(n, spans):
    """O everywhere, (type index 0..2, first row, last row) as B- / I- tags of BIO7"""
    out = [0] * n
    for ty, a, b in spans:
        out[a] = 1 + 2 * ty
        for i in range(a + 1, b + 1):
            out[i] = 2 + 2 * ty
    return out


@pytest.mark.parametrize("span", [(250, 260), (200, 255), (200, 256), (256, 270), (255, 255), (256, 256), (0, 511), (511, 511)])
def test_entities_at_the_chunk_edge(M, span):
    n = 512
    a, b = span
    gt = bio(n, [(1, a, b)])
    m, _ = check(M, 7, BIO7, gt, gt)                                                   # found
    assert m.counts().entity[2].tolist() == [1, 1, 1] and m.entity_scores("micro") == (1.0, 1.0, 1.0)
    m, _ = check(M, 7, BIO7, bio(n, [(2, a, b)]), gt)                                  # same span, another type
    assert m.counts().entity[:, 2].tolist() == [0, 0, 0, 0]
    if b > a:
        m, _ = check(M, 7, BIO7, bio(n, [(1, a + 1, b)]), gt)                          # same type and end, another begin
        assert m.counts().entity[2].tolist() == [1, 1, 0]
        m, _ = check(M, 7, BIO7, bio(n, [(1, a, b - 1)]), gt)                          # same type and begin, another end
        assert m.counts().entity[2].tolist() == [1, 1, 0]
    if a > 0:
        m, _ = check(M, 7, BIO7, bio(n, [(1, a - 1, b)]), gt)
        assert m.counts().entity[2].tolist() == [1, 1, 0]


def test_one_entity_of_1000_rows_carries_its_begin_over_the_chunks(M):
    gt = bio(1000, [(0, 0, 999)])
    m, _ = check(M, 7, BIO7, gt, gt)
    assert m.counts().entity[1].tolist() == [1, 1, 1]
    m, _ = check(M, 7, BIO7, bio(1000, [(0, 1, 999)]), gt)                             # differs in row 0 only: seen 999 rows later
    assert m.counts().entity[1].tolist() == [1, 1, 0]
    gt = bio(1003, [(0, 3, 1002)])                                                     # closed by the virtual O only
    m, _ = check(M, 7, BIO7, gt, gt)
    assert m.counts().entity[1].tolist() == [1, 1, 1]


def test_1000_one_row_entities(M):
    gt = [1] * 1000                                                                    # B-HEADER x 1000
    m, _ = check(M, 7, BIO7, gt, gt)
    assert m.counts().entity[1].tolist() == [1000, 1000, 1000]
    pred = [1, 2] * 500                                                                # B I B I ...: 500 entities, every other begin shared
    m, _ = check(M, 7, BIO7, pred, gt)
    assert m.counts().entity[1].tolist() == [1000, 500, 0]
    m, _ = check(M, 11, IOBES, [4] * 1000, [4, 8] * 500)                               # S-X against S-X, S-Y alternating
    assert m.counts().entity.tolist() == [[500, 1000, 500], [500, 0, 0], [0, 0, 0]]


@pytest.mark.parametrize("n", [1, 256, 257])
def test_last_row_closed_by_the_virtual_o(M, n):
    gt = [0] * (n - 1) + [3]                                                           # ... O B-QUESTION
    m, _ = check(M, 7, BIO7, gt, gt)
    assert m.counts().entity[2].tolist() == [1, 1, 1]
    m, _ = check(M, 7, BIO7, [0] * (n - 1) + [4], gt)                                  # I-QUESTION behind O starts one too
    assert m.counts().entity[2].tolist() == [1, 1, 1]


def test_iobes_tags(M):
    for seed in range(3):
        pred, gt = random_classes(700, 11, seed=40 + seed, run=3)
        m, _ = check(M, 11, IOBES, pred, gt, seed=seed)
        assert m.types == ["X", "Y", "_"] and int(m.counts().entity[2].sum()) > 0      # the bare B / I tags: type `_`


def test_tags_input_equals_scores_input(M):
    pred, gt = random_classes(600, 7, seed=50)
    a, want = check(M, 7, BIO7, pred, gt, seed=1)
    b, _ = check(M, 7, BIO7, pred, gt, as_tags=True)
    assert np.array_equal(a.counts().entity, b.counts().entity) and np.array_equal(a.counts().confusion, b.counts().confusion)
    assert int(b.counts().token.sum()) == 0 and int(a.counts().token.sum()) > 0        # the literal cells come from scores only
    c, _ = check(M, 7, None, pred, gt, as_tags=True)                                   # no tag table: the token tables alone
    assert c.counts().entity.shape == (0, 3) and np.array_equal(c.confusion(), a.confusion())
    assert a.accuracy() == (float(sum(p == g for p, g in zip(pred, gt))), 600)


def test_tie_rows_take_the_first_largest(M):
    x = torch.tensor([[1.0, 1.0, 0.0], [0.0, 2.0, 2.0], [5.0, 5.0, 5.0], [-1.0, -3.0, -1.0], [0.0, -0.0, -1.0], [-0.0, 0.0, -1.0]])
    first = [0, 1, 0, 0, 0, 0]                                                         # by hand: first index of the largest raw score
    gt = [0, 1, 2, 0, 1, 0]
    tags = {"O": 0, "B-A": 1, "I-A": 2}
    m = M.SequenceMetrics(3, tags, device=dev())
    m.update(x.to(dev()), torch.tensor(gt, dtype=torch.int32).to(dev()))
    assert np.array_equal(flat_of(m), want_flat(3, tags, first, gt, [0, 6], rows=x.tolist()))
    assert m.confusion().tolist() == [[3, 0, 0], [1, 1, 0], [1, 0, 0]]


def test_three_sequences_with_empty_ones_between(M):
    pred, gt = random_classes(300, 7, seed=60)
    check(M, 7, BIO7, pred, gt, doc_off=[0, 0, 37, 37, 37, 290, 300, 300])
    check(M, 7, BIO7, pred, gt, doc_off=[5, 37, 37, 290], as_tags=True)                # rows outside the ranges are not touched
    m, _ = check(M, 7, BIO7, pred, gt, doc_off=[10, 10, 10])
    assert int(flat_of(m).sum()) == 0


def test_513_sequences_take_a_second_launch(M):
    pred, gt = random_classes(513 * 3, 7, seed=70, run=5)
    off = list(range(0, 513 * 3 + 1, 3))
    assert len(off) - 1 == 513
    m, _ = check(M, 7, BIO7, pred, gt, doc_off=off)
    one, _ = check(M, 7, BIO7, pred, gt)
    assert int(m.counts().entity[:, 0].sum()) > int(one.counts().entity[:, 0].sum())   # the cuts split entities
    assert np.array_equal(m.confusion(), one.confusion()) and np.array_equal(m.counts().token, one.counts().token)


def test_doc_off_cutting_inside_an_entity(M):
    gt = bio(600, [(0, 100, 400)])
    m, _ = check(M, 7, BIO7, gt, gt, doc_off=[0, 300, 600])
    assert m.counts().entity[1].tolist() == [2, 2, 2]                                  # rows 100 .. 299, and the I- rows 300 .. 400
    m, _ = check(M, 7, BIO7, bio(600, [(0, 100, 399)]), gt, doc_off=[0, 256, 600])
    assert m.counts().entity[1].tolist() == [2, 2, 1]


def test_out_of_range_labels_count_nowhere(M):
    pred, gt = random_classes(520, 7, seed=80)
    for i, v in ((0, -1), (3, 7), (255, 1000), (256, -2 ** 31), (300, 2 ** 31 - 1), (519, 64),
                 (10, 2 ** 32 + 1), (11, -2 ** 32 + 2), (12, 2 ** 40)):                # int64 labels that a plain cast to int32 would wrap into [0, 7)
        gt[i] = v
    m, _ = check(M, 7, BIO7, pred, gt, seed=3)
    assert int(m.counts().confusion.sum()) == 511
    pred[7], pred[256], pred[257], pred[8] = -5, 7, 99, 2 ** 32 + 3                    # tags out of range as well (row 256: both)
    m, _ = check(M, 7, BIO7, pred, gt, as_tags=True)
    assert int(m.counts().confusion.sum()) == 508


def test_updates_accumulate_and_reset_clears(M):
    pa, ga = random_classes(300, 7, seed=90)
    pb, gb = random_classes(257, 7, seed=91)
    _, wa = check(M, 7, BIO7, pa, ga, seed=1)
    _, wb = check(M, 7, BIO7, pb, gb, seed=2)
    m = M.SequenceMetrics(7, BIO7, device=dev())
    m.update(scored(pa, 7, 1).to(dev()), torch.tensor(ga).to(dev()))
    assert np.array_equal(flat_of(m), wa)                                              # (a copy between the updates changes nothing)
    m.update(scored(pb, 7, 2).to(dev()), torch.tensor(gb, dtype=torch.int16).to(dev()))
    assert np.array_equal(flat_of(m), wa + wb)
    m.all_reduce()                                                                     # no process group: the table stays
    assert np.array_equal(flat_of(m), wa + wb)
    m.reset()
    assert int(flat_of(m).sum()) == 0
    m.update(scored(pb, 7, 2).to(dev()), torch.tensor(gb).to(dev()))
    assert np.array_equal(flat_of(m), wb)
    big = M.SequenceMetrics(7, BIO7, device=dev())                                     # the table is 64-bit: a cell beyond 2^32 adds on
    big.load_counts(np.full(wa.shape, 2 ** 40, dtype=np.int64))
    big.update(scored(pa, 7, 1).to(dev()), torch.tensor(ga).to(dev()))
    assert np.array_equal(flat_of(big), wa + 2 ** 40)


def test_same_table_twice_and_in_deterministic_mode(M):
    """The table is the same in deterministic mode BY CONSTRUCTION: vbg_seq_metrics has one form, integer sums, and never reads the
    switch.  The case turns the switch on through ops.set_deterministic, which is all VBG_DETERMINISTIC=1 in the environment does
    (ops reads the variable once, at import, into the same flag), so that a second form added later could not slip past it."""
    from vbg import ops
    pred, gt = random_classes(513 * 2, 64, seed=95, run=3)
    x = scored(pred, 64, 5).to(dev())
    gtd = torch.tensor(gt).to(dev())
    off = list(range(0, 513 * 2 + 1, 2))

    def run():
        m = M.SequenceMetrics(64, tags_for(64), device=dev())
        m.update(x, gtd)
        m.update(x, gtd, doc_off=off)
        return flat_of(m).tobytes()

    first = run()
    assert run() == first
    was = ops._DET_USER[0]
    ops.set_deterministic(True)                                                        # what VBG_DETERMINISTIC=1 sets at import
    try:
        assert ops.deterministic() and run() == first
    finally:
        ops.set_deterministic(was)


def test_reference_token_counts_through_the_device(M):
    g = np.load(GOLDEN, allow_pickle=False)
    for name in g["names"]:
        x, gt = g[f"x_{name}"], g[f"gt_{name}"]
        m = M.SequenceMetrics(x.shape[1], device=dev())
        cut = x.shape[0] // 3
        m.update(torch.from_numpy(x[:cut]).to(dev()), torch.from_numpy(gt[:cut]).to(dev()))
        m.update(torch.from_numpy(x[cut:]).to(dev()), torch.from_numpy(gt[cut:]).to(dev()))
        assert np.array_equal(m.counts().token, g[f"counts_{name}"]), str(name)
        d = m.token_f1()
        assert [[d[k][key] for key in ("precision", "recall", "F1")] for k in range(x.shape[1])] == g[f"prf_{name}"].tolist(), str(name)


def test_rows_with_nan_neither_fault_nor_leave_their_cells(M):
    x = scored(random_classes(600, 5, seed=96)[0], 5, 6)
    x[17, 2] = float("nan")
    x[300] = float("nan")
    x[599, 0] = float("inf")
    m = M.SequenceMetrics(5, {"O": 0, "B-A": 1, "I-A": 2, "B-B": 3, "I-B": 4}, device=dev())
    m.update(x.to(dev()), torch.zeros(600, dtype=torch.int32, device=dev()), doc_off=[0, 400, 600])
    torch.cuda.synchronize()
    assert int(m.counts().confusion.sum()) == 600 and m.counts().confusion[1:].sum() == 0


def test_argument_errors_report_without_launching(M):
    import ctypes as C

    from vbg import lib as L
    from vbg import ops
    m = M.SequenceMetrics(7, BIO7, device=dev())
    x = scored([1] * 10, 7, 1).to(dev())
    gt = torch.ones(10, dtype=torch.int32, device=dev())
    for off in ([0, 11], [0, 6, 5, 10], [-1, 10]):
        with pytest.raises(L.VbgError):
            m.update(x, gt, doc_off=off)
    with pytest.raises(ValueError):
        m.update(x, gt[:9])
    with pytest.raises(ValueError):
        m.update(x[:, :5].contiguous(), gt)
    with pytest.raises(TypeError):
        m.update(x.double(), gt)
    with pytest.raises(TypeError):
        m.update(x, gt.float())
    with pytest.raises(TypeError):
        m.update(x.cpu(), gt)
    f, off = L.lib.vbg_seq_metrics, (C.c_int * 2)(0, 10)
    tags = gt.clone()
    assert f(ops.P(x), ops.P(tags), ops.P(gt), off, 1, 7, 4, m._table, ops.P(m._counts), None) == -1        # both inputs
    assert f(None, None, ops.P(gt), off, 1, 7, 4, m._table, ops.P(m._counts), None) == -1                   # neither
    assert f(ops.P(x), None, ops.P(gt), off, 1, 65, 4, m._table, ops.P(m._counts), None) == -1
    assert f(ops.P(x), None, ops.P(gt), off, 1, 7, 3, m._table, ops.P(m._counts), None) == -1               # a type id >= T
    assert f(ops.P(x), None, ops.P(gt), off, 1, 7, 4, m._table, None, None) == -1
    torch.cuda.synchronize()
    assert int(flat_of(m).sum()) == 0                                                  # nothing was counted
    m.update(x, gt)
    assert m.counts().entity[1].tolist() == [10, 10, 10]
