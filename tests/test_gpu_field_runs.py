"""vbg_field_runs / vbg_field_runs_tags on the device (csrc/decode.hip; ops.field_runs, ops.field_runs_tags, vbg/decode.py list_fields,
list_crf_fields): EVERY run of every document, one record per row, one launch.  Needs a real MI355X.

Classes and scores must be ops.field_decode's / ops.field_decode_tags's bits; start, len, cls and the bits of the fp64 mean must EQUAL
the restatement (tests/crf_span_restate.py list_runs) fed those classes and scores; logp must lie within 1e-9 of the fp64 sum of the
lm / lc that were passed in; a row that starts no run holds a record of zeros.  The class sequences are designed -- by writing the
scores, or the tag path -- around the 256-row chunk walk and the 64-lane ballots: a run across the chunk border, heads on rows 255 and
256, on the first and the last lane of a wave, a single-row last run, one run of 513 rows, 513 runs of one row, and for tags consecutive
begin tags and a begin tag behind a row of its own class."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import crf_posterior_restate as R
import crf_span_restate as S
from test_gpu_decode_tags import bio_table, random_case
from test_gpu_field_decode import classed

LENS = [[1], [2], [255, 256, 257], [513], [0, 3, 0]]
HEADS = {"border": (0, 64, 127, 250, 261), "edges": (0, 63, 64, 255, 256, 320)}      # + the last row: a single-row last run


@pytest.fixture(scope="module")
def ops():
    from vbg import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def D():
    from vbg import decode
    return decode


def dev():
    return torch.device("cuda")


def bits64(v):
    return np.asarray(v, dtype=np.float64).view(np.int64)


def offsets(lens):
    off = [0]
    for n in lens:
        off.append(off[-1] + n)
    return off


def classes(n, C, kind, shift=0):
    """the class of each of n rows: "border" / "edges": runs that start on HEADS and on the last row, a new class at every head;
    "one": one run; "each": every row a run"""
    if kind == "one":
        return [1 + shift % (C - 1)] * n
    if kind == "each":
        return [1 + (r + shift) % (C - 1) for r in range(n)]
    heads = set(HEADS[kind]) | {n - 1}
    out, c = [], shift
    for r in range(n):
        if r in heads:
            c += 1
        out.append(c % C)                                    # (class 0 takes its turn as well)
    return out


def tag_table(C):
    """C 5: "O", B-1 I-1 .. B-4 I-4; C 64: tag k is class k and the odd tags open a run"""
    return bio_table(4) if C == 5 else (list(range(64)), [k % 2 for k in range(64)])


def tags_for(cls, C):
    """a tag path with these classes: C 5: B-c on the first row of a stretch, I-c behind it; C 64: the class itself"""
    if C == 64:
        return list(cls)
    return [0 if c == 0 else (2 * c - 1 if r == 0 or cls[r - 1] != c else 2 * c) for r, c in enumerate(cls)]


def records(D, raw, off):
    rec = raw.cpu().numpy().view(D.RUN).reshape(-1)
    return [rec[lo:hi] for lo, hi in zip(off[:-1], off[1:])]


def compare(D, recs, want, logp_tol):
    """one document's raw records [n] against the restatement's list"""
    heads = recs[recs["len"] > 0]
    assert heads["start"].tolist() == [w[0] for w in want]
    assert heads["len"].tolist() == [w[1] for w in want]
    assert heads["cls"].tolist() == [w[2] for w in want]
    assert np.array_equal(bits64(heads["mean"]), bits64([w[3] for w in want]))
    if logp_tol is None:
        assert bool((heads["logp"] == 0.0).all())
    elif len(want):
        err = np.abs(heads["logp"] - np.array([w[4] for w in want]))
        print("runs", len(want), "max |logp - fp64 sum|", float(err.max()))
        assert float(err.max()) <= logp_tol
    assert np.nonzero(recs["len"] > 0)[0].tolist() == [w[0] for w in want]              # a run's record lies at its first row
    rest = recs[recs["len"] == 0]
    for name in D.RUN.names:
        assert bool((rest[name] == 0).all()), name                                     # every other row: a record of zeros
    assert bool((recs["pad"] == 0).all())


def best_table(runs_per_doc, C):
    nd = len(runs_per_doc)
    start, length, mean = np.full((nd, C), -1, np.int32), np.zeros((nd, C), np.int32), np.zeros((nd, C))
    for d, runs in enumerate(runs_per_doc):
        lst = [(int(r["start"]), int(r["len"]), int(r["cls"]), float(r["mean"]), 0.0) for r in runs]
        for c, w in enumerate(S.best_of(lst, C)):
            if w is not None:
                start[d, c], length[d, c], mean[d, c] = w
    return start, length, mean


def check_scores(ops, D, x, lens, thresh=None):
    off = offsets(lens)
    C = x.shape[1]
    xd = x.to(dev())
    cls, score, raw = ops.field_runs(xd, off, thresh)
    dcls, dscore, _ = ops.field_decode(xd, off, thresh)
    torch.cuda.synchronize()
    assert torch.equal(cls, dcls) and torch.equal(score.view(torch.int32), dscore.view(torch.int32))
    c, s = cls.cpu().tolist(), score.cpu().numpy()
    want = [S.list_runs(c[lo:hi], s[lo:hi], None, None, None, False) for lo, hi in zip(off[:-1], off[1:])]
    for recs, w in zip(records(D, raw, off), want):
        compare(D, recs, w, None)
    out = D.list_fields(xd, thresh=thresh, doc_off=off)
    assert len(out.runs) == len(lens) and out.doc_off == off
    for got, w in zip(out.runs, want):
        assert got["start"].tolist() == [r[0] for r in w] and bool(np.isnan(got["logp"]).all())
    # the best run per class from the list: the restatement's, every run under its own class (the winner loop's quirk is not carried)
    start, length, mean = best_table(out.runs, C)
    for d, w in enumerate(want):
        for k, b in enumerate(S.best_of(w, C)):
            assert (int(start[d, k]), int(length[d, k])) == ((-1, 0) if b is None else b[:2])
            assert b is None or bits64(mean[d, k]) == bits64(b[2])
    return out, want


def check_tags(ops, D, m, path, lens, C, thresh=None, seed=0):
    off = offsets(lens)
    tc, tb = tag_table(C)
    n = m.shape[0]
    g = torch.Generator().manual_seed(9000 + seed)
    lm, lc = -3.0 * torch.rand(n, generator=g), -3.0 * torch.rand(n, generator=g)       # any fp32 values: the kernel adds what it is given
    md, pd, lmd, lcd = m.to(dev()), torch.tensor(path, dtype=torch.int32, device=dev()), lm.to(dev()), lc.to(dev())
    cls, score, raw = ops.field_runs_tags(md, pd, lmd, lcd, tc, tb, C, off, thresh)
    dcls, dscore, _ = ops.field_decode_tags(md, pd, tc, tb, C, off, thresh)
    torch.cuda.synchronize()
    assert torch.equal(cls, dcls) and torch.equal(score.view(torch.int32), dscore.view(torch.int32))
    c, s = cls.cpu().tolist(), score.cpu().numpy()
    l64, c64 = lm.numpy().astype(np.float64), lc.numpy().astype(np.float64)
    want = []
    for lo, hi in zip(off[:-1], off[1:]):
        want.append(S.list_runs(c[lo:hi], s[lo:hi], [bool(tb[t]) for t in path[lo:hi]], l64[lo:hi], c64[lo:hi], True))
    for recs, w in zip(records(D, raw, off), want):
        compare(D, recs, w, 1e-9)
    table = D.TagTable(tc, tb)
    out = D.list_crf_fields((md, pd), (lmd, lcd), table, C, thresh=thresh, doc_off=off)
    for got, w in zip(out.runs, want):
        assert got["start"].tolist() == [r[0] for r in w] and got["cls"].tolist() == [r[2] for r in w]
    # the best run per class from the list is the table of winners
    best = D.decode_tags((md, pd), table, C, thresh=thresh, doc_off=off).best
    start, length, mean = best_table(out.runs, C)
    assert np.array_equal(best["start"], start) and np.array_equal(best["len"], length)
    assert np.array_equal(bits64(best["mean"]), bits64(mean))
    return out, want


def designed(lens, C, kind):
    cls = []
    for k, n in enumerate(lens):
        cls += classes(n, C, kind, shift=k)
    return cls


@pytest.mark.parametrize("C", [5, 64])
@pytest.mark.parametrize("lens", LENS, ids=lambda v: "-".join(str(n) for n in v))
@pytest.mark.parametrize("kind", ["border", "edges", "one", "each"])
def test_scores_designed(ops, D, kind, lens, C):
    cls = designed(lens, C, kind)
    out, want = check_scores(ops, D, classed(cls, C, seed=len(cls) + C), lens)
    assert out.cls.cpu().tolist() == cls
    off = offsets(lens)
    for d, n in enumerate(lens):
        got = [(int(r["start"]), int(r["len"])) for r in out.runs[d]]
        assert got == R.runs(cls[off[d]:off[d + 1]], [False] * n)                       # the runs that were designed
        if kind == "one" and n:
            assert got == [(0, n)]
        if kind == "each":
            assert len(got) == n


@pytest.mark.parametrize("C", [5, 64])
@pytest.mark.parametrize("lens", LENS, ids=lambda v: "-".join(str(n) for n in v))
@pytest.mark.parametrize("kind", ["border", "edges", "one", "each"])
def test_tags_designed(ops, D, kind, lens, C):
    cls = designed(lens, C, kind)
    path = []
    off = offsets(lens)
    for d in range(len(lens)):
        path += tags_for(cls[off[d]:off[d + 1]], C)
    tc, _ = tag_table(C)
    m, _ = random_case(len(path), tc, seed=len(path) + C)
    out, want = check_tags(ops, D, m, path, lens, C, seed=len(path))
    assert out.cls.cpu().tolist() == [tc[t] for t in path]
    if kind == "one" and C == 5:
        for d, n in enumerate(lens):
            assert [(int(r["start"]), int(r["len"])) for r in out.runs[d]] == ([(0, n)] if n else [])


@pytest.mark.parametrize("lens", [[513], [255, 256, 257]], ids=["513", "255-256-257"])
def test_tags_begin_tags(ops, D, lens):
    n = sum(lens)
    tc, tb = tag_table(5)
    m, _ = random_case(n, tc, seed=31)
    # consecutive begin tags: every row its own run, all of one class
    out, _ = check_tags(ops, D, m, [1] * n, lens, 5, seed=1)
    for d, k in enumerate(lens):
        assert out.runs[d]["len"].tolist() == [1] * k and out.runs[d]["cls"].tolist() == [1] * k
    # a begin tag behind rows of its own class, on rows 255, 256 and elsewhere: I-1 I-1 B-1 I-1 ...
    path = [2] * n
    for r in list(range(7, n, 50)) + [255, 256, n - 1]:
        path[r] = 1
    out, _ = check_tags(ops, D, m, path, lens, 5, seed=2)
    off = offsets(lens)
    for d in range(len(lens)):
        heads = [0] + [r - off[d] for r in range(off[d] + 1, off[d + 1]) if path[r] == 1]
        assert out.runs[d]["start"].tolist() == sorted(set(heads))


def test_random_documents_and_rows_in_front(ops, D):
    tc, _ = tag_table(5)
    m, path = random_case(600, tc, seed=41)
    check_tags(ops, D, m, path, [37, 0, 263, 300], 5, seed=3)
    x = classed([int(v) for v in torch.randint(0, 5, (600,), generator=torch.Generator().manual_seed(42))], 5, seed=43)
    check_scores(ops, D, x, [37, 0, 263, 300])
    # documents that start behind row 0: the rows in front belong to nobody and are not written
    xd = x.to(dev())
    cls, score, raw = ops.field_runs(xd, [5, 130, 131, 600])
    whole = ops.field_runs(xd[5:], [0, 125, 126, 595])
    torch.cuda.synchronize()
    assert torch.equal(raw[5:].view(torch.int64), whole[2].view(torch.int64)) and torch.equal(cls[5:], whole[0])


@pytest.mark.parametrize("C", [5, 64])
def test_threshold_in_double(ops, D, C):
    lens = [255, 256, 257]
    cls = designed(lens, C, "border")
    x = classed(cls, C, seed=77)
    base, _ = check_scores(ops, D, x, lens)
    score = base.score.cpu().numpy()
    j = int(np.nonzero(np.array(cls) != 0)[0][300])
    t = float(score[j])
    out, _ = check_scores(ops, D, x, lens, thresh=t)                                   # score < t is false: the row keeps its class
    assert int(out.cls[j]) == cls[j]
    out, _ = check_scores(ops, D, x, lens, thresh=float(np.nextafter(t, 2.0)))
    assert int(out.cls[j]) == 0
    out, _ = check_scores(ops, D, x, lens, thresh=2.0)                                 # every row to class 0: one run per document
    assert [r["len"].tolist() for r in out.runs] == [[255], [256], [257]]
    tc, tb = tag_table(C)
    path = []
    off = offsets(lens)
    for d in range(3):
        path += tags_for(cls[off[d]:off[d + 1]], C)
    m, _ = random_case(len(path), tc, seed=78)
    base, _ = check_tags(ops, D, m, path, lens, C)
    score = base.score.cpu().numpy()
    j = int(np.nonzero(base.cls.cpu().numpy() != 0)[0][300])
    t = float(score[j])
    out, _ = check_tags(ops, D, m, path, lens, C, thresh=t)
    assert int(out.cls[j]) != 0
    out, _ = check_tags(ops, D, m, path, lens, C, thresh=float(np.nextafter(t, 2.0)))
    assert int(out.cls[j]) == 0
    check_tags(ops, D, m, path, lens, C, thresh=2.0)                                    # class 0 everywhere; begin tags still cut


def test_no_document_and_more_than_512_documents(ops, D):
    x = classed([k % 5 for k in range(600)], 5, seed=51)
    out, _ = check_scores(ops, D, x, [1] * 600)
    assert all(len(r) == 1 for r in out.runs)
    tc, _ = tag_table(5)
    m, path = random_case(600, tc, seed=52)
    check_tags(ops, D, m, path, [1] * 600, 5)
    xd = x.to(dev())
    cls, score, raw = ops.field_runs(xd, [0])
    assert tuple(raw.shape) == (600, 4)
    assert D.list_fields(xd[:0], doc_off=[0]).runs == []
    e = torch.zeros(0, dtype=torch.int32, device=dev())
    z = torch.zeros(0, device=dev())
    out = D.list_crf_fields((torch.zeros(0, 9, device=dev()), e), (z, z), D.TagTable(*tag_table(5)), 5, doc_off=[0, 0])
    assert len(out.runs) == 1 and len(out.runs[0]) == 0


def test_argument_errors(ops):
    from vbg.lib import VbgError
    tc, tb = bio_table(2)
    m, path = random_case(8, tc, seed=9)
    d = dev()
    md, pd = m.to(d), torch.tensor(path, dtype=torch.int32, device=d)
    lm = torch.zeros(8, device=d)
    for bad in (dict(tag_class=[0, 1, 1, 3, 2]), dict(tag_class=[0, 1, 1, -1, 2]), dict(tag_begin=[0, 2, 0, 1, 0]), dict(num_classes=65),
                dict(tag_class=tc[:4], tag_begin=tb[:4]), dict(doc_off=[0, 9]), dict(doc_off=[4, 2]), dict(lm=lm[:7]), dict(lc=lm.double()),
                dict(path=pd.long()), dict(path=pd[:7])):
        kw = dict(marginals=md, path=pd, lm=lm, lc=lm, tag_class=tc, tag_begin=tb, num_classes=3)
        kw.update(bad)
        with pytest.raises((VbgError, AssertionError)):
            ops.field_runs_tags(**kw)
    with pytest.raises(VbgError):                                                     # more than 64 tags
        ops.field_runs_tags(torch.zeros(4, 65, device=d), pd[:4], lm[:4], lm[:4], [0] * 65, [0] * 65, 3)
    x = torch.zeros(8, 5, device=d)
    for off in ([0, 9], [4, 2], [-1, 3]):
        with pytest.raises(VbgError):
            ops.field_runs(x, off)
    with pytest.raises(VbgError):                                                     # more than 64 classes
        ops.field_runs(torch.zeros(8, 65, device=d))
    big = 1 << 20                                                                     # 2^20 rows in one document
    xb = torch.zeros(big, 2, device=d)
    with pytest.raises(VbgError):
        ops.field_runs(xb)
    cls, score, raw = ops.field_runs(xb, [0, big - 1, big])
    torch.cuda.synchronize()
    assert int(cls.max()) == 0
