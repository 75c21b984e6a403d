"""vbg_field_decode_tags on the device (csrc/decode.hip; vbg/decode.py decode_tags): the table of winning runs from the crf mode's
marginals and Viterbi path, one launch.  Needs a real MI355X.

Classes, scores (bits) and the record table (start, length, bits of the fp64 mean) must EQUAL the restatement
(tests/crf_posterior_restate.py decode_tags) fed the same fp32 marginals and the same path: the sums are integers, so there is nothing
to tolerate.  Shapes: documents of 1, 2, 255, 256, 257 and 513 rows (the 256-row chunk walk and its edges), an empty document between
two others, ntag = C = 64."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import crf_posterior_restate as R


@pytest.fixture(scope="module")
def D():
    from vbg import decode
    return decode


def dev():
    return torch.device("cuda")


def bits64(v):
    return np.asarray(v, dtype=np.float64).view(np.int64)


def bio_table(nfield):
    """tags: 0 "O", then B-k, I-k per field k = 1 .. nfield; C = nfield + 1"""
    tc, tb = [0], [0]
    for k in range(1, nfield + 1):
        tc += [k, k]
        tb += [1, 0]
    return tc, tb


def random_case(n, tc, seed, run_len=6):
    """a path in runs of 1 .. run_len rows of one tag and row-normalised random marginals that favour the path's tag"""
    g = torch.Generator().manual_seed(seed)
    ntag = len(tc)
    path = []
    while len(path) < n:
        path += [int(torch.randint(0, ntag, (1,), generator=g))] * int(torch.randint(1, run_len + 1, (1,), generator=g))
    path = path[:n]
    m = torch.rand(n, ntag, generator=g)
    if n:
        m[torch.arange(n), torch.tensor(path, dtype=torch.long)] += 3.0 * torch.rand(n, generator=g)
    m = m / m.sum(1, keepdim=True)
    return m.float(), path


def want_table(m, path, off, tc, tb, C, thresh):
    nd = len(off) - 1
    start = np.full((nd, C), -1, dtype=np.int32)
    length = np.zeros((nd, C), dtype=np.int32)
    mean = np.zeros((nd, C), dtype=np.float64)
    cls, score = [], []
    for d in range(nd):
        c, s, win = R.decode_tags(m[off[d]:off[d + 1]], path[off[d]:off[d + 1]], tc, tb, C, thresh)
        cls += c
        score += s
        for k, w in enumerate(win):
            if w is not None:
                start[d, k], length[d, k], mean[d, k] = w
    return cls, np.array(score, dtype=np.float32), start, length, mean


def check(D, m, path, tc, tb, C, doc_off=None, thresh=None):
    n = m.shape[0]
    off = [0, n] if doc_off is None else list(doc_off)
    table = D.TagTable(tc, tb)
    out = D.decode_tags((m.to(dev()), torch.tensor(path, dtype=torch.int32, device=dev())), table, C, thresh=thresh, doc_off=doc_off)
    assert out.best.shape == (len(off) - 1, C) and out.cls.dtype == torch.int32 and out.score.dtype == torch.float32
    lo, hi = off[0], off[-1]
    cls, score, start, length, mean = want_table(m.numpy()[lo:hi], path[lo:hi], [o - lo for o in off], tc, tb, C, thresh)
    assert out.cls.cpu().tolist()[lo:hi] == cls
    assert np.array_equal(out.score.cpu().numpy()[lo:hi].view(np.int32), score.view(np.int32))
    assert np.array_equal(out.best["start"], start), (out.best["start"], start)
    assert np.array_equal(out.best["len"], length)
    assert np.array_equal(bits64(out.best["mean"]), bits64(mean))
    return out


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 513])
def test_random_documents(D, n):
    tc, tb = bio_table(4)
    out = check(D, *random_case(n, tc, seed=1000 + n), tc, tb, 5)
    assert int((out.best["start"] >= 0).sum()) >= 1
    check(D, *random_case(n, tc, seed=2000 + n), tc, tb, 5, thresh=0.5)


def test_an_empty_document_inside_a_batch_of_three(D):
    tc, tb = bio_table(4)
    m, path = random_case(300, tc, seed=3)
    out = check(D, m, path, tc, tb, 5, doc_off=[0, 37, 37, 300])
    assert bool((out.best["start"][1] == -1).all()) and bool((out.best["len"][1] == 0).all()) and bool((out.best["mean"][1] == 0).all())
    check(D, m, path, tc, tb, 5, doc_off=[5, 130, 131, 300])                         # rows in front of the first document are not touched


def test_a_run_across_the_chunk_edge(D):
    tc, tb = bio_table(2)
    path = [0] * 200 + [2] * 100 + [0] * 50 + [4] * 163                              # I-1 over rows 200 .. 299, I-2 up to the last row
    m, _ = random_case(513, tc, seed=4)
    out = check(D, m, path, tc, tb, 3)
    assert (int(out.best["start"][0, 1]), int(out.best["len"][0, 1])) == (200, 100)
    assert (int(out.best["start"][0, 2]), int(out.best["len"][0, 2])) == (350, 163)  # the last run, under its own class


def test_a_begin_tag_on_row_256_behind_its_own_class(D):
    tc, tb = bio_table(2)
    path = [0] * 250 + [1] + [2] * 5 + [1] + [2] * 43                                # B-1 I-1 x 5 | B-1 (row 256) I-1 x 43
    m = torch.zeros(300, 5)
    m[torch.arange(300), torch.tensor(path)] = 0.5
    m[:, 3] += 0.5
    m[256:, 1] += 0.25                                                               # the second run scores higher: 0.75
    m[256:, 3] -= 0.25
    out = check(D, m, path, tc, tb, 3)
    assert (int(out.best["start"][0, 1]), int(out.best["len"][0, 1]), float(out.best["mean"][0, 1])) == (256, 44, 0.75)
    no_begin = check(D, m, path, tc, [0] * 5, 3)
    assert (int(no_begin.best["start"][0, 1]), int(no_begin.best["len"][0, 1])) == (250, 50)


def test_two_identical_runs_the_earlier_wins(D):
    tc, tb = bio_table(2)
    m, path = random_case(600, tc, seed=6)
    path[100:104] = [4] * 4
    path[99], path[104] = 0, 0
    path[400:404] = [4] * 4
    path[399], path[404] = 0, 0
    m[400:404] = m[100:104]
    sel = torch.tensor([k for k, t in enumerate(path) if tc[t] == 2 and not (100 <= k < 104 or 400 <= k < 404)], dtype=torch.long)
    m[sel] = torch.tensor([0.6, 0.1, 0.1, 0.1, 0.1])                                  # every other run of class 2 scores 0.2
    m[100:104] = torch.tensor([0.05, 0.05, 0.05, 0.05, 0.8])
    m[400:404] = m[100:104]
    out = check(D, m, path, tc, tb, 3)
    assert (int(out.best["start"][0, 2]), int(out.best["len"][0, 2])) == (100, 4)


def test_threshold_in_double_and_a_class_without_a_record(D):
    tc, tb = bio_table(2)
    m, path = random_case(257, tc, seed=7)
    base = check(D, m, path, tc, tb, 3)
    score = base.score.cpu().numpy()
    j = int(np.nonzero(base.cls.cpu().numpy() != 0)[0][20])
    t = float(score[j])
    assert int(check(D, m, path, tc, tb, 3, thresh=t).cls[j]) != 0                    # score < t is false
    assert int(check(D, m, path, tc, tb, 3, thresh=float(np.nextafter(t, 2.0))).cls[j]) == 0
    check(D, m, path, tc, tb, 3, thresh=2.0)                                          # every row to class 0; begin tags still cut
    everything = check(D, m, path, tc, [0] * 5, 3, thresh=2.0)                        # no begin tags: one run, two empty classes
    assert everything.best["start"][0].tolist() == [0, -1, -1] and int(everything.best["len"][0, 0]) == 257


def test_64_tags_64_classes(D):
    tc, tb = list(range(64)), [k % 2 for k in range(64)]
    m, path = random_case(513, tc, seed=8, run_len=3)
    check(D, m, path, tc, tb, 64)
    check(D, m, path, tc, tb, 64, doc_off=[0, 1, 3, 258, 513], thresh=0.1)


def test_argument_errors(D):
    from vbg import ops
    from vbg.lib import VbgError
    tc, tb = bio_table(2)
    m, path = random_case(8, tc, seed=9)
    md, pd = m.to(dev()), torch.tensor(path, dtype=torch.int32, device=dev())
    with pytest.raises(VbgError):                                                     # class out of range
        ops.field_decode_tags(md, pd, [0, 1, 1, 3, 2], tb, 3)
    with pytest.raises(VbgError):
        ops.field_decode_tags(md, pd, [0, 1, 1, -1, 2], tb, 3)
    with pytest.raises(VbgError):                                                     # a begin flag that is no flag
        ops.field_decode_tags(md, pd, tc, [0, 2, 0, 1, 0], 3)
    with pytest.raises(VbgError):                                                     # more than 64 tags
        ops.field_decode_tags(torch.zeros(4, 65, device=dev()), pd[:4], [0] * 65, [0] * 65, 3)
    with pytest.raises(VbgError):                                                     # more than 64 classes
        ops.field_decode_tags(md, pd, tc, tb, 65)
    with pytest.raises(VbgError):                                                     # a table of another length
        ops.field_decode_tags(md, pd, tc[:4], tb[:4], 3)
    big = 1 << 20                                                                     # 2^20 rows in one document
    mb = torch.zeros(big, 2, device=dev())
    pb = torch.zeros(big, dtype=torch.int32, device=dev())
    with pytest.raises(VbgError):
        ops.field_decode_tags(mb, pb, [0, 0], [0, 0], 1)
    cls, score, best = ops.field_decode_tags(mb, pb, [0, 0], [0, 0], 1, doc_off=[0, big - 1, big])
    torch.cuda.synchronize()
    assert int(cls.max()) == 0
