"""vbg_field_decode on the device (csrc/decode.hip; vbg/decode.py): classes, scores, runs and the winner of every class from one
launch.  Needs a real MI355X.

Stage 1 is held EXACTLY to ops.row_softmax (bitwise score, first argmax) and to the fp64 restatement at test_row_softmax's tolerance
(1e-5 relative, 1e-6 absolute); stage 2 is held EXACTLY -- start, length and the bits of the fp64 mean -- to stage 2 of the restatement
(tests/decode_restate.py) fed the device's own classes and scores.  Shapes: every chunk edge of the 256-row walk (255 / 256 / 257 rows,
5000 rows as one run and as 5000 runs), the class counts 1, 2, 5 and the largest, 64, empty documents, documents cut inside a run."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import decode_restate as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode.npz")


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


def rnd(n, c, seed, scale=3.0):
    return torch.randn(n, c, generator=torch.Generator().manual_seed(seed)) * scale


def classed(classes, c, seed):
    """rows whose class is given: noise in [-0.5, 0.5), a level in [2, 6) on the row's class"""
    g = torch.Generator().manual_seed(seed)
    n = len(classes)
    x = torch.rand(n, c, generator=g) - 0.5
    x[torch.arange(n), torch.tensor(classes, dtype=torch.long)] = 2.0 + 4.0 * torch.rand(n, generator=g)
    return x


def bits64(v):
    return np.asarray(v, dtype=np.float64).view(np.int64)


def want_table(cls, score, off, c):
    """stage 2 of the restatement per document -> (start, len, mean) arrays [ndoc, C]"""
    nd = len(off) - 1
    start = np.full((nd, c), -1, dtype=np.int32)
    length = np.zeros((nd, c), dtype=np.int32)
    mean = np.zeros((nd, c), dtype=np.float64)
    for d in range(nd):
        for k, w in enumerate(R.stage2(cls[off[d]:off[d + 1]], score[off[d]:off[d + 1]], c)):
            if w is not None:
                start[d, k], length[d, k], mean[d, k] = w
    return start, length, mean


def check(ops, D, x, doc_off=None, thresh=None):
    """both stages on one input; -> the FieldDecode"""
    n, c = x.shape
    xd = x.to(dev())
    out = D.decode_fields(xd, thresh=thresh, doc_off=doc_off)
    off = [0, n] if doc_off is None else list(doc_off)
    lo, hi = off[0], off[-1]
    cls = out.cls.cpu().numpy()[lo:hi]
    score = out.score.cpu().numpy()[lo:hi]
    assert out.best.shape == (len(off) - 1, c) and out.cls.dtype == torch.int32 and out.score.dtype == torch.float32
    if hi > lo:
        # stage 1, exact: the probabilities of ops.row_softmax, their first maximum
        y = ops.row_softmax(xd).cpu().numpy()[lo:hi]
        first = y.argmax(1)
        rows = np.arange(hi - lo)
        assert np.array_equal(score.view(np.int32), y[rows, first].view(np.int32))
        keep = R.threshold(first.tolist(), score.tolist(), thresh)
        assert cls.tolist() == keep
        # stage 1 against fp64
        ref = np.array(R.stage1(x[lo:hi].tolist())[1])
        err = np.abs(score.astype(np.float64) - ref)
        print("stage 1: max |score - fp64|", float(err.max()), "rows", hi - lo, "classes", c)
        assert bool((err <= 1e-6 + 1e-5 * np.abs(ref)).all())
    # stage 2, exact
    start, length, mean = want_table(cls.tolist(), score.tolist(), [o - lo for o in off], c)
    assert np.array_equal(out.best["start"], start), (out.best["start"], start)
    assert np.array_equal(out.best["len"], length)
    assert np.array_equal(bits64(out.best["mean"]), bits64(mean))
    return out


@pytest.mark.parametrize("c", [1, 2, 5, 64])
@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257])
def test_random_rows(ops, D, n, c):
    out = check(ops, D, rnd(n, c, seed=100 * c + n))
    if n == 0:
        assert bool((out.best["start"] == -1).all())
    if n == 1:
        assert int(out.best["start"][0, c - 1]) == 0 and int((out.best["start"] >= 0).sum()) == 1      # filed under the last class


def test_one_long_run(ops, D):
    out = check(ops, D, classed([2] * 5000, 5, seed=1))
    assert out.best["start"][0].tolist() == [-1, -1, 0, -1, -1] and int(out.best["len"][0, 2]) == 5000


def test_every_segment_a_run(ops, D):
    out = check(ops, D, classed([1, 3] * 2500, 5, seed=2))
    assert int(out.best["len"].max()) == 1 and bool((out.best["start"][0, [1, 3]] >= 0).all())


def test_runs_of_mixed_length_across_chunks(ops, D):
    g = torch.Generator().manual_seed(3)
    classes = []
    while len(classes) < 1500:
        k = int(torch.randint(0, 5, (1,), generator=g))
        classes += [k] * int(torch.randint(1, 400, (1,), generator=g))
    check(ops, D, classed(classes[:1500], 5, seed=4))


def test_three_documents_the_middle_one_empty(ops, D):
    out = check(ops, D, rnd(300, 5, seed=5), doc_off=[0, 37, 37, 300])
    assert bool((out.best["start"][1] == -1).all()) and bool((out.best["len"][1] == 0).all())


def test_document_boundary_inside_a_run(ops, D):
    x = classed([2] * 300, 5, seed=6)
    out = check(ops, D, x, doc_off=[0, 130, 300])
    assert out.best["len"][:, 2].tolist() == [130, 170] and out.best["start"][:, 2].tolist() == [0, 0]
    out = check(ops, D, x, doc_off=[5, 130, 131, 300])                     # rows in front of the first document are not touched
    assert out.best["len"][:, 2].tolist() == [125, 0, 169] and int(out.best["len"][1, 4]) == 1       # one row: filed under class C - 1


def test_golden_strings(D):
    g = np.load(GOLDEN, allow_pickle=False)
    for name in g["names"]:
        x = torch.from_numpy(g[f"x_{name}"]).to(dev())
        texts = [str(t) for t in g[f"text_{name}"]]
        got = D.field_strings(x, x.shape[1], (texts,), join="concat")
        assert got[1:] == [str(s) for s in g[f"want_{name}"]], str(name)


def test_threshold_in_double(ops, D):
    x = rnd(257, 5, seed=7, scale=1.0)
    base = check(ops, D, x)
    cls0, score0 = base.cls.cpu().numpy(), base.score.cpu().numpy()
    j = int(np.nonzero(cls0 != 0)[0][100])
    t = float(score0[j])                                                   # the score as a double
    assert int(check(ops, D, x, thresh=t).cls[j]) == cls0[j]               # score < t is false: the row keeps its class
    up = math.nextafter(t, 1.0)
    assert np.float32(up) == score0[j]                                     # an fp32 comparison would still see equality
    assert int(check(ops, D, x, thresh=up).cls[j]) == 0
    zero = check(ops, D, x, thresh=0.0)
    assert torch.equal(zero.cls, base.cls) and torch.equal(zero.score, base.score)
    assert zero.best.tobytes() == base.best.tobytes()


def test_rows_with_nan_stay_inside_their_document(ops, D):
    x = rnd(600, 5, seed=8)
    x[17, 2] = float("nan")
    x[300] = float("nan")
    out = D.decode_fields(x.to(dev()), doc_off=[0, 400, 600])
    torch.cuda.synchronize()
    cls = out.cls.cpu().numpy()
    assert cls.min() >= 0 and cls.max() < 5
    clean = check(ops, D, x[400:])
    assert out.best[1].tobytes() == clean.best[0].tobytes()
