"""vbg_crf_path_logp on the device (csrc/crf.hip; ops.crf_path_logp): the log marginal and the log conditional of every row of a given
tag path, one launch.  Needs a real MI355X.

Held to the fp64 restatement (tests/crf_span_restate.py, itself held to brute force in tests/test_crf_span_host.py) at the tolerance
the project holds the posterior to: on EVERY row exp(lm) and exp(lc) within rtol 1e-4 / atol 1e-6.  Spans of the Viterbi path: the
sum's error within 1e-4 per row of the SPAN -- the per-row relative tolerance in the log domain; it grows with the span's length,
never with the document's.  Inputs are test_gpu_crf_posterior.py's, two paths each: the Viterbi path of ops.crf_posterior and a seeded
random path over the ordinary tags."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import crf_posterior_restate as R
import crf_span_restate as S
from test_gpu_crf_posterior import dev, generated, offsets

CASES = [(3, [4]), (7, [8, 7]), (14, [1, 30, 0, 5]), (64, [6, 9]), (25, [700]), (64, [700, 1])]
HARSH = {"trans_x8": dict(trans_scale=8.0), "em_x20": dict(em_scale=20.0), "em_plus50": dict(em_shift=50.0)}


@pytest.fixture(scope="module")
def ops():
    from vbg import ops as _ops
    return _ops


def ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


def plain_table(ntag):
    """SROIE style: tag k is class k, START / STOP class 0, no begin tags -- runs are cut where the class changes"""
    return [k if k < ntag - 2 else 0 for k in range(ntag)], [0] * ntag


def bio_table(ntag):
    """tag 0 "O", then B-1 I-1 B-2 I-2 ... over the ordinary tags; B- tags open a run"""
    tc, tb = [0] * ntag, [0] * ntag
    for k in range(1, ntag - 2):
        tc[k], tb[k] = (k + 1) // 2, k % 2
    return tc, tb


def random_path(ntag, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, max(ntag - 2, 1), (n,), generator=g, dtype=torch.int32)


def launch(ops, em, trans, start, stop, lens, path=None):
    """-> (lm, lc, path, posterior outputs), all on the device; path None: the Viterbi path"""
    d = dev()
    doc_off = torch.tensor(offsets(lens), dtype=torch.int32, device=d)
    emd, trd = em.to(d), trans.to(d)
    post = ops.crf_posterior(emd, doc_off, trd, start, stop)
    p = post[0] if path is None else path.to(d)
    lm, lc = ops.crf_path_logp(emd, doc_off, trd, start, stop, p)
    torch.cuda.synchronize()
    assert lm.dtype == lc.dtype == torch.float32 and tuple(lm.shape) == tuple(lc.shape) == (em.shape[0],)
    return lm, lc, p, post


def check(ops, em, trans, start, stop, lens, path=None, spans=True):
    """every row against the restatement, the marginals against the posterior's, the spans of the path under two tag tables and, for
    short documents, the whole path against score - log Z"""
    lm, lc, p, post = launch(ops, em, trans, start, stop, lens, path)
    ntag = em.shape[1]
    off = offsets(lens)
    glm, glc = lm.cpu().numpy().astype(np.float64), lc.cpu().numpy().astype(np.float64)
    y = p.cpu().tolist()
    marg = post[3].cpu().numpy().astype(np.float64)
    for k, n in enumerate(lens):
        if n == 0:
            continue
        lo, hi = off[k], off[k + 1]
        e64, t64 = em[lo:hi].numpy().astype(np.float64), trans.numpy().astype(np.float64)
        wlm, wlc = S.path_logp(e64, t64, start, stop, y[lo:hi])
        for name, got, want in (("lm", glm[lo:hi], wlm), ("lc", glc[lo:hi], wlc)):
            err = np.abs(np.exp(got) - np.exp(want))
            share = err / (1e-6 + 1e-4 * np.exp(want))
            print(f"ntag {ntag} rows {n} {name}: max |exp - fp64| {float(err.max()):.3e}, largest share of the tolerance "
                  f"{float(share.max()):.3f}, max log-domain error {float(np.abs(got - want)[np.isfinite(want)].max()):.3e}")
            assert not np.isnan(got).any()
            assert bool((share <= 1.0).all()), (name, int(share.argmax()))
        assert glc[lo] == glm[lo]                                                       # the first row's conditional is its marginal
        pm = marg[np.arange(lo, hi), y[lo:hi]]
        assert bool((np.abs(np.exp(glm[lo:hi]) - pm) <= 1e-6 + 1e-4 * pm).all())        # agreement with vbg_crf_posterior
        if spans:
            for tc, tb in (plain_table(ntag), bio_table(ntag)):
                cls = [tc[t] for t in y[lo:hi]]
                worst = 0.0
                for s, ln in R.runs(cls, [bool(tb[t]) for t in y[lo:hi]]):
                    got = float(glm[lo + s]) + float(np.sum(glc[lo + s + 1:lo + s + ln]))
                    err = abs(got - S.span_logp(wlm, wlc, s, s + ln - 1))
                    worst = max(worst, err / ln)
                    assert err <= 1e-4 * ln, (s, ln, err)
                print(f"ntag {ntag} rows {n}: worst span error per row {worst:.3e}")
        if n <= 30:
            score = R.path_score(e64, t64, start, stop, y[lo:hi])
            logz, _ = R.forward_backward(e64, t64, start, stop)
            whole = abs(float(np.sum(glc[lo:hi])) - (score - logz))
            print(f"ntag {ntag} rows {n}: |sum(lc) - (score - logz)| {whole:.3e}")
            assert whole <= n * 1e-4 + 4 * ulp32(max(abs(score), abs(logz)))
    return lm, lc


@pytest.mark.parametrize("ntag,lens", CASES)
def test_the_viterbi_path(ops, ntag, lens):
    check(ops, *generated(ntag, lens), lens)


@pytest.mark.parametrize("ntag,lens", CASES)
def test_a_random_path(ops, ntag, lens):
    check(ops, *generated(ntag, lens), lens, path=random_path(ntag, sum(lens), 500 + ntag), spans=False)


@pytest.mark.parametrize("name", list(HARSH))
def test_harsh_inputs(ops, name):
    em, trans, start, stop = generated(25, [300], seed=900, **HARSH[name])
    check(ops, em, trans, start, stop, [300])
    check(ops, em, trans, start, stop, [300], path=random_path(25, 300, 901), spans=False)


def test_an_empty_document_touches_no_row(ops):
    lens = [1, 30, 0, 5]
    em, trans, start, stop = generated(14, lens)
    lm, lc, p, _ = launch(ops, em, trans, start, stop, lens)
    d = dev()
    # documents over rows 3 .. 7 and 7 .. 12 with an empty one between them; the rows around keep what they held
    off = torch.tensor([3, 7, 7, 12], dtype=torch.int32, device=d)
    from vbg.lib import check as rc_check, lib
    from vbg.ops import P, _stream
    ws = torch.empty(36 * 14, device=d)
    out_m, out_c = torch.full((36,), 7.0, device=d), torch.full((36,), 9.0, device=d)
    rc_check(lib.vbg_crf_path_logp(P(em.to(d)), P(off), 3, P(trans.to(d)), 14, start, stop, P(p), P(ws), P(out_m), P(out_c), _stream()), "path_logp")
    torch.cuda.synchronize()
    assert bool((out_m[:3] == 7.0).all()) and bool((out_m[12:] == 7.0).all()) and bool((out_c[:3] == 9.0).all()) and bool((out_c[12:] == 9.0).all())
    assert bool((out_m[3:12] <= 0).all()) and bool((out_c[3:12] <= 0).all())
    # all documents empty, rows present in front: nothing is written
    off = torch.tensor([3, 3, 3], dtype=torch.int32, device=d)
    out_m.fill_(7.0)
    out_c.fill_(9.0)
    rc_check(lib.vbg_crf_path_logp(P(em.to(d)), P(off), 2, P(trans.to(d)), 14, start, stop, P(p), P(ws), P(out_m), P(out_c), _stream()), "path_logp")
    torch.cuda.synchronize()
    assert bool((out_m == 7.0).all()) and bool((out_c == 9.0).all())
    # no row at all through the wrapper
    e0 = torch.zeros(0, 14, device=d)
    lm0, lc0 = ops.crf_path_logp(e0, torch.tensor([0, 0], dtype=torch.int32, device=d), trans.to(d), start, stop, torch.zeros(0, dtype=torch.int32, device=d))
    assert tuple(lm0.shape) == tuple(lc0.shape) == (0,)


def test_same_bits_twice_and_in_the_deterministic_mode(ops):
    em, trans, start, stop = generated(25, [300, 41], seed=77)
    first = launch(ops, em, trans, start, stop, [300, 41])[:2]
    second = launch(ops, em, trans, start, stop, [300, 41])[:2]
    ops.set_deterministic(True)
    try:
        third = launch(ops, em, trans, start, stop, [300, 41])[:2]
    finally:
        ops.set_deterministic(False)
    for other in (second, third):
        for a, b in zip(first, other):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_documents_do_not_see_each_other(ops):
    em, trans, start, stop = generated(25, [70, 129], seed=78)
    path = random_path(25, 199, 79)
    lm, lc, _, _ = launch(ops, em, trans, start, stop, [70, 129], path=path)
    lm2, lc2, _, _ = launch(ops, em[70:], trans, start, stop, [129], path=path[70:])
    lm1, lc1, _, _ = launch(ops, em[:70], trans, start, stop, [70], path=path[:70])
    assert torch.equal(lm[70:].view(torch.int32), lm2.view(torch.int32)) and torch.equal(lc[70:].view(torch.int32), lc2.view(torch.int32))
    assert torch.equal(lm[:70].view(torch.int32), lm1.view(torch.int32)) and torch.equal(lc[:70].view(torch.int32), lc1.view(torch.int32))


@pytest.mark.parametrize("ntag", [7, 40])
def test_tags_out_of_range(ops, ntag):
    lens = [9, 4]
    em, trans, start, stop = generated(ntag, lens, seed=80)
    good = random_path(ntag, 13, 81)
    bad = good.clone()
    bad[3], bad[6] = -1, ntag
    bad[8] = 1 << 30                                                                    # the document's last row: the next document is not touched
    lm, lc, _, _ = launch(ops, em, trans, start, stop, lens, path=good)
    bm, bc, _, _ = launch(ops, em, trans, start, stop, lens, path=bad)
    neg = float("-inf")
    for r in (3, 6, 8):
        assert float(bm[r]) == neg and float(bc[r]) == neg
    for r in (4, 7):
        assert float(bc[r]) == neg                                                      # the row behind a tag out of range, in its document
    keep_m = [r for r in range(13) if r not in (3, 6, 8)]
    keep_c = [r for r in range(13) if r not in (3, 4, 6, 7, 8)]
    assert torch.equal(bm[keep_m].view(torch.int32), lm[keep_m].view(torch.int32))
    assert torch.equal(bc[keep_c].view(torch.int32), lc[keep_c].view(torch.int32))


def test_start_and_stop_in_the_path_are_legal(ops):
    em, trans, start, stop = generated(7, [6], seed=82)
    path = torch.tensor([0, start, 1, stop, 2, 3], dtype=torch.int32)
    lm, lc, _, _ = launch(ops, em, trans, start, stop, [6], path=path)
    assert bool(torch.isfinite(lm).all()) and bool(torch.isfinite(lc).all())
    # into START costs -10000, and so does leaving STOP, which the backward vector of the STOP row carries
    assert float(lm[1]) < -9000 and float(lm[3]) < -9000 and float(lc[1]) < -9000 and float(lc[3]) < -9000
    assert float(lm[0]) > -100 and float(lm[5]) > -100


def test_shape_and_dtype_errors(ops):
    from vbg.lib import VbgError
    em, trans, start, stop = generated(7, [8])
    d = dev()
    emd, trd = em.to(d), trans.to(d)
    off = torch.tensor([0, 8], dtype=torch.int32, device=d)
    path = torch.zeros(8, dtype=torch.int32, device=d)
    for s, e in ((-1, stop), (start, 7), (7, stop)):
        with pytest.raises(VbgError):
            ops.crf_path_logp(emd, off, trd, s, e, path)
    with pytest.raises(VbgError):                                                     # more than 64 tags
        ops.crf_path_logp(torch.zeros(4, 65, device=d), torch.tensor([0, 4], dtype=torch.int32, device=d), torch.zeros(65, 65, device=d), 63, 64, path[:4])
    with pytest.raises(VbgError):                                                     # transitions of another size
        ops.crf_path_logp(emd, off, torch.zeros(6, 6, device=d), start, stop, path)
    with pytest.raises(VbgError):                                                     # 64-bit row ranges
        ops.crf_path_logp(emd, off.long(), trd, start, stop, path)
    with pytest.raises(VbgError):                                                     # a path of another type, length, device
        ops.crf_path_logp(emd, off, trd, start, stop, path.long())
    with pytest.raises(VbgError):
        ops.crf_path_logp(emd, off, trd, start, stop, path[:7])
    with pytest.raises(VbgError):
        ops.crf_path_logp(emd, off, trd, start, stop, path.cpu())
