"""vbg_crf_posterior on the device (csrc/crf.hip; ops.crf_posterior): Viterbi path and score, log Z and the posterior marginals of every
row from one launch.  Needs a real MI355X.

The marginals are held to the fp64 restatement (tests/crf_posterior_restate.py, itself held to the reference CRF and to brute force in
tests/test_crf_posterior_host.py) at the tolerance test_crf_vs_oracle holds the same quantity to -- rtol 1e-4, atol 1e-6, on EVERY
entry -- at lengths where the unnormalised recursion of the gradient kernel no longer meets it (700 rows), and on inputs that
stretch the dynamic range (transitions x 8, emissions x 20, emissions + 50).  Path and score must be ops.crf_viterbi's bits."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import crf_posterior_restate as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "crf_posterior.npz")
ROW_SUM_TOL = 64 * 2.0 ** -23


@pytest.fixture(scope="module")
def ops():
    from vbg import ops as _ops
    return _ops


def dev():
    return torch.device("cuda")


def generated(ntag, lens, seed=None, trans_scale=1.0, em_scale=1.0, em_shift=0.0):
    g = torch.Generator().manual_seed(300 + ntag if seed is None else seed)
    em = torch.randn(sum(lens), ntag, generator=g) * em_scale + em_shift
    trans = torch.randn(ntag, ntag, generator=g) * 2 * trans_scale
    start, stop = ntag - 2, ntag - 1
    trans[start, :] = -10000
    trans[:, stop] = -10000
    return em, trans, start, stop


def offsets(lens):
    off = [0]
    for n in lens:
        off.append(off[-1] + n)
    return off


def run(ops, em, trans, start, stop, lens):
    d = dev()
    doc_off = torch.tensor(offsets(lens), dtype=torch.int32, device=d)
    emd, trd = em.to(d), trans.to(d)
    out = ops.crf_posterior(emd, doc_off, trd, start, stop)
    torch.cuda.synchronize()
    return out, (emd, doc_off, trd)


def check(ops, em, trans, start, stop, lens, want=None):
    """every check of the module docstring on one input; want: per document (logz, marginals) in fp64 (None: the restatement)"""
    (path, score, logz, marg), (emd, doc_off, trd) = run(ops, em, trans, start, stop, lens)
    N, ntag = em.shape
    off = offsets(lens)
    assert path.dtype == torch.int32 and tuple(path.shape) == (N,) and tuple(marg.shape) == (N, ntag)
    assert tuple(score.shape) == tuple(logz.shape) == (len(lens),)
    vpath, vscore = ops.crf_viterbi(emd, doc_off, trd, start, stop)
    assert torch.equal(path, vpath)
    assert torch.equal(score.view(torch.int32), vscore.view(torch.int32))
    m = marg.cpu().numpy().astype(np.float64)
    z = logz.cpu().numpy().astype(np.float64)
    assert not np.isnan(m).any() and not np.isnan(z).any()
    assert bool((m[:, [start, stop]] == 0).all())
    if N:
        sums = marg.cpu().numpy().astype(np.float64).sum(1)
        print("row sums: max |sum - 1|", float(np.abs(sums - 1).max()))
        assert float(np.abs(sums - 1).max()) <= ROW_SUM_TOL
    for k, n in enumerate(lens):
        wz, wm = want[k] if want is not None else R.forward_backward(em[off[k]:off[k + 1]].numpy(), trans.numpy(), start, stop)
        got = m[off[k]:off[k + 1]]
        if n:
            err = np.abs(got - wm)
            print(f"ntag {ntag} rows {n}: max |marginal - fp64| {float(err.max()):.3e}, largest share of the tolerance "
                  f"{float((err / (1e-6 + 1e-4 * np.abs(wm))).max()):.3f}, |logz - fp64| {abs(z[k] - wz):.3e}")
            assert bool((err <= 1e-6 + 1e-4 * np.abs(wm)).all())
        assert abs(z[k] - wz) <= 1e-5 + 1e-5 * abs(wz)
    return path, score, logz, marg


@pytest.mark.parametrize("ntag,lens", [(3, [4]), (7, [8, 7]), (14, [1, 30, 0, 5]), (64, [6, 9]), (25, [700]), (64, [700, 1])])
def test_generated(ops, ntag, lens):
    check(ops, *generated(ntag, lens), lens)


@pytest.mark.parametrize("name", ["t9_n15", "t27_n300", "t27_n700"])
def test_fixture(ops, name):
    g = np.load(GOLDEN, allow_pickle=False)
    em, trans = torch.from_numpy(g[f"em_{name}"]), torch.from_numpy(g[f"trans_{name}"])
    start, stop = (int(v) for v in g[f"ends_{name}"])
    path, _, _, _ = check(ops, em, trans, start, stop, [em.shape[0]], want=[(float(g[f"logz_{name}"]), g[f"marg_{name}"])])
    assert path.cpu().tolist() == g[f"path_{name}"].tolist()


@pytest.mark.parametrize("kw", [dict(trans_scale=8.0), dict(em_scale=20.0), dict(em_shift=50.0)], ids=["trans_x8", "em_x20", "em_plus50"])
def test_harsh_inputs(ops, kw):
    check(ops, *generated(25, [300], seed=900, **kw), [300])


def test_an_empty_document_touches_no_row_and_keeps_the_existing_values(ops):
    em, trans, start, stop = generated(14, [1, 30, 0, 5])
    (path, score, logz, marg), (emd, doc_off, trd) = run(ops, em, trans, start, stop, [1, 30, 0, 5])
    tags = torch.zeros(36, dtype=torch.int32, device=dev())
    _, _, z_nll = ops.crf_nll_fwd(emd, tags, doc_off, trd, start, stop)
    _, vscore = ops.crf_viterbi(emd, doc_off, trd, start, stop)
    assert int(logz.view(torch.int32)[2]) == int(z_nll.view(torch.int32)[2])
    assert int(score.view(torch.int32)[2]) == int(vscore.view(torch.int32)[2])
    # all documents empty but rows present in front: nothing is written
    off = torch.tensor([3, 3, 3], dtype=torch.int32, device=dev())
    p2, s2, z2, m2 = ops.crf_posterior(emd, off, trd, start, stop)
    assert float(z2[0]) == float(z2[1]) == float(logz[2])


def test_same_bits_twice_and_in_the_deterministic_mode(ops):
    em, trans, start, stop = generated(25, [300, 41], seed=77)
    first, _ = run(ops, em, trans, start, stop, [300, 41])
    second, _ = run(ops, em, trans, start, stop, [300, 41])
    ops.set_deterministic(True)
    try:
        third, _ = run(ops, em, trans, start, stop, [300, 41])
    finally:
        ops.set_deterministic(False)
    for other in (second, third):
        for a, b in zip(first, other):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_documents_do_not_see_each_other(ops):
    em, trans, start, stop = generated(25, [70, 129], seed=78)
    (path, score, logz, marg), _ = run(ops, em, trans, start, stop, [70, 129])
    (p2, s2, z2, m2), _ = run(ops, em[70:], trans, start, stop, [129])
    assert torch.equal(path[70:], p2) and torch.equal(marg[70:].view(torch.int32), m2.view(torch.int32))
    assert torch.equal(logz[1:].view(torch.int32), z2.view(torch.int32))


def test_argument_errors(ops):
    from vbg.lib import VbgError
    em, trans, start, stop = generated(7, [8])
    d = dev()
    off = torch.tensor([0, 8], dtype=torch.int32, device=d)
    for s, e in ((-1, stop), (start, 7), (7, stop)):
        with pytest.raises(VbgError):
            ops.crf_posterior(em.to(d), off, trans.to(d), s, e)
    with pytest.raises(VbgError):                                                     # more than 64 tags
        ops.crf_posterior(torch.zeros(4, 65, device=d), torch.tensor([0, 4], dtype=torch.int32, device=d), torch.zeros(65, 65, device=d), 63, 64)
    with pytest.raises(VbgError):                                                     # one tag
        ops.crf_posterior(torch.zeros(4, 1, device=d), torch.tensor([0, 4], dtype=torch.int32, device=d), torch.zeros(1, 1, device=d), 0, 0)
    with pytest.raises(VbgError):                                                     # transitions of another size
        ops.crf_posterior(em.to(d), off, torch.zeros(6, 6, device=d), start, stop)
