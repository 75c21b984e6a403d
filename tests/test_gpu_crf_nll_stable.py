"""vbg_crf_nll_stable / vbg_crf_nll_stable_bwd on the device (csrc/crf.hip; ops.crf_nll_stable, Fn.CrfNllStableFn): the crf mode's
training loss with a gradient that holds at any length.  Needs a real MI355X.

Every launch is called with gout[d] = n_d, so what is compared are marginal-scale quantities: marginals less gold indicators.  Both
gradients are held, on EVERY entry, to the fp64 restatement (tests/crf_nll_restate.py, itself held to brute force and to the reference
CRF in tests/test_crf_nll_stable_host.py) at test_crf_vs_oracle's figures -- rtol 1e-4, atol 1e-6 -- applied at that scale: n_d times
stricter in absolute terms than test_crf_vs_oracle, at 300 and 700 rows where vbg_crf_nll_bwd's unnormalised vectors no longer meet
them, and on inputs that stretch the dynamic range (transitions x 8, emissions x 20, emissions + 50)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import crf_nll_restate as R
from test_gpu_crf_posterior import ROW_SUM_TOL, generated, offsets

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "crf_nll.npz")
GOLDEN_POST = os.path.join(HERE, "golden", "crf_posterior.npz")


@pytest.fixture(scope="module")
def ops():
    from vbg import ops as _ops
    return _ops


def dev():
    return torch.device("cuda")


def draw_tags(ntag, N, seed):
    g = torch.Generator().manual_seed(5000 + seed)
    return torch.randint(0, max(ntag - 2, 1), (N,), generator=g).int()


def bits(t):
    return t.contiguous().view(torch.int32)


def launch(ops, em, tags, trans, start, stop, lens, want_grad=True):
    """-> (nll, logz, dem_unit, dtrans_unit) and the device operands"""
    d = dev()
    doc_off = torch.tensor(offsets(lens), dtype=torch.int32, device=d)
    emd, tgd, trd = em.to(d), tags.to(d), trans.to(d)
    out = ops.crf_nll_stable(emd, tgd, doc_off, trd, start, stop, want_grad)
    torch.cuda.synchronize()
    return out, (emd, tgd, doc_off, trd)


def backward(ops, du, tu, doc_off, gout, dtrans=None):
    dtrans = torch.zeros(tu.shape[1:], device=du.device) if dtrans is None else dtrans
    dem = ops.crf_nll_stable_bwd(du, tu, doc_off, gout, dtrans)
    torch.cuda.synchronize()
    return dem, dtrans


def check(ops, em, tags, trans, start, stop, lens, want=None):
    """every check of the module docstring on one input; want: per document (nll, logz, dem_unit, dtrans_unit) in fp64 (None: the
    restatement).  -> the largest share of the gradient tolerance used"""
    (nll, logz, du, tu), (emd, tgd, doc_off, trd) = launch(ops, em, tags, trans, start, stop, lens)
    N, ntag = em.shape
    off = offsets(lens)
    assert tuple(nll.shape) == tuple(logz.shape) == (len(lens),) and tuple(du.shape) == (N, ntag) and tuple(tu.shape) == (len(lens), ntag, ntag)
    gout = torch.tensor([float(n) for n in lens], device=dev())
    dem, dtrans = backward(ops, du, tu, doc_off, gout)
    rows = torch.cat([torch.arange(off[k], off[k + 1]) for k in range(len(lens))]) if N else torch.zeros(0, dtype=torch.long)
    assert torch.equal(bits(dem.cpu()[rows]), bits(du.cpu()[rows]))                   # gout[d] / n_d == 1: the table itself
    u, tr_u = du.cpu().numpy().astype(np.float64), tu.cpu().numpy().astype(np.float64)
    z, l = logz.cpu().numpy().astype(np.float64), nll.cpu().numpy().astype(np.float64)
    assert not np.isnan(u[rows.numpy()]).any() and not np.isnan(tr_u).any() and not np.isnan(z).any() and not np.isnan(l).any()
    share = 0.0
    total = np.zeros((ntag, ntag))
    for k, n in enumerate(lens):
        sl = slice(off[k], off[k + 1])
        wl, wz, wu, wt = want[k] if want is not None else R.nll_and_grads(em[sl].numpy(), tags[sl].numpy(), trans.numpy(), start, stop)
        total += tr_u[k]
        if n:
            got = u[sl]
            assert bool((got[:, [start, stop]] == 0).all())
            ind = np.zeros((n, ntag))
            ind[np.arange(n), tags[sl].numpy()] = 1.0
            sums = (got + ind).sum(1)
            e_em, e_tr = np.abs(got - wu), np.abs(tr_u[k] - wt)
            s_em, s_tr = float((e_em / (1e-6 + 1e-4 * np.abs(wu))).max()), float((e_tr / (1e-6 + 1e-4 * np.abs(wt))).max())
            share = max(share, s_em, s_tr)
            print(f"ntag {ntag} rows {n}: largest share of the tolerance, emissions {s_em:.3f} (max err {float(e_em.max()):.3e}), transitions "
                  f"{s_tr:.3f} (max err {float(e_tr.max()):.3e}); max |row sum - 1| {float(np.abs(sums - 1).max()):.3e}; "
                  f"|nll - fp64| {abs(l[k] - wl):.3e}, |logz - fp64| {abs(z[k] - wz):.3e}")
            assert float(np.abs(sums - 1).max()) <= ROW_SUM_TOL
            assert bool((e_em <= 1e-6 + 1e-4 * np.abs(wu)).all())
            assert bool((e_tr <= 1e-6 + 1e-4 * np.abs(wt)).all())
        else:
            assert l[k] == 0.0 and not tr_u[k].any()
        assert abs(l[k] - wl) <= 1e-5 + 1e-5 * abs(wl)
        assert abs(z[k] - wz) <= 1e-5 + 1e-5 * abs(wz)
    if len([n for n in lens if n]) == 1:                                              # one document: dtrans is its block
        assert np.array_equal(dtrans.cpu().numpy().astype(np.float64), total)
    return share


@pytest.mark.parametrize("ntag,lens", [(3, [4]), (7, [8, 7]), (14, [1, 30, 0, 5]), (33, [5]), (64, [6, 9]), (25, [700]), (64, [700, 1])])
def test_generated(ops, ntag, lens):
    em, trans, start, stop = generated(ntag, lens)
    check(ops, em, draw_tags(ntag, sum(lens), ntag), trans, start, stop, lens)


@pytest.mark.parametrize("name", ["t9_n15", "t27_n300", "t27_n700"])
def test_fixture(ops, name):
    g, gp = np.load(GOLDEN, allow_pickle=False), np.load(GOLDEN_POST, allow_pickle=False)
    assert np.array_equal(g[f"em_{name}"], gp[f"em_{name}"]) and np.array_equal(g[f"trans_{name}"], gp[f"trans_{name}"])
    em, trans, tags = torch.from_numpy(g[f"em_{name}"]), torch.from_numpy(g[f"trans_{name}"]), torch.from_numpy(g[f"tags_{name}"])
    start, stop = (int(v) for v in g[f"ends_{name}"])
    n = em.shape[0]
    want = [(float(g[f"nll_{name}"]), float(gp[f"logz_{name}"]), n * g[f"dem_{name}"], n * g[f"dtrans_{name}"])]
    check(ops, em, tags, trans, start, stop, [n], want=want)


@pytest.mark.parametrize("kw", [dict(trans_scale=8.0), dict(em_scale=20.0), dict(em_shift=50.0)], ids=["trans_x8", "em_x20", "em_plus50"])
def test_harsh_inputs(ops, kw):
    em, trans, start, stop = generated(25, [300], seed=900, **kw)
    check(ops, em, draw_tags(25, 300, 900), trans, start, stop, [300])


def fn_grads(fn, em, tags, trans, start, stop, lens, w):
    d = dev()
    emd, trd = em.to(d).requires_grad_(True), trans.to(d).requires_grad_(True)
    doc_off = torch.tensor(offsets(lens), dtype=torch.int32, device=d)
    nll = fn.apply(emd, trd, tags.to(d), doc_off, start, stop)
    (nll * w.to(d)).sum().backward()
    torch.cuda.synchronize()
    return nll.detach().cpu(), emd.grad.cpu(), trd.grad.cpu()


@pytest.mark.parametrize("ntag,lens", [(7, [8, 7]), (14, [1, 30, 0, 5]), (25, [300, 41])])
def test_random_gout_through_the_autograd_function(ops, ntag, lens):
    from vbg import functions as Fn
    em, trans, start, stop = generated(ntag, lens, seed=410 + ntag)
    tags = draw_tags(ntag, sum(lens), 410 + ntag)
    w = torch.randn(len(lens), generator=torch.Generator().manual_seed(411 + ntag))
    nll, gem, gtr = fn_grads(Fn.CrfNllStableFn, em, tags, trans, start, stop, lens, w)
    off = offsets(lens)
    wem, wtr, wnll = np.zeros(tuple(em.shape)), np.zeros((ntag, ntag)), np.zeros(len(lens))
    for k, n in enumerate(lens):
        if n == 0:
            continue
        sl = slice(off[k], off[k + 1])
        wnll[k], _, u, t = R.nll_and_grads(em[sl].numpy(), tags[sl].numpy(), trans.numpy(), start, stop)
        wem[sl] = float(w[k]) / n * u
        wtr += float(w[k]) / n * t
    assert np.allclose(nll.numpy().astype(np.float64), wnll, rtol=1e-5, atol=1e-5)
    assert np.allclose(gem.numpy().astype(np.float64), wem, rtol=1e-4, atol=1e-6)
    assert np.allclose(gtr.numpy().astype(np.float64), wtr, rtol=1e-4, atol=2e-6)


@pytest.mark.parametrize("ntag,lens", [(7, [8, 7]), (14, [1, 30, 0, 5])])
def test_against_the_default_route_at_short_lengths(ops, ntag, lens):
    """both routes lie within test_crf_vs_oracle's tolerances of fp64 at these lengths, so within twice those of each other"""
    from vbg import functions as Fn
    em, trans, start, stop = generated(ntag, lens)
    tags = draw_tags(ntag, sum(lens), ntag)
    w = torch.randn(len(lens), generator=torch.Generator().manual_seed(420 + ntag))
    a = fn_grads(Fn.CrfNllStableFn, em, tags, trans, start, stop, lens, w)
    b = fn_grads(Fn.CrfNllFn, em, tags, trans, start, stop, lens, w)
    assert torch.allclose(a[0], b[0], rtol=2e-5, atol=2e-5)
    assert torch.allclose(a[1], b[1], rtol=2e-4, atol=2e-6)
    assert torch.allclose(a[2], b[2], rtol=2e-4, atol=4e-6)


def test_same_bits_twice_and_in_the_deterministic_mode(ops):
    lens = [300, 41]
    em, trans, start, stop = generated(25, lens, seed=77)
    tags = draw_tags(25, sum(lens), 77)
    gout = torch.tensor([0.7, -1.3], device=dev())

    def both():
        out, (_, _, doc_off, _) = launch(ops, em, tags, trans, start, stop, lens)
        return list(out) + list(backward(ops, out[2], out[3], doc_off, gout))

    first, second = both(), both()
    ops.set_deterministic(True)
    try:
        third = both()
    finally:
        ops.set_deterministic(False)
    for other in (second, third):
        for a, b in zip(first, other):
            assert torch.equal(bits(a), bits(b))


def test_documents_do_not_see_each_other(ops):
    lens = [70, 129]
    em, trans, start, stop = generated(25, lens, seed=78)
    tags = draw_tags(25, sum(lens), 78)
    (nll, logz, du, tu), _ = launch(ops, em, tags, trans, start, stop, lens)
    for k, (lo, hi) in enumerate([(0, 70), (70, 199)]):
        (n1, z1, du1, tu1), _ = launch(ops, em[lo:hi], tags[lo:hi], trans, start, stop, [hi - lo])
        assert torch.equal(bits(nll[k:k + 1]), bits(n1)) and torch.equal(bits(logz[k:k + 1]), bits(z1))
        assert torch.equal(bits(du[lo:hi]), bits(du1)) and torch.equal(bits(tu[k]), bits(tu1[0]))


def test_dtrans_is_the_ordered_sum_of_the_scaled_blocks(ops):
    lens = [9, 0, 33, 1, 12]
    em, trans, start, stop = generated(14, lens, seed=79)
    tags = draw_tags(14, sum(lens), 79)
    (_, _, du, tu), (_, _, doc_off, _) = launch(ops, em, tags, trans, start, stop, lens)
    g = torch.Generator().manual_seed(80)
    gout = torch.randn(len(lens), generator=g)
    before = torch.randn(14, 14, generator=g)
    dem, dtrans = backward(ops, du, tu, doc_off, gout.to(dev()), before.to(dev()))
    want, off = before.clone(), offsets(lens)
    duc, tuc = du.cpu(), tu.cpu()
    for k, n in enumerate(lens):
        if n == 0:
            continue
        scale = gout[k] / torch.tensor(float(n))                                      # fp32, as the kernel divides
        want = want + scale * tuc[k]                                                  # product rounded, then the sum: no fused multiply-add
        assert torch.equal(bits(dem.cpu()[off[k]:off[k + 1]]), bits(scale * duc[off[k]:off[k + 1]]))
    assert torch.equal(bits(dtrans.cpu()), bits(want))


def test_an_empty_document_touches_no_row_and_its_block_is_zeros(ops):
    from vbg.lib import check as rc_check, lib
    lens = [5, 0, 4]
    em, trans, start, stop = generated(14, lens, seed=81)
    tags = draw_tags(14, 9, 81)
    (nll, logz, du, tu), (emd, tgd, doc_off, trd) = launch(ops, em, tags, trans, start, stop, lens)
    assert float(nll[1]) == 0.0 and not bool(tu[1].any())
    _, _, z_fwd = ops.crf_nll_fwd(emd, tgd, doc_off, trd, start, stop)
    assert torch.equal(bits(logz[1:2]), bits(z_fwd[1:2]))
    # all documents empty with rows present: the tables' rows keep what they held, in the forward launch and in the backward one
    off = torch.tensor([3, 3, 3], dtype=torch.int32, device=dev())
    du2, tu2 = torch.full_like(du, 7.0), torch.full((2, 14, 14), 7.0, device=dev())
    n2, z2 = torch.full((2,), 7.0, device=dev()), torch.full((2,), 7.0, device=dev())
    P = ops.P
    rc_check(lib.vbg_crf_nll_stable(P(emd), P(tgd), P(off), 2, P(trd), 14, start, stop, P(n2), P(z2), P(du2), P(tu2), None), "vbg_crf_nll_stable")
    torch.cuda.synchronize()
    assert bool((du2 == 7.0).all()) and not bool(tu2.any()) and not bool(n2.any())
    assert torch.equal(bits(z2), bits(z_fwd[1:2].repeat(2)))
    dem2, dtr2 = torch.full_like(du, 5.0), torch.full((14, 14), 5.0, device=dev())
    rc_check(lib.vbg_crf_nll_stable_bwd(P(du2), P(tu2), P(off), 2, 14, P(torch.ones(2, device=dev())), P(dem2), P(dtr2), None), "vbg_crf_nll_stable_bwd")
    torch.cuda.synchronize()
    assert bool((dem2 == 5.0).all()) and bool((dtr2 == 5.0).all())


def test_a_loss_only_call_gives_the_same_bits(ops):
    from vbg import functions as Fn
    lens = [41, 0, 130]
    em, trans, start, stop = generated(25, lens, seed=82)
    tags = draw_tags(25, sum(lens), 82)
    (nll, logz, du, tu), (emd, tgd, doc_off, trd) = launch(ops, em, tags, trans, start, stop, lens)
    (nll0, logz0, du0, tu0), _ = launch(ops, em, tags, trans, start, stop, lens, want_grad=False)
    assert du0 is None and tu0 is None
    assert torch.equal(bits(nll), bits(nll0)) and torch.equal(bits(logz), bits(logz0))
    out = Fn.CrfNllStableFn.apply(emd, trd, tgd, doc_off, start, stop)               # no input requires a gradient: no tables
    assert not out.requires_grad and torch.equal(bits(out), bits(nll))


def test_a_second_backward_gives_the_same_bits(ops):
    from vbg import functions as Fn
    lens = [41, 130]
    em, trans, start, stop = generated(25, lens, seed=83)
    tags = draw_tags(25, sum(lens), 83)
    d = dev()
    emd, trd = em.to(d).requires_grad_(True), trans.to(d).requires_grad_(True)
    doc_off = torch.tensor(offsets(lens), dtype=torch.int32, device=d)
    loss = (Fn.CrfNllStableFn.apply(emd, trd, tags.to(d), doc_off, start, stop) * torch.tensor([0.3, 1.7], device=d)).sum()
    loss.backward(retain_graph=True)
    first = (emd.grad.clone(), trd.grad.clone())
    emd.grad, trd.grad = None, None
    loss.backward()
    assert torch.equal(bits(first[0]), bits(emd.grad)) and torch.equal(bits(first[1]), bits(trd.grad))


def test_tags_outside_the_range_index_nothing(ops):
    """include/vbg.h: such a row contributes no indicator and no emission term, the gold transitions into and out of it are skipped;
    the document's result means nothing, its neighbour's is untouched"""
    lens = [6, 9]
    em, trans, start, stop = generated(14, lens, seed=84)
    tags = draw_tags(14, sum(lens), 84)
    bad = tags.clone()
    bad[0], bad[2], bad[3], bad[5] = -1, 14, 2 ** 31 - 1, -2 ** 31                   # first and last row of document 0 among them
    (nll, logz, du, tu), _ = launch(ops, em, bad, trans, start, stop, lens)
    (nll1, logz1, du1, tu1), _ = launch(ops, em[6:], tags[6:], trans, start, stop, [9])
    assert torch.equal(bits(nll[1:]), bits(nll1)) and torch.equal(bits(du[6:]), bits(du1)) and torch.equal(bits(tu[1]), bits(tu1[0]))
    (_, logz0, du0, tu0), _ = launch(ops, em[:6], tags[:6], trans, start, stop, [6])
    assert torch.equal(bits(logz[:1]), bits(logz0))                                   # log Z does not read the tags
    assert bool(torch.isfinite(nll).all()) and bool(torch.isfinite(du).all()) and bool(torch.isfinite(tu).all())
    rows = du.cpu().double()
    for r in (0, 2, 3, 5):                                                            # no indicator: the row is the marginals, which sum to 1
        assert abs(float(rows[r].sum()) - 1.0) <= ROW_SUM_TOL
    for r in (1, 4):                                                                  # a row with its tag in range: the same bits as without the bad rows
        assert torch.equal(bits(du[r]), bits(du0[r]))
    # each of document 0's seven gold transitions (START -> row 0, ..., row 5 -> STOP) touches a bad row: none is taken off the six
    # tables and the terminal marginals, which sum to 1 each
    assert abs(float(tu[0].double().sum()) - 7.0) <= 7 * ROW_SUM_TOL


def test_argument_errors(ops):
    from vbg.lib import VbgError
    em, trans, start, stop = generated(7, [8])
    d = dev()
    off = torch.tensor([0, 8], dtype=torch.int32, device=d)
    tags = torch.zeros(8, dtype=torch.int32, device=d)
    for s, e in ((-1, stop), (start, 7), (7, stop)):
        with pytest.raises(VbgError):
            ops.crf_nll_stable(em.to(d), tags, off, trans.to(d), s, e, True)
    with pytest.raises(VbgError):                                                     # more than 64 tags
        ops.crf_nll_stable(torch.zeros(8, 65, device=d), tags, off, torch.zeros(65, 65, device=d), 63, 64, True)
    with pytest.raises(VbgError):                                                     # transitions of another size
        ops.crf_nll_stable(em.to(d), tags, off, torch.zeros(6, 6, device=d), start, stop, True)
    with pytest.raises(VbgError):                                                     # int64 tags
        ops.crf_nll_stable(em.to(d), tags.long(), off, trans.to(d), start, stop, True)
    with pytest.raises(VbgError):                                                     # int64 row ranges
        ops.crf_nll_stable(em.to(d), tags, off.long(), trans.to(d), start, stop, True)
