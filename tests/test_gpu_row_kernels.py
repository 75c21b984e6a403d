"""The encoder's row kernels (csrc/rowops.hip embed_ln_*, dropout_add_ln_fwd, the three dropout_add_ln_bwd forms; csrc/attn.hip
attn_mask*) against the fp64 restatements of tests/row_restate.py, at the shapes where they change path.

Tolerances are measured, never fixed: for every compared quantity the yardstick E_ref is the error of torch's CPU fp32 statement of the
same operation (F.layer_norm / native_layer_norm with autograd, index_add_ for the tables; for the backward fed with a given (xhat,
rstd), the same formula in fp32 tensor operations) against the fp64 reference ON THE SAME fp32 INPUTS, and the kernel's gate is
max(4 E_ref, 8 * 2^-24) in the same metric -- the factor 4 because the kernel's summation order (wave butterfly, rows in registers,
block fold) differs from torch's; both are fp32 sums of the same terms.  Metrics (row_restate.row_err / col_err): row tensors by max
|error| of a row over max |reference| of that row; column sums by |error| over the sum of |term| of the column, the starting value the
kernel accumulates into counting as one term.  Every figure is printed (`ROWEDGE ...`) before it is asserted; the figures measured on an
MI355X are in profiles/row_kernel_edges.txt.

Measured on an MI355X -- the largest figure over the cases of each family, each column maximised on its own (every single figure with
its case: profiles/row_kernel_edges.txt; 1416 figures, the largest kernel / gate ratio of any one of them is 0.83, dtype0 of one token
of 1000 columns):
    family              quantity                 E_ref     gate      kernel
    add-LN forward      y                        5.0e-6    2.0e-5    5.8e-6
                        xhat                     4.6e-6    1.8e-5    4.6e-6
                        rstd                     7.5e-7    3.0e-6    2.3e-7
    backward, isolated  dx, dres                 2.1e-7    8.4e-7    1.9e-7
                        dgamma, dbeta            1.7e-7    6.9e-7    1.5e-7
                        dbias                    2.6e-7    1.0e-6    1.6e-7
    backward, chained   dx, dres                 4.3e-6    1.7e-5    1.3e-6
                        dgamma                   7.3e-5    2.9e-4    1.5e-4    (1, 2, 7 rows: xhat's error of a row with |mean| / std
                        dbeta                    1.4e-7    5.6e-7    1.5e-7     ~ 100 in columns of that few terms; 8e-7 from 509 rows on)
                        dbias                    5.9e-6    2.4e-5    1.9e-6
    embedding           out, xhat                6.9e-7    2.8e-6    5.3e-7
                        rstd                     2.6e-7    1.0e-6    1.3e-7
                        dword, dpos              6.6e-6    2.6e-5    3.7e-6
                        dtype0, dgamma, dbeta    3.6e-7    1.4e-6    4.0e-7
The three backward forms give the same figures (their column sums are the same sums); the deterministic route of the embedding backward
gives those of torch's index_add_ where one table row takes every token (the same order of additions).

Dropout is pinned bit for bit: the realised keep pattern of both LayerNorm families must equal row_restate.keep_mask (element (t, c)
draws index t * hidden + c), and every value test under dropout uses the PREDICTED mask, with inf planted in x wherever it drops.
The attention mask words are compared bit for bit with row_restate.attn_mask_words on every word the kernel defines.

`wrows` (rows per wave of the backward kernel) is selected by the row count alone -- VBG_LN_WROWS is read once per process, so no test
sets it and the wrows cases skip when it is set.  vbg_ln_bwd_ws_rows(rows) = ceil(rows / (4 wrows)) proves the wrows of the forms that
use the partials workspace.  Below 512 rows that is wrows = 1 for the plane and pair forms (they always use the workspace), while the
fp32 form takes the atomic route without a workspace, whose wrows = 2 is a constant of the entry point that vbg_ln_bwd_ws_rows does
not report: there the dispatch log proves the route."""
import functools
import math
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import row_restate as R

pytestmark = pytest.mark.gpu

f64 = torch.float64
EPS = 1e-12


@pytest.fixture(scope="module")
def ops():
    from vbg import ops as _ops
    return _ops


def dev():
    return torch.device("cuda")


def _rec(fails, case, qty, e_ref, err):
    g = R.gate(e_ref)
    ok = err <= g
    print(f"ROWEDGE {case} {qty} E_ref={e_ref:.3e} gate={g:.3e} kernel={err:.3e} {'ok' if ok else 'FAIL'}")
    if not ok:
        fails.append((case, qty, e_ref, g, err))
    return ok


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------------------------------
# inputs and references of the add-LayerNorm family
# ---------------------------------------------------------------------------------------------------------------------------------------
def _hard_rows(g, rows, hid):
    """rows of scale 2^U{-4..4} around a mean of 30 N(0, 1) standard deviations: |mean| / std reaches ~100"""
    s = torch.exp2(torch.randint(-4, 5, (rows, 1), generator=g).float())
    m = 30.0 * torch.randn(rows, 1, generator=g)
    return (s * (torch.randn(rows, hid, generator=g) + m)).contiguous()


@functools.lru_cache(maxsize=6)
def _ln_case(rows, hid, p, seed=5, sid=3):
    g = torch.Generator().manual_seed(100003 * hid + 17 * rows + int(1000 * p))
    c = types.SimpleNamespace(rows=rows, hid=hid, p=p, seed=seed, sid=sid)
    c.x, c.res = _hard_rows(g, rows, hid), _hard_rows(g, rows, hid)
    c.gam, c.bet = 1 + 0.2 * torch.randn(hid, generator=g), 0.1 * torch.randn(hid, generator=g)
    c.dy = (torch.randn(rows, hid, generator=g) * torch.exp2(torch.randint(-4, 5, (rows, 1), generator=g).float())).contiguous()
    c.start = {k: torch.randn(hid, generator=g) for k in ("dgamma", "dbeta", "dbias")}
    c.keep = R.keep_mask(seed, sid, rows, hid, p) if p > 0 else None
    c.y64, c.xh64, c.rs64 = R.ln_fwd(c.x, c.res, c.gam, c.bet, EPS, c.keep, p)
    # the yardstick: torch fp32 on the same inputs (the dropped positions contribute nothing; kept ones are scaled, then the residual added)
    z32 = R._drop(c.x, c.keep, p) + c.res
    c.y32, mean32, c.rs32 = torch.native_layer_norm(z32, (hid,), c.gam, c.bet, EPS)
    c.xh32 = (z32 - mean32) * c.rs32
    c.rs32 = c.rs32.reshape(-1)
    # x as the kernel gets it: inf wherever the predicted mask drops
    c.xp = c.x.clone()
    if c.keep is not None:
        c.xp[torch.from_numpy(~c.keep)] = float("inf")
    return c


def _bwd32(dy, xhat, rstd, gam, keep, p):
    """the backward formula in fp32 tensor operations: the yardstick of the runs that are fed a given (xhat, rstd)"""
    gg = dy * gam
    m1, m2 = gg.mean(1, keepdim=True), (gg * xhat).mean(1, keepdim=True)
    dz = rstd[:, None] * (gg - m1 - xhat * m2)
    dx = R._drop(dz, keep, p)
    return dict(dz=dz, dx=dx, dgamma=(dy * xhat).sum(0), dbeta=dy.sum(0), dbias=dx.sum(0))


def _with_start(c, r, dtype):
    """the column quantities as the kernels leave them: added into the starting values (one more term of each column)"""
    for k in ("dgamma", "dbeta", "dbias"):
        r[k] = c.start[k].to(dtype) + r[k]
        if "a_" + k in r:
            r["a_" + k] = c.start[k].to(dtype).abs() + r["a_" + k]
    return r


def _autograd(c, dtype):
    x, res = c.x.to(dtype).requires_grad_(True), c.res.to(dtype).requires_grad_(True)
    gam, bet = c.gam.to(dtype).requires_grad_(True), c.bet.to(dtype).requires_grad_(True)
    y = F.layer_norm(R._drop(x, c.keep, c.p) + res, (c.hid,), gam, bet, EPS)
    y.backward(c.dy.to(dtype))
    return dict(dz=res.grad, dx=x.grad, dgamma=gam.grad, dbeta=bet.grad, dbias=x.grad.sum(0))


def _bwd_refs(c, mode):
    """-> (xhat, rstd to feed or None, fp64 reference, fp32 yardstick)"""
    if mode == "isolated":
        xh, rs = c.xh64.float(), c.rs64.float()
        ref = R.ln_bwd(c.dy, xh, rs, c.gam, c.keep, c.p)
        yard = _bwd32(c.dy, xh, rs, c.gam, c.keep, c.p)
        return xh, rs, _with_start(c, ref, f64), _with_start(c, yard, torch.float32)
    ref = _autograd(c, f64)
    asum = R.ln_bwd(c.dy, c.xh64, c.rs64, c.gam, c.keep, c.p)
    ref.update({k: v for k, v in asum.items() if k.startswith("a_")})
    return None, None, _with_start(c, ref, f64), _with_start(c, _autograd(c, torch.float32), torch.float32)


# rows -> wrows of the forms that use the partials workspace (see the module docstring for rows < 512)
WROWS = {1: 1, 2: 1, 7: 1, 509: 1, 512: 1, 515: 1, 1037: 1, 2048: 2, 2051: 2, 3075: 3, 8197: 8, 9300: 8}
BWD_CASES = [(r, 256) for r in WROWS] + [(515, 1024), (2051, 1024), (2051, 768)]


def _run_bwd(ops, c, xhat, rstd, ref, yard, tag, fails):
    """the three backward forms on device tensors (xhat, rstd): gates against `ref`, bit identities between the forms"""
    d = dev()
    from vbg.lib import lib
    rows, hid, p = c.rows, c.hid, c.p
    w = WROWS[rows]
    assert int(lib.vbg_ln_bwd_ws_rows(rows)) == -(-rows // (4 * w)), (rows, w, int(lib.vbg_ln_bwd_ws_rows(rows)))
    dy, gam = c.dy.to(d), c.gam.to(d)
    st = {k: v.to(d) for k, v in c.start.items()}
    # fp32 form
    dg0, db0, s0 = st["dgamma"].clone(), st["dbeta"].clone(), ops.amax_slot(d)
    log = ops.dispatch_log(True)
    try:
        dx0, dres0 = ops.dropout_add_ln_bwd(dy, xhat, rstd, gam, p, c.seed, c.sid, dg0, db0, dx_amax=s0)
    finally:
        ops.dispatch_log(False)
    atomic = log.get("fatomic:ln_bwd", 0) == 1
    assert atomic == (rows < 512 and not ops.deterministic_active()), (rows, log)
    print(f"ROWEDGE {tag} wrows: workspace forms {w} ({int(lib.vbg_ln_bwd_ws_rows(rows))} partial rows), fp32 form "
          f"{'atomic route, wrows 2' if atomic else 'workspace, wrows %d' % w}")
    _rec(fails, tag, "dx", R.row_err(yard["dx"], ref["dx"]), R.row_err(dx0, ref["dx"]))
    _rec(fails, tag, "dres", R.row_err(yard["dz"], ref["dz"]), R.row_err(dres0, ref["dz"]))
    for k, got in (("dgamma", dg0), ("dbeta", db0)):
        _rec(fails, tag, k + "/fp32", R.col_err(yard[k], ref[k], ref["a_" + k]), R.col_err(got, ref[k], ref["a_" + k]))
    if c.keep is not None:
        assert bool((dx0.cpu()[torch.from_numpy(~c.keep)] == 0).all()), "a dropped position received gradient"
    true_bits = int(_bits(dx0.abs().max().reshape(1)).item())
    assert int(s0.max().item()) == true_bits, "amax word of the fp32 form != max |dx|"
    # bf16-plane form
    dg1, db1, dbi1 = st["dgamma"].clone(), st["dbeta"].clone(), st["dbias"].clone()
    pdx, dres1 = ops.dropout_add_ln_bwd_planes(dy, xhat, rstd, gam, p, c.seed, c.sid, dg1, db1, dbi1)
    assert torch.equal(_bits(dres1), _bits(dres0)), "dres of the plane form != fp32 form"
    assert torch.equal(pdx.buf, ops.split_planes(dx0).buf), "bf16 planes != split_planes(dx of the fp32 form)"
    # fp16-pair form
    dg2, db2, dbi2 = st["dgamma"].clone(), st["dbeta"].clone(), st["dbias"].clone()
    s_true, s_bound = ops.amax_slot(d), ops.amax_slot(d)
    q, dres2 = ops.dropout_add_ln_bwd_pair(dy, xhat, rstd, gam, p, c.seed, c.sid, dg2, db2, dbi2, ops.amax(dy), s_true, s_bound)
    assert torch.equal(_bits(dres2), _bits(dres0)), "dres of the pair form != fp32 form"
    assert torch.equal(q.buf, ops.split_planes_pair(dx0, amax_slot_=s_bound).buf), "pair planes != split_planes_pair(dx, bound slot)"
    bound, true_max = float(s_bound.view(torch.float32).max().item()), float(dx0.abs().max())
    assert true_max <= bound, (true_max, bound)
    assert int(s_true.max().item()) == true_bits, "amax word of the pair form != max |dx|"
    for form, trio in (("planes", (dg1, db1, dbi1)), ("pair", (dg2, db2, dbi2))):
        for k, got in zip(("dgamma", "dbeta", "dbias"), trio):
            _rec(fails, tag, f"{k}/{form}", R.col_err(yard[k], ref[k], ref["a_" + k]), R.col_err(got, ref[k], ref["a_" + k]))


def _no_forced_wrows():
    if os.environ.get("VBG_LN_WROWS"):
        pytest.skip("VBG_LN_WROWS is set: the library read it at load, wrows no longer follows the row count")


# ---------------------------------------------------------------------------------------------------------------------------------------
# dropout_add_ln_fwd
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 130])
@pytest.mark.parametrize("hid", [256, 512, 768, 1024])
def test_dropout_add_ln_fwd_vs_fp64(ops, hid, rows, p):
    d = dev()
    c = _ln_case(rows, hid, p)
    tag = f"add_ln_fwd[{rows}x{hid},p={p}]"
    xp, res, gam, bet = c.xp.to(d), c.res.to(d), c.gam.to(d), c.bet.to(d)
    y, xhat, rstd = ops.dropout_add_ln_fwd(xp, res, gam, bet, EPS, p, c.seed, c.sid)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(xhat).all()) and bool(torch.isfinite(rstd).all()), "a dropped inf leaked"
    fails = []
    _rec(fails, tag, "y", R.row_err(c.y32, c.y64), R.row_err(y, c.y64))
    _rec(fails, tag, "xhat", R.row_err(c.xh32, c.xh64), R.row_err(xhat, c.xh64))
    _rec(fails, tag, "rstd", float(((c.rs32.double() - c.rs64).abs() / c.rs64).max()), float(((rstd.cpu().double() - c.rs64).abs() / c.rs64).max()))
    # the planes of y written by the same launch
    ypl, yq = ops.planes_empty(rows, hid, d), ops.pair_empty(rows, hid, d)
    y2, xhat2, rstd2 = ops.dropout_add_ln_fwd(xp, res, gam, bet, EPS, p, c.seed, c.sid, out_planes=ypl, out_pair=yq)
    assert torch.equal(_bits(y2), _bits(y)) and torch.equal(_bits(xhat2), _bits(xhat)) and torch.equal(_bits(rstd2), _bits(rstd))
    assert torch.equal(ypl.buf, ops.split_planes(y).buf), "bf16 planes of y != split_planes(y)"
    assert torch.equal(yq.buf, ops.split_planes_pair(y).buf), "fp16-pair planes of y != split_planes_pair(y)"
    assert not fails, fails


# ---------------------------------------------------------------------------------------------------------------------------------------
# the three backward forms at the edges of wrows
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("rows,hid", BWD_CASES)
def test_dropout_add_ln_bwd_vs_fp64(ops, rows, hid, p):
    _no_forced_wrows()
    d = dev()
    c = _ln_case(rows, hid, p)
    fails = []
    # isolated: the fp32 rounding of the fp64 (xhat, rstd); the reference is the fp64 backward from those same values
    xh, rs, ref, yard = _bwd_refs(c, "isolated")
    _run_bwd(ops, c, xh.to(d), rs.to(d), ref, yard, f"add_ln_bwd[{rows}x{hid},p={p},isolated]", fails)
    # chained: the forward kernel's own outputs; the reference is fp64 autograd of the whole
    _, xhat, rstd = ops.dropout_add_ln_fwd(c.xp.to(d), c.res.to(d), c.gam.to(d), c.bet.to(d), EPS, p, c.seed, c.sid)
    _, _, ref, yard = _bwd_refs(c, "chained")
    _run_bwd(ops, c, xhat, rstd, ref, yard, f"add_ln_bwd[{rows}x{hid},p={p},chained]", fails)
    assert not fails, fails


def test_dropout_add_ln_bwd_reuses_a_larger_workspace(ops):
    """2051 rows, then 515 rows on the same stream with every partials workspace filled with NaN in between: the second call folds only
    the rows its own blocks wrote"""
    _no_forced_wrows()
    from vbg.lib import lib
    d = dev()
    fails = []
    for rows in (2051, 515):
        c = _ln_case(rows, 256, 0.0)
        xh, rs, ref, yard = _bwd_refs(c, "isolated")
        if rows == 515:
            assert ops._LN_WS, "no workspace was allocated by the first call"
            for ws in ops._LN_WS.values():
                ws.fill_(float("nan"))
            for na in (2, 3):
                ws = [v for k, v in ops._LN_WS.items() if k[1] == 256 and k[2] == na and k[3] == ops.raw_stream(d)]
                assert len(ws) == 1 and ws[0].numel() > int(lib.vbg_ln_bwd_ws_rows(515)) * na * 256
        _run_bwd(ops, c, xh.to(d), rs.to(d), ref, yard, f"add_ln_bwd[{rows}x256,reuse]", fails)
    assert not fails, fails


# ---------------------------------------------------------------------------------------------------------------------------------------
# embed_ln_fwd / embed_ln_bwd, default and deterministic
# ---------------------------------------------------------------------------------------------------------------------------------------
V_WORD, N_POS = 50, 20


@functools.lru_cache(maxsize=4)
def _emb_case(hid, ntok, p, same=False, seed=9, sid=1):
    g = torch.Generator().manual_seed(7 * hid + 1000 * ntok + int(100 * p) + (5 if same else 0))
    c = types.SimpleNamespace(hid=hid, ntok=ntok, p=p, seed=seed, sid=sid)

    def table(n):
        return (torch.exp2(torch.randint(-2, 3, (n, 1), generator=g).float()) * (torch.randn(n, hid, generator=g) + 3.0 * torch.randn(n, 1, generator=g))).contiguous()

    c.word, c.pos, c.typ = table(V_WORD), table(N_POS), table(1)[0].contiguous()
    c.gam, c.bet = 1 + 0.2 * torch.randn(hid, generator=g), 0.1 * torch.randn(hid, generator=g)
    c.ids, c.pid = torch.randint(0, V_WORD, (ntok,), generator=g), torch.randint(0, N_POS, (ntok,), generator=g)
    c.ids[0], c.pid[0] = 0, 0                                          # ids that include 0 and V - 1 (one token: V - 1)
    c.ids[-1], c.pid[-1] = V_WORD - 1, N_POS - 1
    if same:
        c.ids[:], c.pid[:] = 7, 3                                      # one table row receives all the gradient
    c.dout = (torch.randn(ntok, hid, generator=g) * torch.exp2(torch.randint(-4, 5, (ntok, 1), generator=g).float())).contiguous()
    c.start = dict(dword=torch.randn(V_WORD, hid, generator=g), dpos=torch.randn(N_POS, hid, generator=g), dtype0=torch.randn(hid, generator=g),
                   dgamma=torch.randn(hid, generator=g), dbeta=torch.randn(hid, generator=g))
    c.keep = R.keep_mask(seed, sid, ntok, hid, p) if p > 0 else None
    c.out64, c.xh64, c.rs64 = R.embed_fwd(c.ids, c.pid, c.word, c.pos, c.typ, c.gam, c.bet, EPS, c.keep, p)
    y32, mean32, rs32 = torch.native_layer_norm((c.word[c.ids] + c.typ) + c.pos[c.pid], (hid,), c.gam, c.bet, EPS)
    c.out32, c.rs32 = R._drop(y32, c.keep, p), rs32.reshape(-1)
    c.xh32 = (((c.word[c.ids] + c.typ) + c.pos[c.pid]) - mean32) * rs32
    # backward from the fp32 rounding of the fp64 (xhat, rstd): fp64 reference and the fp32 yardstick (index_add_ for the tables)
    c.xh, c.rs = c.xh64.float(), c.rs64.float()
    ref = R.embed_bwd(c.dout, c.xh, c.rs, c.ids, c.pid, c.gam, V_WORD, N_POS, c.keep, p)
    g32 = R._drop(c.dout, c.keep, p)
    b = _bwd32(g32, c.xh, c.rs, c.gam, None, 0.0)
    yard = dict(dgamma=b["dgamma"], dbeta=b["dbeta"], dtype0=b["dz"].sum(0),
                dword=torch.zeros(V_WORD, hid).index_add_(0, c.ids, b["dz"]), dpos=torch.zeros(N_POS, hid).index_add_(0, c.pid, b["dz"]))
    for k in c.start:
        ref[k] = c.start[k].double() + ref[k]
        ref["a_" + k] = c.start[k].double().abs() + ref["a_" + k]
        yard[k] = c.start[k] + yard[k]
    c.ref, c.yard = ref, yard
    return c


def _run_embed(ops, c, tag):
    d = dev()
    fails = []
    ids, pid = c.ids.int().to(d), c.pid.int().to(d)
    gam = c.gam.to(d)
    out, xhat, rstd = ops.embed_ln_fwd(ids, pid, c.word.to(d), c.pos.to(d), c.typ.to(d), gam, c.bet.to(d), EPS, c.p, c.seed, c.sid)
    _rec(fails, tag, "out", R.row_err(c.out32, c.out64), R.row_err(out, c.out64))
    _rec(fails, tag, "xhat", R.row_err(c.xh32, c.xh64), R.row_err(xhat, c.xh64))
    _rec(fails, tag, "rstd", float(((c.rs32.double() - c.rs64).abs() / c.rs64).max()), float(((rstd.cpu().double() - c.rs64).abs() / c.rs64).max()))
    if c.keep is not None:
        assert bool((out.cpu()[torch.from_numpy(~c.keep)] == 0).all()), "a dropped output is not zero"
    prev = ops.deterministic()
    for det in (False, True):
        acc = {k: v.to(d).clone() for k, v in c.start.items()}
        try:
            ops.set_deterministic(det)
            ops.embed_ln_bwd(c.dout.to(d), c.xh.to(d), c.rs.to(d), ids, pid, gam, c.p, c.seed, c.sid, acc["dword"], acc["dpos"], acc["dtype0"],
                             acc["dgamma"], acc["dbeta"])
        finally:
            ops.set_deterministic(prev)
        for k in ("dword", "dpos", "dtype0", "dgamma", "dbeta"):
            _rec(fails, tag, f"{k}/{'det' if det else 'atomic'}", R.col_err(c.yard[k], c.ref[k], c.ref["a_" + k]),
                 R.col_err(acc[k], c.ref[k], c.ref["a_" + k]))
    assert not fails, fails


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("ntok", [1, 15, 16, 17, 77])
@pytest.mark.parametrize("hid", [1, 100, 768, 1000, 1024])
def test_embed_ln_vs_fp64(ops, hid, ntok, p):
    _run_embed(ops, _emb_case(hid, ntok, p), f"embed_ln[{ntok}x{hid},p={p}]")


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_embed_ln_all_tokens_on_one_table_row(ops, p):
    _run_embed(ops, _emb_case(768, 77, p, same=True), f"embed_ln[77x768,p={p},one id]")


def test_embed_ln_rejects_hidden_above_1024(ops):
    from vbg.lib import VbgError
    d = dev()
    hid, n = 1025, 4
    z = torch.zeros(n, hid, device=d)
    ids = torch.zeros(n, device=d, dtype=torch.int32)
    v = torch.zeros(hid, device=d)
    with pytest.raises(VbgError, match="argument error"):
        ops.embed_ln_fwd(ids, ids, z, z, v, v, v, EPS, 0.0, 1, 0)
    prev = ops.deterministic()
    for det in (False, True):
        try:
            ops.set_deterministic(det)
            with pytest.raises(VbgError, match="argument error"):
                ops.embed_ln_bwd(z, z, torch.ones(n, device=d), ids, ids, v, 0.0, 1, 0, z.clone(), z.clone(), v.clone(), v.clone(), v.clone())
        finally:
            ops.set_deterministic(prev)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------------
# which element draws which bit
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,sid,rows,hid,p", R.DROPOUT_CASES[:3])
def test_add_ln_dropout_bits_are_the_predicted_ones(ops, seed, sid, rows, hid, p):
    d = dev()
    keep = R.keep_mask(seed, sid, rows, hid, p)
    assert bool((keep.any(1) & ~keep.all(1)).all())                    # every row has a kept and a dropped element
    one, zero = torch.ones(rows, hid, device=d), torch.zeros(rows, hid, device=d)
    gam1, bet0 = torch.ones(hid, device=d), torch.zeros(hid, device=d)
    # dropout(1) + 0 is {0, 1 / (1 - p)}: after the LayerNorm the kept elements of a row are positive, the dropped negative
    y, xhat, rstd = ops.dropout_add_ln_fwd(one, zero, gam1, bet0, EPS, p, seed, sid)
    got = (y > 0).cpu().numpy()
    assert np.array_equal(got, keep), f"{int((got != keep).sum())} of {keep.size} forward keep bits differ from the prediction"
    y_other = ops.dropout_add_ln_fwd(one, zero, gam1, bet0, EPS, p, seed, sid + 1)[0]
    assert not np.array_equal((y_other > 0).cpu().numpy(), keep)
    # backward: dx is dz where kept (dz is a real number, zero with probability zero) and exactly zero where dropped
    dy = torch.randn(rows, hid, generator=torch.Generator().manual_seed(3)).to(d)
    dx, dres = ops.dropout_add_ln_bwd(dy, xhat, rstd, gam1, p, seed, sid, torch.zeros(hid, device=d), torch.zeros(hid, device=d))
    assert int((dres == 0).sum().item()) == 0
    got = (dx != 0).cpu().numpy()
    assert np.array_equal(got, keep), f"{int((got != keep).sum())} backward keep bits differ from the prediction"
    ks = R.keep_scale(p)
    assert torch.equal(dx.cpu()[torch.from_numpy(keep)], (dres.cpu() * ks)[torch.from_numpy(keep)])


def test_embed_ln_dropout_bits_are_the_predicted_ones(ops):
    seed, sid, ntok, hid, p = R.DROPOUT_CASES[3]
    d = dev()
    keep = R.keep_mask(seed, sid, ntok, hid, p)
    c = _emb_case(hid, ntok, 0.0)
    ids, pid = c.ids.int().to(d), c.pid.int().to(d)
    gam0, bet1 = torch.zeros(hid, device=d), torch.ones(hid, device=d)
    args = (ids, pid, c.word.to(d), c.pos.to(d), c.typ.to(d), gam0, bet1, EPS, p)
    out, xhat, rstd = ops.embed_ln_fwd(*args, seed, sid)                # gamma = 0, beta = 1: the output is the keep pattern / (1 - p)
    ks = torch.tensor(R.keep_scale(p), dtype=torch.float32)
    assert torch.equal(out.cpu(), torch.from_numpy(keep).float() * ks)
    assert not np.array_equal((ops.embed_ln_fwd(*args, seed, sid + 1)[0] != 0).cpu().numpy(), keep)
    # backward, gamma = 0: dbeta is the column sum of keep * dout / (1 - p).  dout = 1: the column's count of kept tokens
    acc = [torch.zeros(V_WORD, hid, device=d), torch.zeros(N_POS, hid, device=d)] + [torch.zeros(hid, device=d) for _ in range(3)]
    ops.embed_ln_bwd(torch.ones(ntok, hid, device=d), xhat, rstd, ids, pid, gam0, p, seed, sid, *acc)
    assert torch.equal(torch.round(acc[4].cpu() / ks).long(), torch.from_numpy(keep.sum(0)))
    # ... and bit by bit: one token's gradient at a time (a single non-zero term per column: the sum is exact)
    for t in (0, 16, 76):
        e = torch.zeros(ntok, hid)
        e[t] = 1.0
        acc = [torch.zeros(V_WORD, hid, device=d), torch.zeros(N_POS, hid, device=d)] + [torch.zeros(hid, device=d) for _ in range(3)]
        ops.embed_ln_bwd(e.to(d), xhat, rstd, ids, pid, gam0, p, seed, sid, *acc)
        assert torch.equal(acc[4].cpu(), torch.from_numpy(keep[t]).float() * ks), t


# ---------------------------------------------------------------------------------------------------------------------------------------
# attention dropout words
# ---------------------------------------------------------------------------------------------------------------------------------------
def _mask_meta(lens, heads):
    from model.BERTgrid_generator import flash_tables
    sl = np.asarray(lens, np.int64)
    mask_off, mask_words = flash_tables(sl, heads)[4:6]
    d = dev()
    m = types.SimpleNamespace(nseq=len(sl), heads=heads, maxlen=int(sl.max()), mask_words=int(mask_words))
    m.lens = torch.from_numpy(sl).int().to(d)
    m.mask_off = torch.from_numpy(mask_off).to(d)
    return m, sl, mask_off


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _check_layers(ops, lens, heads, nlayers, p, seed, sid0, stride, per_layer_calls):
    m, sl, mask_off = _mask_meta(lens, heads)
    layers = ops.attn_mask_layers(m, p, seed, sid0, stride, nlayers)
    assert len(layers) == nlayers
    for l, (mq, mk) in enumerate(layers):
        rq, rk, defined = R.attn_mask_words(sl, mask_off, heads, m.maxlen, p, seed, sid0 + l * stride)
        assert defined.size == m.mask_words
        gq, gk = _u32(mq), _u32(mk)
        assert np.array_equal(gq[defined], rq[defined]), f"layer {l}: {int((gq[defined] != rq[defined]).sum())} mask_q words differ"
        assert np.array_equal(gk[defined], rk[defined]), f"layer {l}: {int((gk[defined] != rk[defined]).sum())} mask_k words differ"
        if per_layer_calls:
            sq, sk = ops.attn_mask(m, p, seed, sid0 + l * stride)
            assert np.array_equal(_u32(sq)[defined], rq[defined]) and np.array_equal(_u32(sk)[defined], rk[defined]), f"attn_mask, layer {l}"
    return m


def test_attn_mask_words_odd_block_counts(ops):
    """32-key block counts 1, 1, 1, 2, 3, 4: with an odd count the upper half-wave of the last block pair holds kb == nkb and stores nothing
    (its words would land in the next query's row)"""
    _check_layers(ops, [1, 31, 32, 33, 65, 97], 3, 12, 0.1, 1234, 5, 7, per_layer_calls=True)


def test_attn_mask_layers_split_over_two_launches(ops):
    g = torch.Generator().manual_seed(4)
    lens = torch.randint(1, 5, (456,), generator=g).tolist() + [33]
    m = _check_layers(ops, lens, 12, 12, 0.1, 77, 0, 8, per_layer_calls=False)
    assert 65535 // (m.nseq * m.heads) == 11                           # eleven layers in the first launch, the twelfth in a second


def test_attn_mask_more_groups_than_the_grid_limit(ops):
    g = torch.Generator().manual_seed(5)
    lens = torch.randint(1, 5, (5462,), generator=g).tolist()
    m = _check_layers(ops, lens, 12, 2, 0.1, 78, 3, 5, per_layer_calls=True)
    assert m.nseq * m.heads == 65544 > 65535


# ---------------------------------------------------------------------------------------------------------------------------------------
# arguments the entry points reject before any launch
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hid", [128, 300, 1280])
def test_add_ln_rejects_unsupported_hidden(ops, hid):
    from vbg.lib import VbgError
    d = dev()
    rows = 8
    z, v, r = torch.zeros(rows, hid, device=d), torch.ones(hid, device=d), torch.ones(rows, device=d)
    with pytest.raises(VbgError, match="argument error"):
        ops.dropout_add_ln_fwd(z, z, v, v, EPS, 0.0, 1, 0)
    with pytest.raises(VbgError, match="argument error"):
        ops.dropout_add_ln_bwd(z, z, r, v, 0.0, 1, 0, v.clone(), v.clone())
    if hid % 32 == 0:                                                  # (the plane forms need ld == hidden, a multiple of 32, to be called at all)
        with pytest.raises(VbgError, match="argument error"):
            ops.dropout_add_ln_fwd(z, z, v, v, EPS, 0.0, 1, 0, out_planes=ops.planes_empty(rows, hid, d), out_pair=ops.pair_empty(rows, hid, d))
        with pytest.raises(VbgError, match="argument error"):
            ops.dropout_add_ln_bwd_planes(z, z, r, v, 0.0, 1, 0, v.clone(), v.clone(), v.clone())
        with pytest.raises(VbgError, match="argument error"):
            ops.dropout_add_ln_bwd_pair(z, z, r, v, 0.0, 1, 0, v.clone(), v.clone(), v.clone(), ops.amax_slot(d), ops.amax_slot(d), ops.amax_slot(d))
    torch.cuda.synchronize()


def test_add_ln_rejects_misaligned_rows_and_p_of_one(ops):
    from vbg.lib import VbgError
    d = dev()
    rows, hid = 8, 256
    z, v, r = torch.zeros(rows, hid, device=d), torch.ones(hid, device=d), torch.ones(rows, device=d)
    off = torch.zeros(rows * hid + 4, device=d)[1:1 + rows * hid].view(rows, hid)        # 4 bytes past a 16-byte boundary
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    with pytest.raises(VbgError, match="argument error"):
        ops.dropout_add_ln_fwd(off, z, v, v, EPS, 0.0, 1, 0)
    with pytest.raises(VbgError, match="argument error"):
        ops.dropout_add_ln_bwd(off, z, r, v, 0.0, 1, 0, v.clone(), v.clone())
    with pytest.raises(VbgError, match="argument error"):
        ops.dropout_add_ln_bwd_planes(off, z, r, v, 0.0, 1, 0, v.clone(), v.clone(), v.clone())
    for p in (1.0, -0.1):
        with pytest.raises(VbgError, match="argument error"):
            ops.dropout_add_ln_fwd(z, z, v, v, EPS, p, 1, 0)
        with pytest.raises(VbgError, match="argument error"):
            ops.dropout_add_ln_bwd(z, z, r, v, p, 1, 0, v.clone(), v.clone())
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the in-place elementwise kernels past their grid cap (2048 blocks of 256 threads): grid-stride loop and scalar tail together
# ---------------------------------------------------------------------------------------------------------------------------------------
N_VEC = 2048 * 256 * 4 + 3


def test_add_inplace_past_the_grid_cap(ops):
    g = torch.Generator().manual_seed(11)
    a, b = torch.randn(N_VEC, generator=g), torch.randn(N_VEC, generator=g) * 3
    got = ops.add_(a.to(dev()), b.to(dev())).cpu()
    assert torch.equal(got, (a.double() + b.double()).float())         # an fp32 addition is the rounded exact sum


def test_relu_bwd_past_the_grid_cap(ops):
    g = torch.Generator().manual_seed(12)
    y, dy = torch.relu(torch.randn(N_VEC, generator=g)), torch.randn(N_VEC, generator=g)
    got = ops.relu_bwd_(y.to(dev()), dy.to(dev())).cpu()
    assert torch.equal(got, torch.where(y > 0, dy, torch.zeros(())))
    assert int((got == 0).sum()) > N_VEC // 4 and int((got != 0).sum()) > N_VEC // 4


def test_gelu_bwd_past_the_grid_cap(ops):
    """|dg gelu'(h) - got| <= |dg| max(1, |h|) (2.5e-7 + 1.13 * 2^-24): the bound test_gelu_erf_epilogues holds gelu' itself to, plus the
    rounding of the product (|gelu'| <= 1.13)"""
    g = torch.Generator().manual_seed(13)
    h, dg = torch.randn(N_VEC, generator=g) * 1.5, torch.randn(N_VEC, generator=g)
    got = ops.gelu_bwd_(h.to(dev()), dg.to(dev())).cpu().double()
    hd = h.double()
    ref = dg.double() * (0.5 * (1 + torch.special.erf(hd / 2 ** 0.5)) + hd * torch.exp(-0.5 * hd * hd) / (2 * math.pi) ** 0.5)
    lim = dg.double().abs() * hd.abs().clamp_min(1.0) * (2.5e-7 + 1.13 * 2.0 ** -24)
    assert bool(((got - ref).abs() <= lim).all()), float(((got - ref).abs() / lim.clamp_min(1e-300)).max())
    assert bool((got[-3:] != dg[-3:].double()).all())                  # the scalar tail ran


def test_scale_inplace_past_the_grid_cap(ops):
    n = 2048 * 256 + 1
    a = torch.randn(n, generator=torch.Generator().manual_seed(14))
    s = 0.3
    got = ops.scale_(a.to(dev()), s).cpu()
    assert torch.equal(got, (a.double() * float(np.float32(s))).float())          # an fp32 product is the rounded exact product
