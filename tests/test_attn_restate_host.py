"""tests/attn_restate.py checked on the host: the fp64 statement against torch autograd, the fp32 restatement's finiteness, and the property
every input builder was built to have -- on exactly the batches tests/test_gpu_attention_edges.py runs, so a changed seed or length is
re-checked here without a GPU."""
import numpy as np
import pytest
import torch

import attn_restate as A
import row_restate as R

SCALE = 0.125


def _offsets(lens, heads):
    lens = np.asarray(lens, np.int64)
    lpad = (lens + 31) // 32 * 32
    words = heads * lpad * (lpad // 32)
    return np.concatenate([[0], np.cumsum(words)[:-1]]).astype(np.int64)


def _keeps(lens, heads, p):
    off = _offsets(lens, heads)
    mq, mk, _ = R.attn_mask_words(lens, off, heads, max(lens), p, A.DROP_SEED, A.DROP_STREAM)
    keeps = A.keep_matrices(mq, off, lens, heads)
    for (s, h), k in keeps.items():
        assert (k == A.keep_matrix(mk, int(off[s]), h, lens[s]).T).all()
    return keeps


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_statement_equals_autograd(p):
    lens, heads = [33, 5, 1, 70], 2
    qkv, dO = A.base_inputs(lens, heads, 1)
    keeps = _keeps(lens, heads, p) if p > 0 else None
    ks = R.keep_scale(p) if p > 0 else 1.0
    st = A.statement(qkv, dO, lens, heads, SCALE, keeps, ks)
    ag = A.autograd_reference(qkv, dO, lens, heads, SCALE, keeps, ks)
    for n in ("O", "dq", "dk", "dv"):
        assert A.global_err(st[n], ag[n]) < 1e-12, n
        assert A.group_err(st[n], ag[n], lens, heads)[0] < 1e-12, n
    assert float((st["lse"] - ag["lse"]).abs().max()) < 1e-12


def test_group_err_sees_a_short_sequence_and_demands_exact_zeros():
    lens, heads = [512, 4], 1
    ref = torch.randn(516, 64, dtype=torch.float64)
    ref[512:] *= 1e-3
    got = ref.clone()
    got[513, 7] += 1e-4                                    # 1e-4 of the batch's magnitude, a tenth of the short sequence's
    assert A.global_err(got, ref) < 1e-4
    e, where = A.group_err(got, ref, lens, heads)
    assert where == (1, 0) and e > 1e-2
    ref[512:] = 0.0
    assert A.group_err(ref, ref, lens, heads)[0] == 0.0
    got = ref.clone()
    got[515, 0] = 1e-30
    assert A.group_err(got, ref, lens, heads) == (float("inf"), (1, 0))
    got[515, 0] = float("nan")
    assert A.group_err(got, ref, lens, heads)[0] == float("inf")


def _finite32(qkv, dO, lens, heads, keeps=None, ks=1.0):
    r = A.statement(qkv, dO, lens, heads, SCALE, keeps, ks, dtype=torch.float32)
    for n, v in r.items():
        if n == "smax":
            continue
        assert v.dtype == torch.float32 and bool(torch.isfinite(v).all()), n
    return r


@pytest.mark.parametrize("gammas", [A.GAMMAS, A.GAMMAS_MODEST])
def test_shifted(gammas):
    lens, heads = A.LENS_SHIFT, A.HEADS_SHIFT
    qkv0, dO = A.base_inputs(lens, heads, 2)
    qkv, info = A.shifted(qkv0, lens, heads, gammas)
    assert set(info["cls"].tolist()) == set(range(len(gammas)))          # every shift class occurs, in every sequence
    ref = A.statement(qkv, dO, lens, heads, SCALE)
    m = ref["rowmax"]
    if gammas is A.GAMMAS:
        assert float(m.min()) < -88.7 and float(m.max()) > 88.7          # past the range of exp in fp32, both ways
    else:
        assert -25.0 < float(m.min()) < -8.0 and float(m.max()) < 16.0
    # all scores of a row move by its shift ...
    for c, g in enumerate(gammas):
        rows = info["cls"] == c
        assert float(((m[:, rows] - info["shift"][rows]).abs()).max()) < 8.0
    # ... and the gradient of the shifted query column is the cancellation kappa scale sum_j dS_ij = 0
    for h in range(heads):
        assert float(ref["dq"][:, h * 64 + info["col"]].abs().max()) < 1e-12 * float(ref["dq"].abs().max())
    _finite32(qkv, dO, lens, heads)


def test_shift_does_not_move_the_probabilities():
    """the statement handles any shift: O and dv of shifted queries equal those of the same batch with gamma = 0"""
    lens, heads = A.LENS_SHIFT, A.HEADS_SHIFT
    qkv0, dO = A.base_inputs(lens, heads, 2)
    qkv, _ = A.shifted(qkv0, lens, heads, A.GAMMAS)
    flat, _ = A.shifted(qkv0, lens, heads, (0.0,))
    a, b = A.statement(qkv, dO, lens, heads, SCALE), A.statement(flat, dO, lens, heads, SCALE)
    for n in ("O", "dv"):
        assert A.group_err(a[n], b[n], lens, heads)[0] < 1e-12, n


def test_late_max():
    lens, heads = A.LENS_LATE, A.HEADS_LATE
    qkv0, dO = A.base_inputs(lens, heads, 3)
    qkv, info = A.late_max(qkv0, lens, heads)
    assert info["last"] >= 0.25 and info["first"] >= 0.25, info
    assert info["std"] >= 10.0, info
    _finite32(qkv, dO, lens, heads)


def test_ramp_and_zero_rows():
    lens, heads = A.LENS_RAMP, A.HEADS_RAMP
    qkv0, dO0 = A.base_inputs(lens, heads, 4)
    qkv, dO, info = A.ramp_v_and_dO(qkv0, dO0, lens, heads)
    r0 = A.row_starts(lens)
    for s, L in enumerate(lens):
        f = info["factor"][int(r0[s]):int(r0[s]) + L]
        t = f[::32]
        assert bool((t[1:] == (2.0 if s % 2 == 0 else 0.5) * t[:-1]).all())       # doubles (halves) at every tile
        assert float(f.max()) <= 2.0 ** 7 and float(f.min()) >= 2.0 ** -8
    assert torch.equal(qkv[:, 128:], qkv0[:, 128:] * info["factor"][:, None]) and torch.equal(qkv[:, :128], qkv0[:, :128])
    _finite32(qkv, dO, lens, heads)
    qz, dz, zi = A.zero_rows(qkv0, dO0, lens, heads)
    assert zi["zero_seq"] == 1 and len(zi["q"]) and len(zi["k"]) and len(zi["v"])
    ref = A.statement(qz, dz, lens, heads, SCALE)
    a, b = int(r0[1]), int(r0[1]) + lens[1]
    for n in ("dq", "dk", "dv"):
        assert float(ref[n][a:b].abs().max()) == 0.0 and float(ref[n][:a].abs().max()) > 0.0
    # a zero query row attends uniformly: its output is the mean of v
    q = zi["q"][0]
    assert float((ref["O"][q] - qz[:lens[0], 128:].double().mean(0)).abs().max()) < 1e-12
    _finite32(qz, dz, lens, heads)
    _finite32(qkv0, torch.zeros_like(dO0), lens, heads)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_batch_has_fully_dropped_rows(p):
    lens, heads = A.LENS_DROP, A.HEADS_DROP
    keeps = _keeps(lens, heads, p)
    dropped = A.fully_dropped_rows(keeps, lens, heads)
    assert len(dropped) >= 1
    qkv, dO = A.base_inputs(lens, heads, 6)
    ks = R.keep_scale(p)
    ref = A.statement(qkv, dO, lens, heads, SCALE, keeps, ks)
    r0 = A.row_starts(lens)
    for s, h, i in dropped:
        assert float(ref["O"][int(r0[s]) + i, h * 64:(h + 1) * 64].abs().max()) == 0.0
    _finite32(qkv, dO, lens, heads, keeps, ks)
