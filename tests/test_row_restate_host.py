"""The restatements of tests/row_restate.py against independent statements, on the CPU: the fp64 LayerNorm backward against torch fp64
autograd, the numpy RNG against what csrc/vbg_common.h's own rng_u32 printed (tools/rng_u32_host.cpp -> tests/golden/rng_u32.txt), the
keep rate of the masks the GPU tests pin, and the two orientations of the attention mask words against each other."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import row_restate as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
f64 = torch.float64


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def test_layernorm_backward_equals_fp64_autograd():
    g = torch.Generator().manual_seed(1)
    rows, hid, p = 37, 256, 0.1
    x = torch.randn(rows, hid, generator=g, dtype=f64).requires_grad_(True)
    res = torch.randn(rows, hid, generator=g, dtype=f64).requires_grad_(True)
    gam = (1 + 0.2 * torch.randn(hid, generator=g, dtype=f64)).requires_grad_(True)
    bet = (0.1 * torch.randn(hid, generator=g, dtype=f64)).requires_grad_(True)
    keep = R.keep_mask(3, 4, rows, hid, p)
    assert 0 < keep.sum() < keep.size
    y = F.layer_norm(torch.from_numpy(keep).to(f64) * x * R.keep_scale(p) + res, (hid,), gam, bet, 1e-12)
    gy = torch.randn(rows, hid, generator=g, dtype=f64)
    y.backward(gy)
    y2, xhat, rstd = R.ln_fwd(x.detach(), res.detach(), gam.detach(), bet.detach(), 1e-12, keep, p)
    assert _rel(y2, y.detach()) <= 1e-12
    r = R.ln_bwd(gy, xhat, rstd, gam.detach(), keep, p)
    assert _rel(r["dx"], x.grad) <= 1e-12 and _rel(r["dz"], res.grad) <= 1e-12
    assert _rel(r["dgamma"], gam.grad) <= 1e-12 and _rel(r["dbeta"], bet.grad) <= 1e-12
    assert _rel(r["dbias"], x.grad.sum(0)) <= 1e-12
    assert bool((r["dx"][torch.from_numpy(~keep)] == 0).all())
    # a dropped position contributes nothing, whatever it holds
    xp = x.detach().clone()
    xp[torch.from_numpy(~keep)] = float("inf")
    assert torch.equal(R.ln_fwd(xp, res.detach(), gam.detach(), bet.detach(), 1e-12, keep, p)[0], y2)


def test_embedding_form_equals_fp64_autograd():
    g = torch.Generator().manual_seed(2)
    V, Pn, hid, n, p = 11, 5, 100, 37, 0.1
    word = torch.randn(V, hid, generator=g, dtype=f64).requires_grad_(True)
    pos = torch.randn(Pn, hid, generator=g, dtype=f64).requires_grad_(True)
    typ = torch.randn(hid, generator=g, dtype=f64).requires_grad_(True)
    gam = (1 + 0.2 * torch.randn(hid, generator=g, dtype=f64)).requires_grad_(True)
    bet = (0.1 * torch.randn(hid, generator=g, dtype=f64)).requires_grad_(True)
    ids = torch.randint(0, V, (n,), generator=g)              # 37 draws of 11 ids: repeated
    pid = torch.randint(0, Pn, (n,), generator=g)
    assert len(set(ids.tolist())) < n
    keep = R.keep_mask(8, 9, n, hid, p)
    out = torch.from_numpy(keep).to(f64) * F.layer_norm(word[ids] + typ + pos[pid], (hid,), gam, bet, 1e-12) * R.keep_scale(p)
    gy = torch.randn(n, hid, generator=g, dtype=f64)
    out.backward(gy)
    o2, xhat, rstd = R.embed_fwd(ids, pid, word.detach(), pos.detach(), typ.detach(), gam.detach(), bet.detach(), 1e-12, keep, p)
    assert _rel(o2, out.detach()) <= 1e-12
    r = R.embed_bwd(gy, xhat, rstd, ids, pid, gam.detach(), V, Pn, keep, p)
    for name, ref in (("dword", word.grad), ("dpos", pos.grad), ("dtype0", typ.grad), ("dgamma", gam.grad), ("dbeta", bet.grad)):
        assert _rel(r[name], ref) <= 1e-12, name


def test_rng_equals_the_header():
    """the fixture is the output of a host program that includes csrc/vbg_common.h; indices above 2^32 and stream 2^40 are in it"""
    rows, thr = [], []
    with open(os.path.join(GOLDEN, "rng_u32.txt")) as f:
        for line in f:
            if line.startswith("#"):
                continue
            t = line.split()
            if t[0] == "thr":
                thr.append((float(t[1]), int(t[2])))
            else:
                rows.append(tuple(int(v) for v in t))
    assert len(rows) == 6 * 6 * 13 and len(thr) == 7
    assert any(r[2] > 2 ** 32 for r in rows) and any(r[1] == 2 ** 40 for r in rows)
    for seed, sid, idx, want in rows:                                        # one at a time
        assert int(R.rng_u32(seed, sid, idx)) == want, (seed, sid, idx)
    a = np.array(rows, dtype=np.uint64)                                     # and as arrays (the form keep_mask uses)
    assert np.array_equal(R.rng_u32(a[:, 0], a[:, 1], a[:, 2]), a[:, 3].astype(np.uint32))
    for p, want in thr:
        assert R.drop_threshold(p) == want, p
    assert R.thr16(0.1) == 6554 and R.thr16(0.5) == 32768 and R.thr16(0.0) == 0 and R.thr16(1.0) == 65535


@pytest.mark.parametrize("seed,sid,rows,hidden,p", R.DROPOUT_CASES)
def test_keep_rate_of_the_pinned_masks(seed, sid, rows, hidden, p):
    keep = R.keep_mask(seed, sid, rows, hidden, p)
    n, q = keep.size, 1.0 - float(np.float32(p))
    sigma = math.sqrt(q * (1 - q) / n)
    dev = abs(float(keep.mean()) - q) / sigma
    print(f"keep rate {keep.mean():.6f} vs {q:.6f}: {dev:.2f} sigma of n = {n}")
    assert dev <= 4.0
    assert not np.array_equal(keep, R.keep_mask(seed, sid + 1, rows, hidden, p))


def _bits(words, Q, nkb):
    w = words.reshape(Q, nkb)
    return ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(Q, 32 * nkb).astype(bool)


def test_attn_mask_words_orientations_and_stream_ids():
    from model.BERTgrid_generator import flash_tables
    lens, heads, p = np.asarray([1, 31, 32, 33, 65, 97], np.int64), 3, 0.1
    mask_off, words = flash_tables(lens, heads)[4:6]
    mq, mk, defined = R.attn_mask_words(lens, mask_off, heads, int(lens.max()), p, 1234, 5)
    assert mq.size == words and np.array_equal(defined, np.arange(words))      # the tables leave no gap between sequences
    for s, L in enumerate(lens):
        nkb = (int(L) + 31) // 32
        Q = 32 * nkb
        for h in range(heads):
            o = int(mask_off[s]) + h * Q * nkb
            kq, kk = _bits(mq[o:o + Q * nkb], Q, nkb), _bits(mk[o:o + Q * nkb], Q, nkb)
            assert np.array_equal(kk, kq.T), (s, h)
    rate = _bits(mq[:32], 32, 1).mean()
    assert 0.7 < rate < 1.0
    # a layer's words depend on (sid0, l, stride) only through sid0 + l * stride
    a = R.attn_mask_words(lens, mask_off, heads, 97, p, 1234, 5 + 3 * 7)
    b = R.attn_mask_words(lens, mask_off, heads, 97, p, 1234, 26)
    c = R.attn_mask_words(lens, mask_off, heads, 97, p, 1234, 5 + 3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and not np.array_equal(a[0], c[0])
    # one draw spelled out: group (seq 3, head 2), query 40, key 33 -> hash index (((g maxlen + q) ceil(maxlen / 32) + 1) 8 + 0, slice 1
    g, q, maxlen = 3 * heads + 2, 40, 97
    z = int(R.rng_state(1234, 5, ((g * maxlen + q) * 4 + 1) * 8 + 0))
    bit = ((z >> 16) & 0xFFFF) >= R.thr16(p)
    o = int(mask_off[3]) + 2 * 64 * 2
    assert bool((mq[o + q * 2 + 1] >> 1) & 1) == bit and bool((mk[o + 33 * 2 + 1] >> (40 - 32)) & 1) == bit
