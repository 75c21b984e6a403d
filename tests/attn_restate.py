"""Self-attention on packed variable-length sequences restated in plain torch, independent of the library (no import of vbg), plus the
per-group error metric and the input builders of tests/test_gpu_attention_edges.py.

The operation (transformers' BertSelfAttention, model/BERTgrid_generator.py:134), per (sequence, head) with q, k, v [L, dh] taken from
the columns h dh, hidden + h dh, 2 hidden + h dh of qkv [ntok, 3 hidden]:
    S = q k^T scale;  m_i = max_j S_ij;  l_i = sum_j exp(S_ij - m_i);  P = exp(S - m) / l;  lse = m + log l
    Pd = P o keep ks (dropout: keep in {0, 1}, ks = keep scale);  O = Pd v
and its gradient for a given dO, written out (tests/test_attn_restate_host.py holds it to torch autograd at 1e-12):
    dPd = dO v^T;  dP = dPd o keep ks;  delta_i = sum_j P_ij dP_ij;  dS = P o (dP - delta)
    dq = dS k scale;  dk = dS^T q scale;  dv = Pd^T dO.
`statement` runs this in fp64 -- the reference -- or in fp32 on the CPU: the yardstick of "fp32-grade".  Softmax is invariant under a
shift of a row's scores; the statement subtracts the row maximum and therefore handles any shift, which is what the kernels have to match.

Dropout keeps are read back from the mask words attn_mask_kernel wrote (layout: tests/row_restate.py) by `keep_matrix`."""
import numpy as np
import torch

f64 = torch.float64


def keep_matrix(words, off, head, L):
    """mask words [L_pad, nkb] of one (sequence, head) -> bool [L, L] (query, key)"""
    nkb = (L + 31) // 32
    w = words[off + head * nkb * 32 * nkb: off + (head + 1) * nkb * 32 * nkb].reshape(nkb * 32, nkb).astype(np.uint32)
    bits = ((w[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & 1).reshape(nkb * 32, nkb * 32)
    return bits[:L, :L].astype(bool)


def keep_matrices(words, mask_off, lens, heads):
    """-> {(seq, head): bool [L, L]} from the query-major words of a whole batch"""
    return {(s, h): keep_matrix(words, int(mask_off[s]), h, int(L)) for s, L in enumerate(lens) for h in range(heads)}


def row_starts(lens):
    return np.concatenate([[0], np.cumsum(np.asarray(lens, np.int64))[:-1]]).astype(np.int64)


def groups(lens, heads):
    """(seq, head, first token row, L) of every (sequence, head) block"""
    r0 = row_starts(lens)
    return [(s, h, int(r0[s]), int(L)) for s, L in enumerate(lens) for h in range(heads)]


def statement(qkv, dO, lens, heads, scale, keeps=None, keep_scale=1.0, dtype=f64, dh=64):
    """-> dict(O, dq, dk, dv [ntok, heads dh]; lse, rowmax [heads, ntok]; smax = max |S|) of the operation above in `dtype` on the CPU.
    keeps: {(seq, head): bool [L, L]} or None; keep_scale: an INPUT of the operation, used as given."""
    hid = heads * dh
    x, g = qkv.detach().cpu().to(dtype), dO.detach().cpu().to(dtype)
    ntok = x.shape[0]
    out = {n: torch.zeros(ntok, hid, dtype=dtype) for n in ("O", "dq", "dk", "dv")}
    out["lse"], out["rowmax"] = torch.zeros(heads, ntok, dtype=dtype), torch.zeros(heads, ntok, dtype=dtype)
    smax = 0.0
    for s, h, r0, L in groups(lens, heads):
        rows, cols = slice(r0, r0 + L), slice(h * dh, (h + 1) * dh)
        q, k, v = x[rows, h * dh:(h + 1) * dh], x[rows, hid + h * dh:hid + (h + 1) * dh], x[rows, 2 * hid + h * dh:2 * hid + (h + 1) * dh]
        S = (q @ k.t()) * scale
        m = S.amax(1, keepdim=True)
        e = torch.exp(S - m)
        l = e.sum(1, keepdim=True)
        P = e / l
        kf = None if keeps is None else torch.from_numpy(np.ascontiguousarray(keeps[(s, h)])).to(dtype) * keep_scale
        Pd = P if kf is None else P * kf
        dPd = g[rows, cols] @ v.t()
        dP = dPd if kf is None else dPd * kf
        dS = P * (dP - (P * dP).sum(1, keepdim=True))
        out["O"][rows, cols] = Pd @ v
        out["dq"][rows, cols] = (dS @ k) * scale
        out["dk"][rows, cols] = (dS.t() @ q) * scale
        out["dv"][rows, cols] = Pd.t() @ g[rows, cols]
        out["lse"][h, rows] = (m + torch.log(l))[:, 0]
        out["rowmax"][h, rows] = m[:, 0]
        smax = max(smax, float(S.abs().max()))
    out["smax"] = smax
    return out


def autograd_reference(qkv, dO, lens, heads, scale, keeps=None, keep_scale=1.0, dh=64):
    """the same through torch: softmax(Q K^T scale) -> keep ks -> P V in fp64, gradients by autograd -> dict(O, lse, dq, dk, dv)"""
    hid = heads * dh
    x = qkv.detach().cpu().to(f64).requires_grad_(True)
    g = dO.detach().cpu().to(f64)
    O = torch.zeros(x.shape[0], hid, dtype=f64)
    lse = torch.zeros(heads, x.shape[0], dtype=f64)
    loss = 0.0
    for s, h, r0, L in groups(lens, heads):
        rows, cols = slice(r0, r0 + L), slice(h * dh, (h + 1) * dh)
        sc = (x[rows, h * dh:(h + 1) * dh] @ x[rows, hid + h * dh:hid + (h + 1) * dh].t()) * scale
        pr = torch.softmax(sc, -1)
        if keeps is not None:
            pr = pr * torch.from_numpy(np.ascontiguousarray(keeps[(s, h)])).to(f64) * keep_scale
        o = pr @ x[rows, 2 * hid + h * dh:2 * hid + (h + 1) * dh]
        O[rows, cols] = o.detach()
        lse[h, rows] = torch.logsumexp(sc, -1).detach()
        loss = loss + (o * g[rows, cols]).sum()
    loss.backward()
    return dict(O=O, lse=lse, dq=x.grad[:, :hid], dk=x.grad[:, hid:2 * hid], dv=x.grad[:, 2 * hid:])


# ---- error metric ------------------------------------------------------------------------------------------------------------------------
def group_errs(got, ref, lens, heads, dh=64):
    """max |got - ref| / max |ref| of every (sequence, head) block of a [ntok, heads dh] output, in the order of `groups`.  A block whose
    reference is all zeros must be zero exactly: anything else counts as inf (and so does a value that is not finite)."""
    got, ref = got.detach().cpu().to(f64), ref.detach().cpu().to(f64)
    errs = []
    for s, h, r0, L in groups(lens, heads):
        a, b = got[r0:r0 + L, h * dh:(h + 1) * dh], ref[r0:r0 + L, h * dh:(h + 1) * dh]
        den = float(b.abs().max())
        if not bool(torch.isfinite(a).all()):
            errs.append(float("inf"))
        elif den == 0.0:
            errs.append(0.0 if float(a.abs().max()) == 0.0 else float("inf"))
        else:
            errs.append(float((a - b).abs().max()) / den)
    return errs


def group_err(got, ref, lens, heads, dh=64):
    """-> (the worst group's value, its (seq, head))"""
    errs = group_errs(got, ref, lens, heads, dh)
    i = int(np.argmax(errs))
    s, h, _, _ = groups(lens, heads)[i]
    return errs[i], (s, h)


def global_err(got, ref):
    """the metric of tests/test_gpu_attention.py: max |error| over max |reference| of the whole tensor"""
    return float((got.detach().cpu().to(f64) - ref.detach().cpu().to(f64)).abs().max() / ref.detach().cpu().to(f64).abs().max())


FLOOR = dict(O=2e-6, dq=5e-6, dk=5e-6, dv=5e-6, lse=5e-6)       # the project's fp32-grade numbers (lse: absolute)
FACTOR = 8.0


def gate(name, e32, floor=None):
    """max(floor, 8 e32): e32 = the fp32 restatement's error on the same inputs.  The factor covers what the fp32 torch statement does not
    have: __expf (a couple of ulp plus its argument reduction) and another summation order over up to 512 keys."""
    return max(FLOOR[name] if floor is None else floor, FACTOR * e32)


# ---- input builders: deterministic from a seed, each returns the inputs and the property it was built to have -----------------------------
def base_inputs(lens, heads, seed, dh=64):
    """plain randn q / k / v and dO"""
    g = torch.Generator().manual_seed(seed)
    ntok, hid = int(np.sum(lens)), heads * dh
    return torch.randn(ntok, 3 * hid, generator=g), torch.randn(ntok, hid, generator=g)


KAPPA = 16.0
SHIFT_COL = 5
GAMMAS = (0.0, 2.0, 8.0, 60.0, -60.0)          # at scale 0.125 and kappa 16: shifts of 0, -4, -16, -120, +120
GAMMAS_MODEST = (0.0, 2.0, 8.0)


def shifted(qkv, lens, heads, gammas=GAMMAS, scale=0.125, dh=64):
    """column SHIFT_COL of every head: each key gets the constant kappa, query i gets -gamma_i (gammas cycle over the rows of a sequence),
    so all scores of row i move by -gamma_i kappa scale and the probabilities do not move at all.  d(q) in that column is
    kappa scale sum_j dS_ij = 0 exactly.  -> (qkv, dict(shift [ntok] = the shift of each row's scores, cls [ntok] = index into gammas))"""
    x = qkv.clone()
    hid = heads * dh
    cls = torch.cat([torch.arange(int(L)) % len(gammas) for L in lens])
    gam = torch.tensor(gammas, dtype=x.dtype)[cls]
    for h in range(heads):
        x[:, h * dh + SHIFT_COL] = -gam
        x[:, hid + h * dh + SHIFT_COL] = KAPPA
    return x, dict(shift=(-gam * KAPPA * scale).to(f64), cls=cls, col=SHIFT_COL)


def late_max(qkv, lens, heads, scale=0.125, dh=64):
    """key rows scaled by a_j = max(12, 64 2^(-d_j / 8)), d_j = the key's distance from the END of the sequence where (seq + head) is even
    (magnitudes grow: a row's maximum arrives in the last tiles) and from its START where it is odd (they fall: the maximum settles in the
    first tile).  With q ~ N(0, 1) the scaled scores have standard deviation a_j >= 12: peaked probabilities.
    -> (qkv, dict(last, first = share of (row, head) pairs whose arg-max key lies in the last / first 32-key tile, std = of the scores))"""
    x = qkv.clone()
    hid = heads * dh
    n_last = n_first = n = 0
    sq = cnt = 0.0
    for s, h, r0, L in groups(lens, heads):
        d = torch.arange(L, dtype=x.dtype)
        d = (L - 1 - d) if (s + h) % 2 == 0 else d
        a = torch.clamp(64.0 * torch.exp2(-d / 8.0), min=12.0)
        x[r0:r0 + L, hid + h * dh:hid + (h + 1) * dh] *= a[:, None]
        S = (x[r0:r0 + L, h * dh:(h + 1) * dh].to(f64) @ x[r0:r0 + L, hid + h * dh:hid + (h + 1) * dh].to(f64).t()) * scale
        am = S.argmax(1)
        n_last += int((am >= (L - 1) // 32 * 32).sum())
        n_first += int((am < 32).sum())
        n += L
        sq += float((S * S).sum())
        cnt += L * L
    return x, dict(last=n_last / n, first=n_first / n, std=(sq / cnt) ** 0.5)


def ramp_v_and_dO(qkv, dO, lens, heads, dh=64):
    """V rows and dO rows scaled by 2^(t - 8) for key / query tile t (32 rows), ascending along even sequences and descending along odd
    ones: the bound the fp16 forms scale their score gradients with grows at every tile, in DQ through V and in DKV through dO.
    -> (qkv, dO, dict(factor [ntok]))"""
    x, g = qkv.clone(), dO.clone()
    hid = heads * dh
    fac = []
    for s, L in enumerate(lens):
        t = torch.arange(int(L)) // 32
        t = t if s % 2 == 0 else ((int(L) - 1) // 32 - t)
        fac.append(torch.exp2((t - 8).to(x.dtype)))
    fac = torch.cat(fac)
    x[:, 2 * hid:] *= fac[:, None]
    g *= fac[:, None]
    return x, g, dict(factor=fac)


def zero_rows(qkv, dO, lens, heads, dh=64):
    """a few token rows of q, of k and of v exactly zero (all heads) in every sequence long enough, and dO zero for the whole of sequence 1
    -> (qkv, dO, dict(q, k, v = token rows zeroed, zero_seq))"""
    x, g = qkv.clone(), dO.clone()
    hid = heads * dh
    r0 = row_starts(lens)
    rows = dict(q=[], k=[], v=[])
    for s, L in enumerate(lens):
        L = int(L)
        if L < 4:
            continue
        rows["q"] += [int(r0[s]) + 1, int(r0[s]) + L // 2]
        rows["k"] += [int(r0[s]), int(r0[s]) + L - 1]
        rows["v"] += [int(r0[s]) + 2, int(r0[s]) + L - 1]
    x[rows["q"], 0:hid] = 0.0
    x[rows["k"], hid:2 * hid] = 0.0
    x[rows["v"], 2 * hid:] = 0.0
    zs = 1 if len(lens) > 1 else None
    if zs is not None:
        g[int(r0[zs]):int(r0[zs]) + int(lens[zs])] = 0.0
    return x, g, dict(zero_seq=zs, **rows)


def fully_dropped_rows(keeps, lens, heads):
    """[(seq, head, query)] whose every key is dropped"""
    return [(s, h, int(i)) for s, h, _, L in groups(lens, heads) for i in np.nonzero(~keeps[(s, h)].any(1))[0]]


# the batches the GPU tests use (tests/test_attn_restate_host.py checks the builders' properties on exactly these)
LENS_SHORT, HEADS_SHORT = [1, 31, 32, 33, 63, 64, 65, 96], 2
LENS_LONG, HEADS_LONG = [255, 256, 257, 385, 511, 1], 1
LENS_SHIFT, HEADS_SHIFT = [33, 70, 129, 64], 2
LENS_LATE, HEADS_LATE = [512, 200, 97], 2
LENS_RAMP, HEADS_RAMP = [512, 512, 130], 1
LENS_DROP, HEADS_DROP = [1] * 24 + [2] * 8 + [3] * 4 + [33, 257], 2
DROP_SEED, DROP_STREAM = 1234, 5
