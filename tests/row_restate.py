"""The encoder's row kernels restated in plain numpy / torch fp64, independent of the library (no import of vbg).

Dropout RNG (csrc/vbg_common.h rng_u32): a splitmix64-style finaliser over 64-bit wrap-around arithmetic,
    z = seed + 0x9E3779B97F4A7C15 (sid + 1) + idx 0xBF58476D1CE4E5B9;  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;
    z *= 0x94D049BB133111EB;  z ^= z >> 31;  draw = (z >> 16) mod 2^32;  keep <=> draw >= uint32(double(float32(p)) 2^32).
Element (t, c) of a [rows, hidden] tensor draws index t * hidden + c, in the LayerNorm kernels (x before the residual is added), in the
embedding kernels (the LayerNorm's output) and in both backward passes.  Kept values are scaled by keep_scale(p) = 1 / (1 - p) computed
in fp32 -- an fp32 INPUT of the operation here, so the fp64 statements below use that rounded value exactly.

Attention dropout (csrc/attn.hip attn_mask_kernel): group g = seq * heads + head, query q, 32-key block kb draw eight hashes of index
(((g maxlen + q) ceil(maxlen / 32) + kb) 8 + c; bit 4c + e of the word is (16-bit slice e of hash c) >= thr16(p).  mask_q[off + q nkb +
kb] holds the keys 32 kb ... 32 kb + 31 of query q, mask_k[off + key nkb + qb] the queries 32 qb ... of that key (the same bits,
transposed); off = mask_off[seq] + head * 32 nkb * nkb, nkb = ceil(len / 32).

LayerNorm: z = keep x keep_scale + res, xhat = (z - mean z) rstd, rstd = 1 / sqrt(var z + eps) (biased variance), y = xhat gamma + beta.
Backward from (xhat, rstd) AS GIVEN: dz = rstd (g gamma - mean(g gamma) - xhat mean(g gamma xhat)), dx = keep dz keep_scale, dres = dz,
dgamma = sum_t g xhat, dbeta = sum_t g.  The embedding form gathers word[ids] + type0 + pos[pid], normalises, and drops the OUTPUT."""
import numpy as np
import torch

U64 = np.uint64
f64 = torch.float64
_K0, _K1, _K2 = U64(0x9E3779B97F4A7C15), U64(0xBF58476D1CE4E5B9), U64(0x94D049BB133111EB)


def _u64(v):
    """python int / array -> uint64 array (values taken mod 2^64)"""
    if isinstance(v, (int, np.integer)):
        return np.asarray(int(v) & 0xFFFFFFFFFFFFFFFF, dtype=U64)
    return np.asarray(v).astype(U64)


def rng_state(seed, sid, idx):
    """the finalised 64-bit hash of (seed, stream, index); every argument an int or an array (broadcast)"""
    with np.errstate(over="ignore"):
        z = _u64(seed) + _K0 * (_u64(sid) + U64(1)) + _u64(idx) * _K1
        z = z ^ (z >> U64(30))
        z = z * _K1
        z = z ^ (z >> U64(27))
        z = z * _K2
        z = z ^ (z >> U64(31))
    return z


def rng_u32(seed, sid, idx):
    return ((rng_state(seed, sid, idx) >> U64(16)) & U64(0xFFFFFFFF)).astype(np.uint32)


def drop_threshold(p):
    t = float(np.float32(p)) * 4294967296.0
    if t <= 0:
        return 0
    if t >= 4294967295.0:
        return 4294967295
    return int(t)


def thr16(p):
    t = float(np.float32(p)) * 65536.0 + 0.5
    return int(min(max(t, 0.0), 65535.0))


def keep_scale(p):
    """1 / (1 - p) as the kernels' callers compute it: in fp32"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def keep_mask(seed, sid, rows, hidden, p):
    """bool [rows, hidden]: element (t, c) is kept iff the draw of index t * hidden + c reaches the threshold"""
    thr = drop_threshold(p)
    idx = np.arange(rows * hidden, dtype=U64)
    return (rng_u32(seed, sid, idx) >= np.uint32(thr)).reshape(rows, hidden)


# ---- attention dropout words ---------------------------------------------------------------------------------------------------------
def attn_mask_words(lens, mask_off, heads, maxlen, p, seed, sid):
    """-> (mask_q, mask_k, defined): uint32 word arrays as attn_mask_kernel writes them and the (sorted) indices of the words it defines
    -- every (q < 32 nkb, kb < nkb) of every (sequence, head); all other words are left zero here and uninitialised by the kernel"""
    lens = np.asarray(lens, np.int64)
    mask_off = np.asarray(mask_off, np.int64)
    nkb_all = (lens + 31) // 32
    total = int((mask_off + heads * 32 * nkb_all * nkb_all).max()) if lens.size else 0
    mq, mk = np.zeros(total, np.uint32), np.zeros(total, np.uint32)
    defined = []
    t16 = U64(thr16(p))
    mkb = (int(maxlen) + 31) // 32
    sh16 = (U64(16) * np.arange(4, dtype=U64))
    wbit = (np.uint32(1) << np.arange(32, dtype=np.uint32))
    for nkb in np.unique(nkb_all):
        nkb = int(nkb)
        if nkb == 0:
            continue
        seqs = np.nonzero(nkb_all == nkb)[0]
        Q = 32 * nkb
        per = max(1, (1 << 18) // (heads * Q * nkb))                    # sequences per batch: <= 2^21 hashes at a time
        for s0 in range(0, len(seqs), per):
            ss = seqs[s0:s0 + per]
            g = (ss[:, None] * heads + np.arange(heads)[None, :]).astype(np.int64)                       # [S, heads]
            q = np.arange(Q, dtype=np.int64)
            kb = np.arange(nkb, dtype=np.int64)
            idx0 = ((g[:, :, None, None] * int(maxlen) + q[None, None, :, None]) * mkb + kb[None, None, None, :]) * 8
            z = rng_state(seed, sid, (idx0[..., None] + np.arange(8)).astype(U64))                        # [S, heads, Q, nkb, 8]
            keep = (((z[..., None] >> sh16) & U64(0xFFFF)) >= t16).reshape(len(ss), heads, Q, nkb, 32)   # bit 4c + e
            wq = (keep * wbit).sum(-1, dtype=np.uint64).astype(np.uint32)                                # [S, heads, Q, nkb]
            K = keep.reshape(len(ss), heads, Q, Q)                                                       # [.., query, key]
            kt = K.transpose(0, 1, 3, 2).reshape(len(ss), heads, Q, nkb, 32)                             # [.., key, qb, i]
            wk = (kt * wbit).sum(-1, dtype=np.uint64).astype(np.uint32)                                  # [S, heads, key, nkb]
            base = mask_off[ss][:, None] + np.arange(heads)[None, :] * (Q * nkb)                          # [S, heads]
            pos = (base[:, :, None] + np.arange(Q * nkb)[None, None, :]).reshape(-1)
            mq[pos] = wq.reshape(-1)
            mk[pos] = wk.reshape(-1)
            defined.append(pos)
    defined = np.sort(np.concatenate(defined)) if defined else np.zeros(0, np.int64)
    return mq, mk, defined


# ---- LayerNorm in fp64 -----------------------------------------------------------------------------------------------------------------
def _drop(v, keep, p):
    """keep * v * keep_scale(p) with dropped positions contributing exactly nothing (whatever they hold)"""
    if keep is None:
        return v
    return torch.where(torch.as_tensor(keep), v * keep_scale(p), torch.zeros((), dtype=v.dtype))


def ln_fwd(x, res, gamma, beta, eps, keep=None, p=0.0):
    """-> (y, xhat, rstd) in fp64 of LN(keep x keep_scale + res)"""
    z = _drop(x.to(f64), keep, p)
    if res is not None:
        z = z + res.to(f64)
    mean = z.mean(1, keepdim=True)
    var = ((z - mean) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (z - mean) * rstd
    return xhat * gamma.to(f64) + beta.to(f64), xhat, rstd[:, 0]


def ln_bwd(g, xhat, rstd, gamma, keep=None, p=0.0):
    """backward of ln_fwd from xhat and rstd as given -> dict(dz, dx, dgamma, dbeta, dbias) (+ the column sums of |term| of the three
    column quantities as a_dgamma, a_dbeta, a_dbias: the scale a column's rounding error is measured against)"""
    g, xhat, rstd, gam = g.to(f64), xhat.to(f64), rstd.to(f64), gamma.to(f64)
    gg = g * gam
    m1 = gg.mean(1, keepdim=True)
    m2 = (gg * xhat).mean(1, keepdim=True)
    dz = rstd[:, None] * (gg - m1 - xhat * m2)
    dx = _drop(dz, keep, p)
    return dict(dz=dz, dx=dx, dgamma=(g * xhat).sum(0), dbeta=g.sum(0), dbias=dx.sum(0),
                a_dgamma=(g * xhat).abs().sum(0), a_dbeta=g.abs().sum(0), a_dbias=dx.abs().sum(0))


def embed_fwd(ids, pid, word, pos, type0, gamma, beta, eps, keep=None, p=0.0):
    """-> (out, xhat, rstd): dropout(LN(word[ids] + type0 + pos[pid]))"""
    x = word.to(f64)[ids.long()] + type0.to(f64) + pos.to(f64)[pid.long()]
    y, xhat, rstd = ln_fwd(x, None, gamma, beta, eps)
    return _drop(y, keep, p), xhat, rstd


def embed_bwd(dout, xhat, rstd, ids, pid, gamma, nword, npos, keep=None, p=0.0):
    """backward of embed_fwd from xhat and rstd as given: the table gradients are index_add_ scatters of dz in fp64
    -> dict(dword, dpos, dtype0, dgamma, dbeta) + a_* = the same sums over |term|"""
    g = _drop(dout.to(f64), keep, p)
    r = ln_bwd(g, xhat, rstd, gamma)
    dz, hidden = r["dz"], xhat.shape[1]
    out = dict(dgamma=r["dgamma"], dbeta=r["dbeta"], a_dgamma=r["a_dgamma"], a_dbeta=r["a_dbeta"], dtype0=dz.sum(0), a_dtype0=dz.abs().sum(0))
    for name, n, ix in (("dword", nword, ids), ("dpos", npos, pid)):
        out[name] = torch.zeros(n, hidden, dtype=f64).index_add_(0, ix.long(), dz)
        out["a_" + name] = torch.zeros(n, hidden, dtype=f64).index_add_(0, ix.long(), dz.abs())
    return out


# ---- error metrics ---------------------------------------------------------------------------------------------------------------------
def row_err(got, ref):
    """row tensors: max |error| of a row over max |reference| of that row, maximised over rows"""
    got, ref = got.detach().cpu().to(f64), ref.detach().cpu().to(f64)
    den = ref.abs().amax(1)
    num = (got - ref).abs().amax(1)
    return float((num / torch.where(den > 0, den, torch.ones_like(den))).max()) if ref.numel() else 0.0


def col_err(got, ref, asum):
    """column sums: |error| over the sum of |term| of that column, maximised over columns (any leading shape: table rows count as columns)"""
    got, ref, asum = got.detach().cpu().to(f64).reshape(-1), ref.detach().cpu().to(f64).reshape(-1), asum.detach().cpu().to(f64).reshape(-1)
    num = (got - ref).abs()
    return float((num / torch.where(asum > 0, asum, torch.ones_like(asum))).max()) if ref.numel() else 0.0


def gate(e_ref):
    """the kernel's gate from the yardstick's error: four times torch's fp32 error on the same inputs (another order of the same fp32
    sums), and never below eight fp32 roundings"""
    return max(4.0 * e_ref, 8.0 * 2.0 ** -24)


# (seed, sid, rows, hidden, p) of the GPU tests that pin the dropout bits (tests/test_gpu_row_kernels.py); the last is the embedding form.
# tests/test_row_restate_host.py checks the keep rate of each: change a seed and that check runs on the new one
DROPOUT_CASES = [(123, 7, 130, 768, 0.1), (5, 3, 515, 256, 0.1), (11, 2, 2051, 1024, 0.5), (9, 1, 77, 1000, 0.1)]
