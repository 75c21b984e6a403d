"""The unfused attention route (ops.attn_unfused_fwd / attn_unfused_bwd: grouped GEMMs around the row softmax of csrc/rowops.hip) -- what
an encoder layer runs when vbg.ops.flash_ok is false, i.e. head size != 64 or a sequence past 512 -- against the fp64 statement of
tests/attn_restate.py with the per-(sequence, head) metric and gates of tests/test_gpu_attention_edges.py: max(floor, 8 e32) per block
and output, e32 = the statement in torch fp32 on the CPU on the same inputs.  The dropout keeps are read from the sign of the stored
probabilities (sign bit = dropped: include/vbg.h vbg_softmax_fwd)."""
import numpy as np
import pytest
import torch

import attn_restate as A
from test_gpu_attention_edges import GUARD, _guarded, _note, _untouched

pytestmark = pytest.mark.gpu


def _meta(lens, heads, dh):
    from model.BERTgrid_generator import attention_tables
    from vbg import functions as Fn
    dev = torch.device("cuda")
    sl = np.asarray(lens, np.int64)
    tabs, soff, s_elems, maxlen, ld = attention_tables(sl, heads, dh, heads * dh)
    m = Fn.AttnMeta()
    m.ntok, m.nseq, m.heads, m.dh, m.maxlen, m.ld, m.s_elems = int(sl.sum()), len(sl), heads, dh, maxlen, ld, s_elems
    m.ngroups = len(sl) * heads
    m.soff = torch.from_numpy(soff.astype(np.int64)).to(dev)
    m.lens = torch.from_numpy(sl).int().to(dev)
    m.ldp = torch.full((len(sl),), ld, dtype=torch.int32, device=dev)
    m.t_qk, m.t_pv, m.t_dp, m.t_dv, m.t_dq = (torch.from_numpy(tabs[k].reshape(-1).astype(np.int64)).to(dev) for k in ("qk", "pv", "dp", "dv", "dq"))
    m.t_dk = m.t_dq
    return m, soff, ld


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("lens,heads,dh", [([513, 7, 130], 2, 64), ([40, 5], 2, 32)])
def test_unfused_attention_vs_fp64(lens, heads, dh, p):
    """513: the first length past the fused kernels' limit (the row softmax then holds 16 elements per lane instead of 8); head size 32"""
    from vbg import ops
    dev = torch.device("cuda")
    assert not ops.flash_ok(heads * dh, 4 * heads * dh, dh, max(lens))
    meta, soff, ld = _meta(lens, heads, dh)
    hid, ntok = heads * dh, meta.ntok
    scale = 1.0 / (dh ** 0.5)
    qkv, dO = A.base_inputs(lens, heads, 21, dh)
    qd = qkv.to(dev)
    Pw = torch.full((meta.s_elems + GUARD,), 0x7FC0DEAD, dtype=torch.int32, device=dev).view(torch.float32)
    P = Pw[:meta.s_elems]
    Cw, ctxv = _guarded(ntok, hid, dev)
    ops.attn_unfused_fwd(meta, qd, P, ctxv, p, A.DROP_SEED, A.DROP_STREAM)
    dqkv = ops.attn_unfused_bwd(meta, qd, P, dO.to(dev), p)
    torch.cuda.synchronize()
    assert _untouched(Cw, ntok, hid) and bool((Pw.view(torch.int32)[meta.s_elems:] == 0x7FC0DEAD).all()), "written past the end"
    assert torch.equal(qd.cpu(), qkv), "the backward pass changed its input"
    Pc = P.cpu()
    keeps = ks = None
    if p > 0:
        ks = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))          # as rowops.hip and the GEMM descriptor hold it: fp32
        keeps = {}
    for g, (s, h, r0, L) in enumerate(A.groups(lens, heads)):
        blk = Pc[int(soff[g]):int(soff[g]) + L * ld].view(L, ld)
        assert float(blk[:, L:].abs().sum()) == 0.0, "pad columns of P"
        if p > 0:
            keeps[(s, h)] = (~torch.signbit(blk[:, :L])).numpy()
    if p > 0:
        rate = np.mean([k.mean() for (s, h), k in keeps.items() if lens[s] >= 40])
        assert abs(rate - (1.0 - p)) < 0.02, rate
    r64, r32 = (A.statement(qkv, dO, lens, heads, scale, keeps, ks if p > 0 else 1.0, dtype=dt, dh=dh) for dt in (torch.float64, torch.float32))
    d = dqkv.cpu()
    got = dict(O=ctxv.cpu(), dq=d[:, :hid], dk=d[:, hid:2 * hid], dv=d[:, 2 * hid:])
    bad = []
    for out in ("O", "dq", "dk", "dv"):
        ek, e32 = A.group_errs(got[out], r64[out], lens, heads, dh), A.group_errs(r32[out], r64[out], lens, heads, dh)
        gates = [A.gate(out, e) for e in e32]
        i = int(np.argmax([a / g for a, g in zip(ek, gates)]))
        s, h, _, L = A.groups(lens, heads)[i]
        _note(f"unfused {lens} dh {dh} p {p} {out}: kernel {max(ek):.3e} (worst group), e32 {max(e32):.3e}; nearest its gate: seq {s} (L {L}) head {h} "
              f"kernel {ek[i]:.3e} e32 {e32[i]:.3e} gate {gates[i]:.3e}")
        bad += [(out, A.groups(lens, heads)[j][:2], ek[j], gates[j]) for j in range(len(ek)) if not ek[j] <= gates[j]]
    assert not bad, bad
