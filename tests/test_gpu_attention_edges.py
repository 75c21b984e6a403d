"""Fused attention kernels (csrc/attn.hip) at their edges: tile and workgroup tails, shifted softmax rows, maxima that arrive late,
operand scales that grow tile by tile, zero rows, dropout that empties a row, strided outputs -- against the fp64 statement of
tests/attn_restate.py, PER (sequence, head) block and per output.

Gate of every block and output: max(floor, 8 e32), e32 = the same metric of the statement run in torch fp32 on the CPU on the same inputs
(computed here, never from the kernel's output), floor = the project's fp32-grade numbers 2e-6 (O) / 5e-6 (gradients; lse: absolute).
FORM 2 (`amp`: one fp16 product) keeps its 3e-3 gate over the whole tensor.  tests/test_attn_restate_host.py checks on the host that
every builder's inputs have the property they are used for.

Every run also checks that 128 guard rows behind the last token of every output are untouched, that the padding rows of the statistics
buffers (lse, both planes, and delta) still hold the zeros they were prefilled with after each of the three passes, and the amax slot.

With VBG_ATTN_EDGES_OUT set, one line per case / form / output (kernel error, e32, gate) is appended to that file."""
import functools
import os

import numpy as np
import pytest
import torch

import attn_restate as A

pytestmark = pytest.mark.gpu

SCALE = 0.125
GUARD = 128
PAT32 = 0x7FC0DEAD          # guard pattern of the fp32 buffers (a NaN: a guard row that leaks into a result is seen, too)
PAT16 = 0x5A5A              # ... and of the 16-bit planes
PAD = 32                    # sentinel columns on either side of a strided view (case 6)


def _meta(lens, heads):
    from model.BERTgrid_generator import flash_tables
    from vbg import functions as Fn
    dev = torch.device("cuda")
    sl = np.asarray(lens, np.int64)
    row0, pad_off, ntok_pad, tok_pad, mask_off, mask_words, tasks = flash_tables(sl, heads)
    m = Fn.AttnMeta()
    m.nseq, m.heads, m.dh, m.maxlen, m.ntok = len(sl), heads, 64, int(sl.max()), int(sl.sum())
    m.lens = torch.from_numpy(sl).int().to(dev)
    m.seq_row0 = torch.from_numpy(row0).int().to(dev)
    m.pad_off = torch.from_numpy(pad_off).int().to(dev)
    m.tok_pad = torch.from_numpy(tok_pad).int().to(dev)
    m.mask_off = torch.from_numpy(mask_off).to(dev)
    m.tasks = torch.from_numpy(tasks.reshape(-1)).int().to(dev)
    m.ntok_pad, m.mask_words, m.ntasks = ntok_pad, mask_words, int(tasks.shape[0])
    return m, tok_pad, mask_off


def _guarded(rows, cols, dev, pad=0):
    """fp32 [rows + GUARD, cols + 2 pad] full of the guard pattern -> (whole buffer, the [rows, cols] view the kernels get)"""
    whole = torch.full((rows + GUARD, cols + 2 * pad), PAT32, dtype=torch.int32, device=dev).view(torch.float32)
    return whole, whole[:rows, pad:pad + cols]


def _untouched(whole, rows, cols, pad=0):
    w = whole.view(torch.int32)
    ok = bool((w[rows:] == PAT32).all())
    if pad:
        ok = ok and bool((w[:rows, :pad] == PAT32).all()) and bool((w[:rows, pad + cols:] == PAT32).all())
    return ok


def _drive(lens, heads, qkv, dO, p, form, strided=False):
    """the three passes through ops.attn as tests/test_gpu_attention.py::_run drives them -> dict(O, lse, dq, dk, dv, keeps, ks)"""
    from vbg import ops
    from vbg.lib import ATTN_DKV, ATTN_DQ, ATTN_FWD
    dev = torch.device("cuda")
    meta, tok_pad, mask_off = _meta(lens, heads)
    hid, ntok = heads * 64, meta.ntok
    pad = PAD if strided else 0
    slot_do = None
    if form == 0:
        pq, pdo = ops.split_planes(qkv.to(dev)), ops.split_planes(dO.to(dev))
    else:
        pq = ops.split_planes_pair(qkv.to(dev))
        slot_do = ops.amax(dO.to(dev))
        pdo = ops.split_planes_pair(dO.to(dev), amax_slot_=slot_do)
    masks = ops.attn_mask(meta, p, A.DROP_SEED, A.DROP_STREAM) if p > 0 else None
    Ow, O = _guarded(ntok, hid, dev, pad)
    Kw, kbar = _guarded(ntok, hid, dev, pad)
    Dw, dqkv = _guarded(ntok, 3 * hid, dev, pad)
    if strided:
        assert O.stride(0) != hid and dqkv.stride(0) != 3 * hid and O.stride(0) == kbar.stride(0)
    opl = ops.planes_empty(ntok + GUARD, hid, dev)
    oq = ops.pair_empty(ntok + GUARD, hid, dev)
    opl.buf.fill_(PAT16)
    oq.buf.fill_(PAT16)
    opl.rows = oq.rows = ntok
    stats = torch.zeros(3, heads, meta.ntok_pad, device=dev)          # (m, 1 / l, delta): zero in the padding rows, as the model's stat_pool
    lse, delta = stats[:2], stats[2]
    padpos = torch.ones(meta.ntok_pad, dtype=torch.bool)
    padpos[torch.from_numpy(tok_pad)] = False
    padpos = padpos.to(dev)

    def pads_zero():
        return bool((stats.view(torch.int32)[:, :, padpos] == 0).all())

    slot = ops.amax_slot(dev)
    if form == 2:
        ops.set_amp(True)
    try:
        ops.attn(meta, ATTN_FWD, pq, None, O, lse, None, masks, SCALE, p, kbar=kbar, out_planes=opl, out_pair=oq)
        assert pads_zero(), "FWD wrote a padding row of the statistics"
        ops.attn(meta, ATTN_DQ, pq, pdo, dqkv, lse, delta, masks, SCALE, p, kbar=kbar, o=O, out_amax=slot, do_amax=slot_do)
        assert pads_zero(), "DQ wrote a padding row of the statistics"
        ops.attn(meta, ATTN_DKV, pq, pdo, dqkv, lse, delta, masks, SCALE, p, out_amax=slot, do_amax=slot_do)
        assert pads_zero(), "DKV wrote a padding row of the statistics"
    finally:
        ops.set_amp(False)
    torch.cuda.synchronize()
    # ---- nothing behind the last token, nothing beside a strided view ---------------------------------------------------------------
    assert _untouched(Ow, ntok, hid, pad), "O: guard rows / sentinel columns written"
    assert _untouched(Kw, ntok, hid, pad), "kbar: guard rows / sentinel columns written"
    assert _untouched(Dw, ntok, 3 * hid, pad), "dqkv: guard rows / sentinel columns written"
    assert bool((opl.buf[:, ntok:] == PAT16).all()), "planes of O: guard rows written"
    assert bool((oq.buf[:, ntok:] == PAT16).all()), "fp16-pair planes of O: guard rows written"
    Oc, dc = O.contiguous(), dqkv.contiguous()
    finite = bool(torch.isfinite(Oc).all()) and bool(torch.isfinite(kbar).all()) and bool(torch.isfinite(dc).all()) and bool(torch.isfinite(stats).all())
    if finite:          # (a NaN fails the caller's gate with the figures printed; these three compare bit patterns)
        assert torch.equal(opl.buf[:, :ntok, :hid], ops.split_planes(Oc).buf[:, :, :hid]), "planes of O written by the forward kernel != split(O)"
        assert torch.equal(oq.buf[:, :ntok, :hid], ops.split_planes_pair(Oc).buf[:, :, :hid]), "fp16-pair planes of O != split_pair(O)"
        assert int(slot.max().item()) == int(dc.abs().max().view(torch.int32).item()), "amax slot != max |dqkv|"
    keeps = ks = None
    if p > 0:
        ks = ops.attn_keep_scale(p)
        mq, mk = masks[0].cpu().numpy().view(np.uint32), masks[1].cpu().numpy().view(np.uint32)
        keeps = A.keep_matrices(mq, mask_off, lens, heads)
        for (s, h), k in keeps.items():
            assert (k == A.keep_matrix(mk, int(mask_off[s]), h, lens[s]).T).all(), "the two mask orientations disagree"
    st = stats.cpu().double()
    tp = torch.from_numpy(tok_pad)
    m, il = st[0][:, tp], st[1][:, tp]
    d = dc.cpu()
    return dict(O=Oc.cpu(), dq=d[:, :hid], dk=d[:, hid:2 * hid], dv=d[:, 2 * hid:], lse=m - torch.log(il), il=il, finite=finite, keeps=keeps, ks=ks,
                slot=int(slot.max().item()))


# ---- the cases: name -> (lens, heads, qkv, dO, p); built once, with their fp64 / fp32 statements --------------------------------------------
def _build(name):
    if name == "len_short":
        lens, heads = A.LENS_SHORT, A.HEADS_SHORT
        return (lens, heads) + A.base_inputs(lens, heads, 11) + (0.0,)
    if name == "len_long":
        lens, heads = A.LENS_LONG, A.HEADS_LONG
        return (lens, heads) + A.base_inputs(lens, heads, 12) + (0.0,)
    if name in ("shift", "shift_modest", "shift_drop"):
        lens, heads = A.LENS_SHIFT, A.HEADS_SHIFT
        qkv, dO = A.base_inputs(lens, heads, 2)
        qkv, _ = A.shifted(qkv, lens, heads, A.GAMMAS_MODEST if name == "shift_modest" else A.GAMMAS)
        return lens, heads, qkv, dO, (0.1 if name == "shift_drop" else 0.0)
    if name == "late_max":
        lens, heads = A.LENS_LATE, A.HEADS_LATE
        qkv, dO = A.base_inputs(lens, heads, 3)
        return lens, heads, A.late_max(qkv, lens, heads)[0], dO, 0.0
    if name in ("ramp", "zero_rows", "zero_dO"):
        lens, heads = A.LENS_RAMP, A.HEADS_RAMP
        qkv, dO = A.base_inputs(lens, heads, 4)
        if name == "ramp":
            qkv, dO, _ = A.ramp_v_and_dO(qkv, dO, lens, heads)
        elif name == "zero_rows":
            qkv, dO, _ = A.zero_rows(qkv, dO, lens, heads)
        else:
            dO = torch.zeros_like(dO)
        return lens, heads, qkv, dO, 0.0
    if name in ("drop_0.1", "drop_0.5"):
        lens, heads = A.LENS_DROP, A.HEADS_DROP
        return (lens, heads) + A.base_inputs(lens, heads, 6) + (float(name[5:]),)
    if name == "strided":
        lens, heads = [33, 130, 4], 2
        return (lens, heads) + A.base_inputs(lens, heads, 7) + (0.0,)
    raise KeyError(name)


_case = functools.lru_cache(maxsize=None)(_build)
_REFS = {}


def _refs(name, keeps, ks):
    """(fp64 statement, fp32 restatement) of a case: computed once, shared by the forms (the keeps of a case are the same in every run)"""
    if name not in _REFS:
        lens, heads, qkv, dO, _ = _case(name)
        _REFS[name] = tuple(A.statement(qkv, dO, lens, heads, SCALE, keeps, ks if keeps is not None else 1.0, dtype=dt) for dt in (torch.float64, torch.float32))
    return _REFS[name]


def _note(line):
    print("attn_edges:", line)
    path = os.environ.get("VBG_ATTN_EDGES_OUT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _check(name, form, strided=False, floors=None):
    """floors: {output: floor} raised for this one case, derived at the caller"""
    lens, heads, qkv, dO, p = _case(name)
    r = _drive(lens, heads, qkv, dO, p, form, strided)
    r64, r32 = _refs(name, r["keeps"], r["ks"])
    bad = []
    for out in ("O", "dq", "dk", "dv"):
        ek, e32 = A.group_errs(r[out], r64[out], lens, heads), A.group_errs(r32[out], r64[out], lens, heads)
        if form == 2:
            den = float(r64[out].abs().max())
            if not bool(torch.isfinite(r[out]).all()):
                e = float("inf")
            elif den == 0.0:                                  # an all-zero reference must be met exactly
                e = 0.0 if float(r[out].abs().max()) == 0.0 else float("inf")
            else:
                e = A.global_err(r[out], r64[out])
            _note(f"{name} form {form} {out}: kernel {e:.3e} of the whole tensor (gate 3.0e-03); worst group {max(ek):.3e}, e32 {max(e32):.3e}")
            if not e < 3e-3:
                bad.append((out, e))
            continue
        gates = [A.gate(out, e, None if floors is None else floors.get(out)) for e in e32]
        i = int(np.argmax([a / g for a, g in zip(ek, gates)]))
        s, h, r0, L = A.groups(lens, heads)[i]
        extra = ""
        if ek[i] == float("inf"):
            extra = f"; max |kernel| of that group {float(r[out][r0:r0 + L, h * 64:(h + 1) * 64].abs().max()):.3e}, max |reference| {float(r64[out][r0:r0 + L, h * 64:(h + 1) * 64].abs().max()):.3e}"
        _note(f"{name} form {form} {out}: kernel {max(ek):.3e} (worst group), e32 {max(e32):.3e}; nearest its gate: seq {s} (L {L}) head {h} "
              f"kernel {ek[i]:.3e} e32 {e32[i]:.3e} gate {gates[i]:.3e}" + extra)
        bad += [(out, A.groups(lens, heads)[j][:2], ek[j], gates[j]) for j in range(len(ek)) if not ek[j] <= gates[j]]
    el = float((r["lse"] - r64["lse"]).abs().max())
    e32l = float((r32["lse"].double() - r64["lse"]).abs().max())
    gl = A.gate("lse", e32l)
    _note(f"{name} form {form} lse: kernel {el:.3e} absolute, e32 {e32l:.3e}, gate {gl:.3e}")
    if form != 2 and not el <= gl:
        bad.append(("lse", el, gl))
    assert r["finite"], ("not finite", name, form, bad)
    assert not bad, bad
    return r, r64


F01 = pytest.mark.parametrize("form", [0, 1])
F012 = pytest.mark.parametrize("form", [0, 1, 2])


@F012
@pytest.mark.parametrize("name", ["len_short", "len_long"])
def test_lengths(name, form):
    """1, 31 ... 96 (tile tails, nt = 1: nothing prefetched, odd and even nt on the two-stage ring) and 255 ... 511, 1 (the 128-row workgroup
    tail: waves whose own rows lie past the sequence)"""
    _check(name, form)


@F012
@pytest.mark.parametrize("name", ["shift", "shift_modest", "shift_drop"])
def test_softmax_shift(name, form):
    """rows whose scores all move by 0, -4, -16, -120 or +120 (`shift`, and `shift_drop` with dropout 0.1), or by 0 / -4 / -16 only
    (`shift_modest`): the probabilities do not move, so nothing may.  L = 33, 70, 129 have keys past L in their last tile, L = 64 has none.
    Before the tail-tile mask of the DQ pass (csrc/attn.hip) those pad keys carried the "probability" exp(-m) / l: inf once m < -88.7
    (FORM 0: NaN in delta', dQ and through delta in dK / dV), past fp16's range after the dS scaling for a few units already (FORM 1 / 2:
    inf times the zero K row = NaN) -- which `shift_modest` separates from the overflow of exp."""
    _check(name, form)


@F01
def test_late_maximum(form):
    """key magnitudes that grow (fall) along the sequence: the online softmax rescales its accumulators in the last tiles (`alpha != 1`)
    against peaked probabilities, or settles in the first.

    FORM 1, dV: its floor is raised for this case to ONE fp32 ulp of the largest scaled score, 2^-23 max |S| (max |S| from the fp64
    statement of the inputs: 2.5e2 here, floor 3.0e-5).  Derivation: the DKV pass recomputes P' = exp(S' - m) / l with m and l from the
    forward pass.  In FORM 0 both passes form S by the same six piece products in the same order -- S' = S bit for bit, the row's largest
    probability is exp(0) / l.  In FORM 1 the forward pass folds the 2^-11 into per-lane scaled query fragments (one accumulator) while
    DKV, its registers full, keeps the cross terms in an accumulator of their own and folds it behind the product: two roundings of the
    same sum that differ by up to an ulp of S, so P' = P exp(S' - S) carries the RELATIVE error scale ulp(S) ~ 2^-23 |S scale| --
    nothing at |S| ~ 3 (randn), 1e-5 at |S| ~ 2e2, and with probabilities this peaked one (query, key) pair makes up a dV row, so
    nothing averages it out.  The fp32 torch statement uses ONE S for m and for P and cannot show it; dQ and dK come from dS, whose
    cancellation dP - delta costs the yardstick the same order.  Measured (profiles/attn_edges.txt): dV 1.0e-5, e32 1.0e-6."""
    floors = None
    if form == 1:
        lens, heads, qkv, dO, _ = _case("late_max")
        smax = _refs("late_max", None, None)[0]["smax"]
        floors = {"dv": 2.0 ** -23 * smax}
        _note(f"late_max form 1 dv: floor raised to 2^-23 max |S| = {floors['dv']:.3e} (max |S| = {smax:.4e})")
    _check("late_max", form, floors=floors)


@F012
@pytest.mark.parametrize("name", ["ramp", "zero_rows", "zero_dO"])
def test_scale_ramps_and_zero_rows(name, form):
    """V and dO that double (halve) at every tile: the bound-driven rescale of the dS accumulators (FORM 1 / 2) at every tile of DQ and of
    DKV; all-zero rows of q, k, v (no row scaling) and a sequence whose dO is zero (its gradients must be zero exactly: the group metric);
    dO zero for the whole batch: the dS scale is never set (`esc == 0`), dqkv must be exactly zero and the amax slot with it"""
    r, _ = _check(name, form)
    if name == "zero_dO":
        for out in ("dq", "dk", "dv"):
            assert float(r[out].abs().max()) == 0.0, out
        assert r["slot"] == 0


@F01
@pytest.mark.parametrize("name", ["drop_0.1", "drop_0.5"])
def test_dropout_edges(name, form):
    """many sequences of 1 ... 3 tokens: query rows whose keys are ALL dropped give O = 0 exactly, and the gradients follow the reference"""
    r, _ = _check(name, form)
    lens, heads = A.LENS_DROP, A.HEADS_DROP
    dropped = A.fully_dropped_rows(r["keeps"], lens, heads)
    assert len(dropped) >= 1
    r0 = A.row_starts(lens)
    for s, h, i in dropped:
        assert float(r["O"][int(r0[s]) + i, h * 64:(h + 1) * 64].abs().max()) == 0.0, (s, h, i)


@F01
def test_leading_dimensions(form):
    """O, kbar and dqkv as column views of wider buffers (row strides hid + 64 and 3 hid + 64, O's equal to kbar's): the sentinel columns
    on both sides stay untouched and the results are those of the reference"""
    _check("strided", form, strided=True)


def test_max_len_513_is_an_argument_error():
    """the staged mask / statistics tables hold 16 tiles: a longer sequence is refused before any launch"""
    from vbg import ops
    from vbg.lib import ATTN_FWD, VbgError
    lens, heads = [513], 1
    meta, _, _ = _meta(lens, heads)
    dev = torch.device("cuda")
    qkv, _ = A.base_inputs(lens, heads, 8)
    Ow, O = _guarded(513, 64, dev)
    lse = torch.zeros(2, heads, meta.ntok_pad, device=dev)
    with pytest.raises(VbgError, match="vbg_attn failed: argument error"):
        ops.attn(meta, ATTN_FWD, ops.split_planes(qkv.to(dev)), None, O, lse, None, None, SCALE, 0.0)
    torch.cuda.synchronize()
    assert _untouched(Ow, 0, 64) and float(lse.abs().max()) == 0.0
