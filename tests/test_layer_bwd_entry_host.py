"""The one-call encoder layer backward (include/vbg.h vbg_bert_layer_bwd, csrc/encoder.hip) without a GPU: the ctypes mirror of its
descriptor against the C compiler, every argument rule (an argument error is returned before the first launch, so none of these calls
touches a device), and the switch that selects the entry."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bwd_desc_offsets_against_the_c_compiler(tmp_path):
    """sizeof and every field offset of vbg_bert_layer_bwd_desc from gcc over include/vbg.h == the ctypes mirror"""
    from vbg.lib import BertLayerBwdDesc, PlanesRef
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    structs = (("vbg_bert_layer_bwd_desc", BertLayerBwdDesc), ("vbg_planes_ref", PlanesRef))
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "vbg.h"', 'int main(void) {']
    for st, cls in structs:
        src.append(f'printf("{st} sizeof %zu\\n", sizeof({st}));')
        for name, _ in cls._fields_:
            src.append(f'printf("{st} {name} %zu\\n", offsetof({st}, {name}));')
    src += ['return 0; }']
    cfile = tmp_path / "off.c"
    cfile.write_text("\n".join(src))
    exe = str(tmp_path / "off")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(cfile), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {(a, b): int(c) for a, b, c in (ln.split() for ln in out if ln)}
    for st, cls in structs:
        assert got[(st, "sizeof")] == C.sizeof(cls), st
        for name, _ in cls._fields_:
            assert got[(st, name)] == getattr(cls, name).offset, (st, name)


def test_bwd_entry_is_declared_and_bound():
    from vbg import lib as L
    assert "vbg_bert_layer_bwd" in L.SIGNATURES and hasattr(L.lib, "vbg_bert_layer_bwd")
    src = open(os.path.join(ROOT, "include", "vbg.h")).read()
    assert "int vbg_bert_layer_bwd(const vbg_bert_layer_bwd_desc* desc, void* stream);" in src


FAKE = 0x10000          # a non-NULL, 64 KB aligned address that is never dereferenced: every case below fails its argument check first
OPTIONAL = ("mask_q", "mask_k", "mask_off", "det_scratch", "det_ws")


def _complete():
    """a descriptor in which every mandatory operand is named (bert-base widths, 84 tokens) and the optional ones are absent"""
    from vbg.lib import BertLayerBwdDesc, PlanesRef
    d = BertLayerBwdDesc()
    for name, typ in BertLayerBwdDesc._fields_:
        if typ is C.c_void_p and name not in OPTIONAL:
            setattr(d, name, FAKE)
        elif typ is PlanesRef:
            r = getattr(d, name)
            r.buf, r.plane, r.ld = FAKE, 96 * 3072, 3072
    d.ntok, d.hidden, d.inter, d.heads = 84, 768, 3072, 12
    d.qdfo.ld = d.qdao.ld = 768
    d.qdqkv.ld = 2304
    d.form, d.form_attn = 1, 1
    d.tile_dh = d.tile_dx1 = d.tile_dctx = d.tile_dx = 128129
    d.cq_mul_dh, d.cq_mul_dctx = 1.13 * 1.01, 1.01
    d.ntasks, d.max_len, d.ntok_pad = 2, 42, 128
    d.attn_scale, d.keep_scale = 0.125, 1.0
    return d


def _call(d):
    from vbg.lib import lib
    return lib.vbg_bert_layer_bwd(C.byref(d), None)


def test_null_and_empty_descriptors_are_argument_errors():
    from vbg.lib import BertLayerBwdDesc, lib
    assert lib.vbg_bert_layer_bwd(None, None) == -1
    d = BertLayerBwdDesc()
    d.ntok, d.hidden, d.inter, d.heads = 128, 768, 3072, 12
    d.form, d.form_attn = 1, 1
    assert _call(d) == -1          # sizes but no operands: argument error, nothing launched


def _hidden_not_heads(d):
    d.heads = 11


def _hidden_not_256(d):
    d.hidden, d.heads = 640 + 64, 11          # 704 = 11 * 64, a multiple of 32 and not of 256
    d.qdfo.ld = d.qdao.ld = 704
    d.qdqkv.ld = 3 * 704


def _form_low(d):
    d.form = 0


def _form_high(d):
    d.form = 3


def _form_attn(d):
    d.form_attn = 0


def _det_without_scratch(d):
    d.deterministic = 1


def _det_without_ws(d):
    d.deterministic, d.det_scratch = 1, FAKE


def _masks_without_offsets(d):
    d.mask_q = d.mask_k = FAKE
    d.keep_scale = 1.25


def _one_mask(d):
    d.mask_q, d.mask_off = FAKE, FAKE


RULES = [_hidden_not_heads, _hidden_not_256, _form_low, _form_high, _form_attn, _det_without_scratch, _det_without_ws, _masks_without_offsets,
         _one_mask]


@pytest.mark.parametrize("breaker", RULES, ids=lambda f: f.__name__.lstrip("_"))
def test_argument_rules(breaker):
    d = _complete()
    breaker(d)
    assert _call(d) == -1


@pytest.mark.parametrize("slot", ["s_dy", "s_dfo", "s_dfo_ref", "s_dh", "s_dx1", "s_dao", "s_dao_ref", "s_dctx", "s_dqkv", "s_dx"])
def test_a_missing_amax_slot_is_an_argument_error(slot):
    d = _complete()
    setattr(d, slot, None)
    assert _call(d) == -1


@pytest.mark.parametrize("field", ["dy", "h", "kbar", "ln_ws", "delta", "dx1", "dqkv", "dx", "dbi", "dbqkv", "dwqkv", "l1_wo", "tasks"])
def test_a_missing_operand_is_an_argument_error(field):
    d = _complete()
    setattr(d, field, None)
    assert _call(d) == -1


@pytest.mark.parametrize("planes", ["pqkv", "qx", "qctx", "qx1", "qg", "wqkv_t", "wo_t", "wi_t", "wo2_t", "qdfo", "qdh", "qdao", "pdctx", "qdqkv"])
def test_a_missing_plane_tensor_is_an_argument_error(planes):
    d = _complete()
    getattr(d, planes).buf = None
    assert _call(d) == -1


def test_switch():
    """VBG_LAYER_BWD_ENTRY: on by default, read once at import, its own cell (VBG_LAYER_ENTRY is the forward's); a GEMM profiler hook
    keeps both halves on the per-launch path"""
    from vbg import ops
    was = ops._LAYER_BWD_ENTRY[0]
    try:
        ops.set_layer_bwd_entry(True)
        assert ops.layer_bwd_entry_ok() is True
        ops.set_layer_bwd_entry(False)
        assert ops._LAYER_BWD_ENTRY[0] is False and ops.layer_bwd_entry_ok() is False and ops._LAYER_ENTRY[0] is True
        ops.set_layer_bwd_entry(True)
        ops.set_gemm_profiler(object())
        try:
            assert ops.layer_bwd_entry_ok() is False and ops.layer_entry_ok() is False
        finally:
            ops.set_gemm_profiler(None)
        assert ops.layer_bwd_entry_ok() is True
    finally:
        ops.set_layer_bwd_entry(was)
    code = "import sys; sys.path.insert(0, sys.argv[1]); from vbg import ops; print(ops._LAYER_BWD_ENTRY[0] is False, ops._LAYER_ENTRY[0] is True)"
    pkg = os.path.join(ROOT, "vibertgrid-pytorch_amd")
    for value, want in ((None, "False True"), ("0", "True True"), ("1", "False True")):          # (a fresh interpreter each)
        env = {k: v for k, v in os.environ.items() if k not in ("VBG_LAYER_BWD_ENTRY", "VBG_LAYER_ENTRY")}
        if value is not None:
            env["VBG_LAYER_BWD_ENTRY"] = value
        got = subprocess.run([sys.executable, "-c", code, pkg], env=env, check=True, capture_output=True, text=True).stdout.strip()
        assert got == want, (value, got)


def test_route_bit():
    """_LayerRoute.entry_bwd: the all-pair backward with both LayerNorms' affine gradients sunk and a hidden size the bound kernels take,
    the switch on; independent of the forward's entry bit"""
    from vbg import functions as Fn, ops
    base = (768, 3072, 64, 512, 4128, True, True, True, None)
    cells = (ops._LAYER_ENTRY, ops._LAYER_BWD_ENTRY, ops._PAIR_BWD)
    saved = [c[0] for c in cells]
    try:
        ops._LAYER_ENTRY[0], ops._LAYER_BWD_ENTRY[0], ops._PAIR_BWD[0] = True, True, True
        r = Fn._layer_route(*base, ln_sunk=True)
        assert r.pair_bwd and r.entry and r.entry_bwd
        assert not Fn._layer_route(*base).entry_bwd and not Fn._layer_route(*base, ln_sunk=False).entry_bwd
        assert not Fn._layer_route(*((704,) + base[1:]), ln_sunk=True).entry_bwd                      # hidden % 256 != 0
        assert not Fn._layer_route(*(base[:7] + (False, None)), ln_sunk=True).entry_bwd               # not the all-pair backward
        ops._LAYER_ENTRY[0] = False
        r = Fn._layer_route(*base, ln_sunk=True)
        assert not r.entry and r.entry_bwd
        ops._LAYER_ENTRY[0], ops._LAYER_BWD_ENTRY[0] = True, False
        r = Fn._layer_route(*base, ln_sunk=True)
        assert r.entry and not r.entry_bwd
        ops._LAYER_BWD_ENTRY[0], ops._PAIR_BWD[0] = True, False
        assert not Fn._layer_route(*base, ln_sunk=True).entry_bwd
    finally:
        for c, v in zip(cells, saved):
            c[0] = v


def test_amax_slots_come_from_the_pools_and_cross_them():
    from vbg import ops
    import torch
    dev = torch.device("cpu")
    was = ops._AMAX_POOL_SLOTS[0]
    ops._AMAX_POOL.clear()
    ops._AMAX_POOL_SLOTS[0] = 4
    try:
        first = ops.amax_slot(dev)
        first[0] = 7
        nine = ops.amax_slots(dev, 9)
        assert len(nine) == 9 and all(s.shape == first.shape and s.dtype == torch.int32 and int(s.abs().max()) == 0 for s in nine)
        ptrs = [s.data_ptr() for s in nine] + [first.data_ptr()]
        assert len(set(ptrs)) == 10                                                # distinct slots, none handed out twice
        assert nine[0].data_ptr() == first.data_ptr() + 4 * first.numel()          # the rest of the current pool first ...
        assert len({s.untyped_storage().data_ptr() for s in nine}) == 3            # ... then fresh pools: 3 + 4 + 2
        nxt = ops.amax_slot(dev)
        assert nxt.data_ptr() == nine[8].data_ptr() + 4 * first.numel() and int(first[0]) == 7          # never rewound
    finally:
        ops._AMAX_POOL_SLOTS[0] = was
        ops._AMAX_POOL.clear()
