"""Host side of the frozen-BatchNorm epilogue (no GPU): the ABI of vbg_bn_epilogue and of the grown vbg_gemm_desc against the C
compiler, the switch with its environment parsing, and the routing predicate of ConvBnFn.forward as a pure function."""
import itertools
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_layouts_against_the_c_compiler(tmp_path):
    """offsetof / sizeof from gcc over include/vbg.h == the ctypes mirrors; every field in front of the new one keeps its offset (the
    epilogue is appended behind slab_stride), and a zeroed descriptor carries no epilogue"""
    import ctypes as C
    import shutil
    from vbg.lib import BnEpilogue, GemmDesc
    assert [n for n, _ in GemmDesc._fields_][-2:] == ["slab_stride", "bn"]
    assert GemmDesc.bn.offset == GemmDesc.slab_stride.offset + 8 and C.sizeof(GemmDesc) == GemmDesc.bn.offset + C.sizeof(BnEpilogue)
    assert C.sizeof(BnEpilogue) == 56 and BnEpilogue.relu.offset == 40 and BnEpilogue.amax.offset == 48
    assert not GemmDesc().bn.mean and GemmDesc().bn.relu == 0
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "vbg.h"', 'int main(void) {']
    pairs = (("vbg_bn_epilogue", BnEpilogue), ("vbg_gemm_desc", GemmDesc))
    for st, cls in pairs:
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
    for st, cls in pairs:
        assert got[(st, "sizeof")] == C.sizeof(cls), st
        for name, _ in cls._fields_:
            assert got[(st, name)] == getattr(cls, name).offset, (st, name)


def test_entry_point_is_declared_bound_and_rejects_null_arguments():
    from vbg import lib as L
    assert "vbg_conv3x3_bn" in L.SIGNATURES and hasattr(L.lib, "vbg_conv3x3_bn")
    assert L.lib.vbg_version() == 100
    f = L.lib.vbg_conv3x3_bn
    assert f(None, None, None, None, 1, 16, 16, 16, 128, 1, None, None, None, 1, 0, None, None) == -1          # no epilogue, no operands
    import ctypes as C
    assert f(None, None, None, None, 1, 16, 16, 16, 128, 1, None, None, None, 1, 0, C.byref(L.BnEpilogue()), None) == -1


def test_switch_and_environment():
    from vbg import ops
    assert ops.bn_epilogue_enabled() is False                       # off by default
    ops.set_bn_epilogue(True)
    try:
        assert ops.bn_epilogue_enabled() is True
    finally:
        ops.set_bn_epilogue(False)
    assert ops.bn_epilogue_enabled() is False
    code = "import sys; sys.path.insert(0, sys.argv[1]); from vbg import ops; print(int(ops.bn_epilogue_enabled()))"
    pkg = os.path.join(ROOT, "vibertgrid-pytorch_amd")
    for value, want in ((None, "0"), ("0", "0"), ("1", "1")):          # (read once, at import: a fresh interpreter each)
        env = {k: v for k, v in os.environ.items() if k != "VBG_BN_EPILOGUE"}
        if value is not None:
            env["VBG_BN_EPILOGUE"] = value
        got = subprocess.run([sys.executable, "-c", code, pkg], env=env, check=True, capture_output=True, text=True).stdout.strip()
        assert got == want, (value, got)


def test_routing_predicate():
    """fused exactly when: switch on, frozen statistics, no input needs a gradient, no SyncBatchNorm exchange"""
    from vbg import ops
    none = (False,) * 14
    for on, training, sync, nig in itertools.product((False, True), (False, True), (False, True),
                                                     (none, (True,) + none[1:], none[:1] + (True,) + none[2:], none[:6] + (True,) + none[7:])):
        want = on and not training and not sync and nig == none
        assert ops.bn_epilogue_route(training, nig, sync, on=on) is want, (on, training, sync, nig)
    # without `on` the predicate reads the switch
    assert ops.bn_epilogue_route(False, none, False) is False
    ops.set_bn_epilogue(True)
    try:
        assert ops.bn_epilogue_route(False, none, False) is True
        assert ops.bn_epilogue_route(True, none, False) is False
    finally:
        ops.set_bn_epilogue(False)
