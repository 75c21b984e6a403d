"""ConvFn / ConvBnFn against tests/golden/conv_bits.npz: the bits of every output and gradient in deterministic mode, and the kernel
families taken (ops.dispatch_log) in both modes, as recorded on an MI355X by the commit before the nodes took their routing from
vbg.ops.ConvPlan (tests/golden/make_golden_conv_bits.py holds the cases and replays them here).  Values of the default mode, whose
BatchNorm statistics are added with float atomics, stay with tests/test_gpu_kernels.py."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_golden_conv_bits as M          # noqa: E402

sys.path.remove(GOLDEN)


@pytest.fixture(scope="module")
def fix(golden):
    return M.load(golden("conv_bits.npz"))


def test_the_fixture_holds_every_case(fix):
    ids = [c[0] for c in M.case_ids()]
    assert len(ids) == len(M.SHAPES) * (1 + len(M.BN_CASES) + len(M.EPI_CASES)) and sorted(fix) == sorted(ids)
    assert all("y" in fix[cid][0] for cid in ids)
    # every tensor the generator names is recorded where the case has it
    assert set(fix["wide256/bn/train/res1/relu1"][0]) == set(M.TENSORS) - {"db"} and "db" in fix["wide256/conv"][0]


def test_the_shapes_reach_their_routes():
    from vbg import ops
    assert all(M.routes(ops).values()), M.routes(ops)


@pytest.mark.parametrize("name", list(M.SHAPES))
def test_bits_and_dispatch(fix, name):
    from vbg import functions as Fn
    from vbg import ops
    dev = torch.device("cuda")
    src = M.inputs(name)
    for cid, shape, kind, args in M.case_ids():
        if shape != name:
            continue
        want, want_det, want_default = fix[cid]
        with ops.deterministic_scope(True):
            got, log = M.run_case(ops, Fn, dev, src, name, kind, args)
        assert log == want_det, (cid, log)
        assert sorted(got) == sorted(want), cid
        for t, (sha, samples) in got.items():
            assert np.array_equal(samples, want[t][1]), (cid, t, samples.view(np.float32), want[t][1].view(np.float32))
            assert sha == want[t][0], (cid, t)
        with ops.deterministic_scope(False):
            _, log = M.run_case(ops, Fn, dev, src, name, kind, args)
        assert log == want_default, (cid, log)
