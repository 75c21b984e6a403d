"""Deterministic mode, host side: the switch (environment, latching, scope restore) and the argument checks of the fixed-order entry
points, which reject bad calls before any launch (no GPU needed)."""
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "vibertgrid-pytorch_amd")


def _env_value(v):
    env = dict(os.environ)
    env.pop("VBG_DETERMINISTIC", None)
    if v is not None:
        env["VBG_DETERMINISTIC"] = v
    code = f"import sys; sys.path.insert(0, {PKG!r}); from vbg import ops; print(int(ops.deterministic()), int(ops.deterministic_active()))"
    return subprocess.check_output([sys.executable, "-c", code], env=env, text=True).split()


def test_env_switch():
    assert _env_value(None) == ["0", "0"]
    assert _env_value("0") == ["0", "0"]
    assert _env_value("") == ["0", "0"]
    assert _env_value("1") == ["1", "1"]


def test_scope_restores_and_latch_follows_torch_flag():
    from vbg import ops
    prev_user, prev_det = ops._DET_USER[0], ops._DET[0]
    prev_flag = torch.are_deterministic_algorithms_enabled()
    try:
        ops.set_deterministic(False)
        assert not ops.deterministic() and not ops.deterministic_active()
        with ops.deterministic_scope(True):
            assert ops.deterministic() and ops.deterministic_active()
            with ops.deterministic_scope(False):
                assert not ops.deterministic_active()
            assert ops.deterministic_active()
        assert not ops.deterministic() and not ops.deterministic_active()
        torch.use_deterministic_algorithms(True)
        assert ops.deterministic()
        ops.latch_deterministic()
        assert ops.deterministic_active()
        torch.use_deterministic_algorithms(False)
        ops.latch_deterministic()
        assert not ops.deterministic_active()
        ops.set_deterministic(True)
        ops.latch_deterministic()
        assert ops.deterministic_active()
    finally:
        torch.use_deterministic_algorithms(prev_flag)
        ops._DET_USER[0], ops._DET[0] = prev_user, prev_det


def test_autograd_functions_pin_the_mode():
    """the backward of a forward sees the mode that forward ran with (vbg/functions.py _pin_arithmetic)"""
    from vbg import functions, ops

    class Probe(torch.autograd.Function):
        seen = []

        @staticmethod
        def forward(ctx, x):
            return x * 2

        @staticmethod
        def backward(ctx, g):
            Probe.seen.append(ops.deterministic_active())
            return g * 2

    functions._pin_arithmetic(Probe)
    prev = (ops._DET_USER[0], ops._DET[0])
    try:
        x = torch.ones(3, requires_grad=True)
        with ops.deterministic_scope(True):
            y = Probe.apply(x).sum()
        assert not ops.deterministic_active()
        y.backward()
        assert Probe.seen == [True] and not ops.deterministic_active()
    finally:
        ops._DET_USER[0], ops._DET[0] = prev


def test_argument_errors_without_a_launch():
    from vbg import lib as L
    lib = L.lib
    assert lib.vbg_colsum_det(None, 4, 8, 4, None, 0, None, None) == -1
    assert lib.vbg_colsum_det(None, 2, 8, 4, None, 0, None, None) == -1          # ld < N
    assert lib.vbg_sum_det(None, 10, 0, None, None, None) == -1
    assert lib.vbg_sort_i32(None, 10, None, None, None, 0, None) == -1
    assert lib.vbg_sort_i32(None, 0, None, None, None, 0, None) == 0              # empty: nothing to do
    assert lib.vbg_segment_rows_add(None, 4, None, None, 3, 8, None, 8, None) == -1   # lds < C
    assert lib.vbg_segment_rows_add(None, 8, None, None, 0, 8, None, 8, None) == 0
    assert lib.vbg_ce_bwd_rows(None, 4, 4, None, None, 5, None, None, 1.0, 0, 0, 0, None, None, None) == -1
    assert lib.vbg_roi_align_bwd_det(None, 1, 8, 8, 4, None, None, 1, 7, 0.25, None, None) == -1
    assert lib.vbg_roi_align_bwd_det(1, 1, 8, 8, 4, 1, 1, 1, 9, 0.25, 1, None) == -1      # out > 8
    assert lib.vbg_roi_align_bwd_det(1, 1, 8, 4096, 4, 1, 1, 1, 7, 0.25, 1, None) == -1   # weight table beyond LDS
    assert lib.vbg_bn_stats_det(None, 8, 64, None, None, None) == -1
    assert lib.vbg_bn_bwd_reduce_det(None, None, None, 8, 64, None, None, 0, None, None, None) == -1
    assert lib.vbg_bn_det_ws_rows(0, 64) == 0 and lib.vbg_bn_det_ws_rows(8, 6) == 0 and lib.vbg_bn_det_ws_rows(524288, 64) >= 32
    assert lib.vbg_embed_ln_bwd_det(None, None, None, 4, 64, None, 0.0, 0, 0, None, None, None) == -1
    assert lib.vbg_crf_nll_bwd_det(None, None, None, 1, None, 4, 0, 1, None, None, None, None, None, None) == -1
    assert lib.vbg_embed_ln_bwd_det_blocks(0) == 0 and lib.vbg_embed_ln_bwd_det_blocks(17) == 2
    assert lib.vbg_colsum_det_ws_elems(0, 8) == 8 and lib.vbg_colsum_det_ws_elems(10 ** 7, 8) == 256 * 8
    assert lib.vbg_sum_det_ws_elems() == 256
