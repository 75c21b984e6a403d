"""Device sampling without a GPU: the switch and the seed rule of vbg.ops, and the argument checks of the new entry points (they
come before any launch)."""
import torch

import sample_restate as S


def test_switch_defaults_off_and_toggles():
    from vbg import ops
    assert ops.device_sampling_enabled() is False
    ops.set_device_sampling(True)
    try:
        assert ops.device_sampling_enabled() is True
    finally:
        ops.set_device_sampling(False)


def test_seed_rule_and_counter():
    from vbg import ops
    state = torch.random.get_rng_state()
    try:
        torch.manual_seed(0x1_2345_6789)
        ops.reset_sample_counter()
        assert ops.next_sample_seed() == S.step_seed(0, 0x1_2345_6789) == 0x23456789
        assert ops.next_sample_seed() == 0x9E3779B1 + 0x23456789
        ops.reset_sample_counter(7)
        assert ops.next_sample_seed() == S.step_seed(7, 0x1_2345_6789)
        assert ops.SAMPLE_STREAM0 == S.STREAM0 == 0x10000
    finally:
        ops.reset_sample_counter()
        torch.random.set_rng_state(state)


def test_argument_errors_do_not_need_a_gpu():
    from vbg import lib as L
    sc = L.SampleCats()
    sc.c[0].k = 4
    f = L.lib.vbg_sample_select
    assert L.lib.vbg_sample_ws_bytes(1000, 2, 8) == (4 * 2048 + 64 + 2 * 1000) * 4          # a function of N and ncat only
    assert L.lib.vbg_sample_ws_bytes(10, 5, 4) < 0 and L.lib.vbg_sample_ws_bytes(-1, 1, 4) < 0
    assert f(None, 64, 1, sc, 1, 0, None, None, None, None, 1 << 30, None) == -1             # null outputs
    assert f(None, 64, 5, sc, 1, 0, None, None, None, None, 1 << 30, None) == -1             # more than 4 categories
    assert f(None, 2 ** 31, 1, sc, 1, 0, None, None, None, None, 1 << 40, None) == -1        # N >= 2^31
    sc.c[0].k = 0
    assert f(None, 64, 1, sc, 1, 0, None, None, None, None, 1 << 30, None) == -1             # k <= 0
    oc = L.OhemCats()
    oc.c[0].cap, oc.c[0].k = 4097, 8
    assert L.lib.vbg_ohem_topk(None, 2, 2, None, None, 1, oc, None, None, 0, 0, 0, None, None, None) == -1
    assert L.lib.vbg_ce_fwd_dyn(None, 2, 2, None, None, 8, None, None, 0, 0, 0, None, None) == -1          # no device count
    assert L.lib.vbg_ce_bwd_dyn(None, 2, 2, None, None, 8, None, None, None, 1.0, 0, 0, 0, None, None) == -1
