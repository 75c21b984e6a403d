"""Weight averaging, the host side (no GPU; the library itself must load): the argument checks of vbg_lerp / vbg_swap, the numpy
restatement of the lerp against fp64 within the derived bound, and the schedule logic of vbg.optim.WeightAverage over a FlatGroup
in host memory with ops.lerp_ / ops.swap_ replaced by recording stand-ins (torch.lerp / an exchange on the CPU)."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_optim_groups_host import LAYOUT, OFFSETS, TOTAL
from weight_average_restate import OVERFLOWING, PLANTED, homed_six, lerp_bound, lerp_f64, lerp_restate, operands

WEIGHTS = [1 - 0.999, 1 - 0.9999, 1 / 3, 0.5, 0.75, 1.0, 0.0]


def test_argument_errors_do_not_need_a_gpu():
    from vbg import lib as L
    lerp, swap = L.lib.vbg_lerp, L.lib.vbg_swap
    assert lerp(None, None, 0, 0.5, None) == 0 and swap(None, None, 0, None) == 0               # n == 0 looks at no pointer
    buf = (C.c_float * 16)()
    a, b = C.addressof(buf), C.addressof(buf) + 32
    assert lerp(None, a, 4, 0.5, None) == -1 and lerp(a, None, 4, 0.5, None) == -1 and lerp(None, None, 4, 0.5, None) == -1
    assert swap(None, a, 4, None) == -1 and swap(a, None, 4, None) == -1
    assert lerp(a, b, -1, 0.5, None) == -1 and swap(a, b, -1, None) == -1
    assert swap(a, a, 4, None) == -1                                                              # the same range
    assert swap(a, b, 9, None) == -1 and swap(b, a, 9, None) == -1                                # 8 elements apart, 9 long: overlap
    assert swap(a, a, 0, None) == 0


def test_restatement_against_fp64_within_the_derived_bound():
    """both branches and their boundary, on the operands the device tests use; pairs whose difference overflows fp32 are left out
    (the statement forms p - a first: +-inf there, by torch's definition too) and exactly the planted ones are"""
    for n in (7, 1023, 5000):
        a, p, pos = operands(n, seed=n)
        a, p = a.numpy(), p.numpy()
        finite = np.isfinite(a) & np.isfinite(p)
        with np.errstate(all="ignore"):
            overflow = finite & ~np.isfinite((p - a).astype(np.float32))
        assert set(np.flatnonzero(overflow)) == {i for i, k in pos.items() if k in OVERFLOWING}
        keep = finite & ~overflow
        assert keep.sum() >= n - len(PLANTED)
        for w in WEIGHTS:
            out = lerp_restate(a, p, w).astype(np.float64)
            err = np.abs(out - lerp_f64(a, p, w))[keep]
            assert (err <= lerp_bound(a, p)[keep]).all(), (n, w, float(err.max()))
    # the branch really changes at |w| = 0.5, and the two statements differ in their bits somewhere (so the boundary is worth a test)
    a, p, _ = operands(5000, seed=1)
    a, p = a.numpy()[1000:], p.numpy()[1000:]                        # (behind the planted pairs)
    lo, hi = lerp_restate(a, p, np.nextafter(np.float32(0.5), np.float32(0))), lerp_restate(a, p, 0.5)
    assert np.array_equal(hi, p - (p - a) * np.float32(0.5)) and np.array_equal(lo, a + np.nextafter(np.float32(0.5), np.float32(0)) * (p - a))
    assert (a + np.float32(0.5) * (p - a) != hi).any()


# ---- schedule logic ------------------------------------------------------------------------------------------------------------
@pytest.fixture
def recorded(monkeypatch):
    """ops.lerp_ / ops.swap_ replaced: every call is noted as (name, tensor identity, weight) and carried out by torch on the CPU"""
    from vbg import ops
    calls = []

    def lerp_(avg, p, w):
        calls.append(("lerp", avg.data_ptr(), p.data_ptr(), w))
        avg.copy_(torch.lerp(avg, p, w))
        return avg

    def swap_(a, b):
        calls.append(("swap", a.data_ptr(), b.data_ptr(), ops._W_EPOCH[0]))
        t = a.clone()
        a.copy_(b)
        b.copy_(t)

    monkeypatch.setattr(ops, "lerp_", lerp_)
    monkeypatch.setattr(ops, "swap_", swap_)
    return calls


def _step(model, k):
    with torch.no_grad():
        for i, p in enumerate(model.parameters()):
            p.add_(0.01 * (k + 1) * torch.cos(torch.arange(p.numel(), dtype=torch.float32).reshape(p.shape) + i))


def test_first_update_copies_then_one_lerp_per_group(recorded):
    from vbg.optim import WeightAverage
    model, g = homed_six(LAYOUT, "cpu")
    assert g.offsets == OFFSETS and g.total == TOTAL
    avg = WeightAverage(model, kind="ema", decay=0.9)
    assert avg.groups is None                                         # binding waits for the first update
    avg.update()
    assert recorded == [] and avg.n_averaged == 1 and avg.groups == [g]
    assert torch.equal(avg.shadows[0], g.pflat) and avg.shadows[0].data_ptr() != g.pflat.data_ptr()
    _step(model, 0)
    avg.update()
    assert len(recorded) == 1 and recorded[0][:3] == ("lerp", avg.shadows[0].data_ptr(), g.pflat.data_ptr())
    assert recorded[0][3] == 1.0 - 0.9 and avg.n_averaged == 2 and avg.calls == 2


def test_swa_weights_every_start_and_callable_decay(recorded):
    from vbg.optim import WeightAverage
    model, g = homed_six(LAYOUT, "cpu")
    swa = WeightAverage(model, kind="swa")
    for k in range(5):
        swa.update()
        _step(model, k)
    assert [c[3] for c in recorded] == [1 / 2, 1 / 3, 1 / 4, 1 / 5] and swa.n_averaged == 5
    del recorded[:]
    # every=3, start=2: of the calls 1, 2, ... the 5th, 8th and 11th average; the 5th copies
    model, g = homed_six(LAYOUT, "cpu")
    avg = WeightAverage(model, kind="swa", every=3, start=2)
    seen = []
    for k in range(11):
        avg.update()
        seen.append(avg.n_averaged)
        if k == 3:
            assert avg.groups is None                                 # nothing bound, nothing allocated before the first averaging call
    assert seen == [0, 0, 0, 0, 1, 1, 1, 2, 2, 2, 3] and [c[3] for c in recorded] == [1 / 2, 1 / 3] and avg.calls == 11
    del recorded[:]
    # a warm-up schedule: decay as a function of n_averaged, asked once per lerp with the count before it
    model, g = homed_six(LAYOUT, "cpu")
    asked = []

    def decay(n):
        asked.append(n)
        return min(0.999, (1 + n) / (10 + n))

    ema = WeightAverage(model, kind="ema", decay=decay)
    for k in range(4):
        ema.update()
    assert asked == [1, 2, 3] and [c[3] for c in recorded] == [1.0 - min(0.999, (1 + n) / (10 + n)) for n in (1, 2, 3)]
    assert "decay" not in ema.state_dict()
    for bad in (dict(kind="mean"), dict(decay=1.5), dict(every=0), dict(start=-1), dict(buffers="all")):
        with pytest.raises(ValueError):
            WeightAverage(model, **bad)


@pytest.mark.parametrize("kind", ["ema", "swa"])
def test_counting_is_averaged_models(recorded, kind):
    """with torch.lerp standing in for the kernel, five updates follow torch.optim.swa_utils.AveragedModel's on the CPU.  Not bit for
    bit here: torch's CPU lerp rounds its vector lanes and its scalar tail differently, and a parameter falls into other lanes of the
    flat buffer than of its own tensor (the device test compares bits).  The bound is twice lerp_bound's 4 * 2^-24 * (|a| + |p|) with
    |a|, |p| < 8 for these values -- two results, each within the bound of the exact one; the parameters move by 1e-2 per step, so a
    wrong weight or a missed copy is off by 1e-3 and more."""
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    from vbg.optim import WeightAverage
    from weight_average_restate import SixModel
    model, g = homed_six(LAYOUT, "cpu")
    twin = SixModel(LAYOUT)
    ref = AveragedModel(twin, multi_avg_fn=get_ema_multi_avg_fn(0.99)) if kind == "ema" else AveragedModel(twin)
    avg = WeightAverage(model, kind=kind, decay=0.99)
    for k in range(5):
        _step(model, k)
        _step(twin, k)
        avg.update()
        ref.update_parameters(twin)
        want = dict(ref.module.named_parameters())
        for i, n in enumerate(g.names):
            got = g.view(avg.shadows[0], i)
            assert float(want[n].detach().abs().max()) < 8.0
            assert float((got - want[n].detach()).abs().max()) <= 2 * 4 * 2.0 ** -24 * 16.0, (k, n)
    assert avg.n_averaged == int(ref.n_averaged) == 5


def test_applied_swaps_back_and_invalidates(recorded):
    from vbg import ops
    from vbg.optim import WeightAverage
    model, g = homed_six(LAYOUT, "cpu")
    avg = WeightAverage(model, kind="ema", decay=0.5)
    with pytest.raises(RuntimeError):
        avg.swap()                                                    # nothing averaged yet
    avg.update()
    _step(model, 0)
    avg.update()
    live, mean = g.pflat.clone(), avg.shadows[0].clone()
    assert not torch.equal(live, mean)
    del recorded[:]

    def dirty():
        g._planes_tag = g._pair_tag = g._tp["tag"] = g._tq["tag"] = ("stale",)
        g._plain_tags[(0, 1, 32)] = ("stale",)
        g._ver["p"] = {0: (1,)}

    def clean():
        return (g._planes_tag, g._pair_tag, g._tp["tag"], g._tq["tag"]) == (None,) * 4 and not g._plain_tags and not g._ver

    dirty()
    e0 = ops._W_EPOCH[0]
    with avg.applied() as inside:
        assert inside is avg and avg.is_applied and clean() and ops._W_EPOCH[0] == e0 + 1          # invalidated AFTER the exchange ...
        assert recorded[-1][3] == e0                                                               # (... which ran at the old epoch)
        assert torch.equal(g.pflat, mean) and torch.equal(avg.shadows[0], live)
        assert torch.equal(model.stem_weight.detach(), g.view(mean, g.names.index("stem_weight")))
        with pytest.raises(RuntimeError):
            avg.update()
        with pytest.raises(RuntimeError):
            with avg.applied():
                pass
        with pytest.raises(RuntimeError):
            avg.copy_to()
        dirty()
    assert not avg.is_applied and clean() and ops._W_EPOCH[0] == e0 + 2 and len(recorded) == 2
    assert torch.equal(g.pflat, live) and torch.equal(avg.shadows[0], mean)
    # an exception inside the block: the live weights are back, the caches told again
    dirty()
    with pytest.raises(KeyError):
        with avg.applied():
            raise KeyError("validation failed")
    assert not avg.is_applied and clean() and ops._W_EPOCH[0] == e0 + 4
    assert torch.equal(g.pflat, live) and torch.equal(avg.shadows[0], mean)
    # copy_to: the average becomes the live weights; the same invalidation
    dirty()
    avg.copy_to()
    assert torch.equal(g.pflat, mean) and torch.equal(avg.shadows[0], mean) and clean() and ops._W_EPOCH[0] == e0 + 5


def test_binding_errors_and_unhomed_parameters(recorded):
    from vbg.optim import FlatGroup, WeightAverage
    from weight_average_restate import SixModel
    # no flat home at all
    plain = SixModel(LAYOUT)
    with pytest.raises(ValueError, match="AveragedModel"):
        WeightAverage(plain).update()
    # a trained parameter outside the buffers is named; one that never gets a gradient, and a frozen one, are left alone
    model = SixModel(LAYOUT)
    named = list(model.named_parameters())
    g = FlatGroup([np_ for np_ in named if np_[0] not in ("head_bias", "mid_weight")], "cpu")
    model.mid_weight.requires_grad_(False)
    avg = WeightAverage(model)
    model.head_bias.grad = torch.zeros_like(model.head_bias)
    with pytest.raises(ValueError, match="head_bias"):
        avg.update()
    model.head_bias.grad = None
    avg.update()
    assert avg.groups == [g] and avg.n_averaged == 1
    assert set(avg.state_dict()["shadow"]) == set(g.names)
    # the parameters moved away from the buffer the average is bound to
    model.stem_weight.data = model.stem_weight.data.clone()
    with pytest.raises(RuntimeError, match="moved"):
        avg.update()
    with pytest.raises(RuntimeError, match="moved"):
        avg.swap()


def test_state_dict_round_trip_and_averaged_state_dict(recorded):
    from vbg.optim import WeightAverage
    model, g = homed_six(LAYOUT, "cpu")
    model.register_buffer("running", torch.arange(4, dtype=torch.float32))
    model.register_buffer("ticks", torch.tensor(3))
    avg = WeightAverage(model, kind="ema", decay=0.75, every=2, buffers="average")
    for k in range(4):
        _step(model, k)
        model.running += 1.0
        avg.update()
    assert avg.n_averaged == 2 and torch.equal(avg._buf_avg[0], torch.lerp(torch.arange(4.) + 2, torch.arange(4.) + 4, 0.25))
    sd = avg.state_dict()
    assert {k: sd[k] for k in ("n_averaged", "calls", "kind", "decay", "every", "start", "buffers")} == \
        {"n_averaged": 2, "calls": 4, "kind": "ema", "decay": 0.75, "every": 2, "start": 0, "buffers": "average"}
    assert set(sd["shadow"]) == set(g.names) and set(sd["shadow_buffers"]) == {"running"}
    for i, n in enumerate(g.names):
        assert sd["shadow"][n].shape == g.params[i].shape and sd["shadow"][n].data_ptr() != g.view(avg.shadows[0], i).data_ptr()
    # the averaged checkpoint: the model's keys, averaged parameters and float buffers, live integer buffer; the model undisturbed
    live = {k: v.clone() for k, v in model.state_dict().items()}
    asd = avg.averaged_state_dict()
    assert list(asd) == list(model.state_dict())
    for i, n in enumerate(g.names):
        assert torch.equal(asd[n], g.view(avg.shadows[0], i)) and not torch.equal(asd[n], live[n])
    assert torch.equal(asd["running"], avg._buf_avg[0]) and torch.equal(asd["ticks"], live["ticks"])
    assert all(torch.equal(v, live[k]) for k, v in model.state_dict().items())
    with avg.applied():                                               # the same checkpoint from inside the block
        assert torch.equal(model.running, asd["running"]) and int(model.ticks) == 3
        inside = avg.averaged_state_dict()
        assert all(torch.equal(inside[k], asd[k]) for k in asd)
    assert torch.equal(model.running, live["running"])
    # a second model with another layout history: loading binds, copies per parameter, keeps the padding zero
    model2, g2 = homed_six(LAYOUT, "cpu", seed=5)
    model2.register_buffer("running", torch.zeros(4))
    model2.register_buffer("ticks", torch.tensor(0))
    avg2 = WeightAverage(model2, kind="ema", decay=0.5, buffers="average")
    avg2.load_state_dict(sd)
    assert (avg2.n_averaged, avg2.calls, avg2.every, avg2.decay) == (2, 4, 2, 0.75)
    assert torch.equal(avg2.shadows[0], avg.shadows[0]) and torch.equal(avg2._buf_avg[0], avg._buf_avg[0])
    with pytest.raises(ValueError):
        WeightAverage(model2, kind="swa", buffers="average").load_state_dict(sd)
    # the padding between the slots of the average stays zero through updates
    covered = torch.zeros(TOTAL, dtype=torch.bool)
    for off, p in zip(g.offsets, g.params):
        covered[off:off + p.numel()] = True
    assert not avg.shadows[0][~covered].any() and avg.shadows[0][covered].abs().min() > 0
