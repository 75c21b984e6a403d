"""Weight averaging on the device: vbg_lerp against torch's own lerp bit for bit and against fp64 within the derived bound, vbg_swap
as an exact exchange of bit patterns, vbg.optim.WeightAverage against torch.optim.swa_utils.AveragedModel on a small FlatGroup, no
host sync in update() / applied(), and the model: training with an average kept and applied in between equals training without one,
the eval forward inside applied() is the forward of a fresh net loaded with averaged_state_dict(), and a checkpoint of the average
resumes bit for bit.  Needs a real MI355X."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_model import build_product, to_dev
from test_gpu_small_kernels import bits
from test_gpu_train_loop import _net, _torch_opts
from test_optim_groups_host import LAYOUT, TOTAL
from test_oracle_golden import _e2e_inputs, e2e_cfg
from weight_average_restate import OVERFLOWING, homed_six, lerp_bound, lerp_f64, operands, SixModel

# one full sweep of the capped grid (2048 blocks x 256 threads x 4 elements), a second stride, a scalar tail: the smallest size that
# exercises the stride loop
SIZES = [1, 3, 4, 5, 7, 1023, 2_097_152 + 1024 + 3]
WEIGHTS = [1 - 0.999, 1 - 0.9999, 1 / 3, 0.5, 0.75, 1.0, 0.0]          # both branches of torch's statement and their boundary
CASES = [(n, 0) for n in SIZES] + [(1023, 1)]                           # (elements, offset): offset 1 = both pointers 4 bytes off 16
PAD = 8


def dev():
    return torch.device("cuda")


def framed(values, off):
    """`values` inside a device buffer with NaN / 1e30 canaries on both sides -> (buffer, the range as a view).  The range starts
    16-byte aligned for off == 0 and `off` elements behind that otherwise"""
    n = values.numel()
    buf = torch.empty(PAD + off + n + PAD)
    buf[0::2] = float("nan")
    buf[1::2] = 1e30
    buf[PAD + off:PAD + off + n] = values
    buf = buf.to(dev())
    view = buf[PAD + off:PAD + off + n]
    assert view.data_ptr() % 16 == 4 * off and view.is_contiguous()
    return buf, view


def canaries_intact(buf, off, n):
    want = torch.empty(buf.numel())
    want[0::2] = float("nan")
    want[1::2] = 1e30
    got = bits(buf)
    lo, hi = PAD + off, PAD + off + n
    return torch.equal(got[:lo], bits(want)[:lo]) and torch.equal(got[hi:], bits(want)[hi:])


def same_bits_or_class(out, ref):
    """finite results: the same bits; non-finite ones: the same class (NaN, +inf, -inf)"""
    fin = torch.isfinite(ref)
    return (torch.equal(torch.isnan(out), torch.isnan(ref)) and torch.equal(torch.isfinite(out), fin)
            and torch.equal(out[~fin & ~torch.isnan(ref)], ref[~fin & ~torch.isnan(ref)])
            and torch.equal(out[fin].view(torch.int32), ref[fin].view(torch.int32)))


@pytest.fixture(scope="module")
def lerp_runs():
    """every (size, offset, weight) once: (a, p, positions of the planted pairs, kernel result, torch's result, canaries intact),
    on the host; shared by the bit test and the fp64 test"""
    from vbg import ops
    runs = {}
    for n, off in CASES:
        a, p, pos = operands(n, seed=n + off)
        for w in WEIGHTS:
            abuf, av = framed(a, off)
            pbuf, pv = framed(p, off)
            ref = av.clone()
            torch._foreach_lerp_([ref], [pv.clone()], w)
            ops.lerp_(av, pv, w)
            torch.cuda.synchronize()
            ok = canaries_intact(abuf, off, n) and torch.equal(bits(pbuf), bits(framed(p, off)[0]))
            runs[(n, off, w)] = (a, p, pos, av.cpu(), ref.cpu(), ok)
    return runs


@pytest.mark.parametrize("n,off", CASES)
def test_lerp_is_torchs_lerp_bit_for_bit(lerp_runs, n, off):
    for w in WEIGHTS:
        a, p, pos, out, ref, ok = lerp_runs[(n, off, w)]
        assert ok, (n, off, w, "a canary or the second operand changed")
        assert same_bits_or_class(out, ref), (n, off, w, int((out.view(torch.int32) != ref.view(torch.int32)).sum()))
        # a == p exactly (not the pair of -0.0: +0.0 on the first branch, in torch too) stays exactly that under every weight
        for i, k in pos.items():
            if k in (3, 8):
                assert bits(out)[i] == bits(a)[i], (n, w, i)


@pytest.mark.parametrize("n,off", CASES)
def test_lerp_against_fp64_within_the_derived_bound(lerp_runs, n, off):
    """|out - (a + w (p - a))| <= 4 * 2^-24 * (|a| + |p|) + 2^-149 on every pair of finite operands -- except pairs whose difference
    p - a overflows fp32: torch's statement forms that difference first, so its result there is +-inf or NaN by definition.  Exactly
    the planted +-FLT_MAX pairs are excluded."""
    for w in WEIGHTS:
        a, p, pos, out, _, _ = lerp_runs[(n, off, w)]
        a, p, out = a.numpy(), p.numpy(), out.numpy().astype(np.float64)
        finite = np.isfinite(a) & np.isfinite(p)
        overflow = finite & (np.abs(p.astype(np.float64) - a.astype(np.float64)) > float(np.finfo(np.float32).max))
        assert set(np.flatnonzero(overflow)) == {i for i, k in pos.items() if k in OVERFLOWING}
        keep = finite & ~overflow
        assert np.isfinite(out[keep]).all()
        err, bound = np.abs(out - lerp_f64(a, p, w))[keep], lerp_bound(a, p)[keep]
        worst = int(np.argmax(err - bound))
        assert (err <= bound).all(), (n, off, w, float(err[worst]), float(bound[worst]))


def swap_values(n, seed):
    """int32 patterns read as fp32: normal deviates with quiet and signalling NaN payloads, -0.0, denormals and infinities planted"""
    a, p, _ = operands(n, seed=seed)
    special = [0x7FC12345, -0x005FFFFF, -0x80000000, 0x00000001, -0x7FFFFFFF, 0x7F800000, 0x7FA00001, 0x007FFFFF]
    for t, shift, order in ((a, 0, special), (p, 3, special[::-1])):
        ti = t.view(torch.int32)
        for k, s in enumerate(order):
            i = (11 * k + shift) % n if n < 1023 else (n - 1 - 13 * k - shift if k % 2 else 7 * k + shift)
            ti[i] = s
    return a, p


@pytest.mark.parametrize("n,off", CASES)
def test_swap_exchanges_bit_patterns_exactly(n, off):
    from vbg import ops
    from vbg.lib import VbgError
    a, b = swap_values(n, seed=50 + n)
    abuf, av = framed(a, off)
    bbuf, bv = framed(b, off)
    a, b = av.cpu(), bv.cpu()                                          # (what the device holds before the exchange)
    for pattern in (0x7FC12345, 0x7FA00001, -0x005FFFFF, -0x80000000, 0x00000001) if n >= 1023 else ():          # (they reached the device as planted)
        assert (bits(a) == pattern).any() and (bits(b) == pattern).any(), hex(pattern)
    ops.swap_(av, bv)
    torch.cuda.synchronize()
    assert torch.equal(bits(av), bits(b)) and torch.equal(bits(bv), bits(a)) and not torch.equal(bits(a), bits(b))
    assert canaries_intact(abuf, off, n) and canaries_intact(bbuf, off, n)
    ops.swap_(av, bv)                                                  # applied twice: the identity
    torch.cuda.synchronize()
    assert torch.equal(bits(av), bits(a)) and torch.equal(bits(bv), bits(b))
    assert canaries_intact(abuf, off, n) and canaries_intact(bbuf, off, n)
    if n >= 8:                                                         # the same or overlapping ranges are refused, nothing is written
        before = bits(abuf)
        for x, y in ((av, av), (av[:n - 1], av[1:]), (av[4:], av[:n - 4])):
            with pytest.raises(VbgError):
                ops.swap_(x, y)
        torch.cuda.synchronize()
        assert torch.equal(bits(abuf), before)


def _nudge(model, k):
    with torch.no_grad():
        for i, p in enumerate(model.parameters()):
            p.add_(0.01 * (k + 1) * torch.cos(torch.arange(p.numel(), dtype=torch.float32, device=p.device).reshape(p.shape) + i))


@pytest.mark.parametrize("kind", ["ema", "swa"])
def test_weight_average_is_averaged_model_bit_for_bit(kind):
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    from vbg.optim import WeightAverage
    model, g = homed_six(LAYOUT, dev())
    twin = SixModel(LAYOUT).to(dev())
    assert g.total == TOTAL and all(torch.equal(a, b) for a, b in zip(model.parameters(), twin.parameters()))
    ref = AveragedModel(twin, multi_avg_fn=get_ema_multi_avg_fn(0.99)) if kind == "ema" else AveragedModel(twin)
    avg = WeightAverage(model, kind=kind, decay=0.99)
    covered = torch.zeros(TOTAL, dtype=torch.bool)
    for off, p in zip(g.offsets, g.params):
        covered[off:off + p.numel()] = True
    for k in range(5):
        _nudge(model, k)
        _nudge(twin, k)
        avg.update()
        ref.update_parameters(twin)
        want = dict(ref.module.named_parameters())
        for i, n in enumerate(g.names):
            assert torch.equal(bits(g.view(avg.shadows[0], i)), bits(want[n])), (kind, k, n)
            assert not torch.equal(bits(g.view(avg.shadows[0], i)), bits(g.params[i])) or k == 0
        assert not bits(avg.shadows[0])[~covered].any() and not bits(g.pflat)[~covered].any()          # padding still zero (+0.0)
    assert avg.n_averaged == int(ref.n_averaged) == 5


def test_no_host_sync_in_update_and_applied():
    from vbg.optim import WeightAverage
    model, g = homed_six(LAYOUT, dev())
    avg = WeightAverage(model, kind="ema", decay=0.9)
    avg.update()                                                       # (binds, allocates, copies)
    _nudge(model, 0)
    live = g.pflat.clone()
    torch.cuda.synchronize()
    raised = None
    torch.cuda.set_sync_debug_mode("error")
    try:
        avg.update()
        with avg.applied():
            pass
    except RuntimeError as e:
        raised = str(e)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert raised is None, raised
    assert avg.n_averaged == 2 and torch.equal(bits(g.pflat), bits(live)) and not torch.equal(bits(avg.shadows[0]), bits(live))


# ---- the model -----------------------------------------------------------------------------------------------------------------
DECAY = 0.5          # (a short memory: after two steps the average sits half a step behind the live weights)


def _train(net, dbatch, opts, steps, after=None):
    for s in steps:
        random.seed(100 + s)
        loss = net(*dbatch)
        for o in opts:
            o.zero_grad()
        loss.backward()
        for o in opts:
            o.step()
        if after is not None:
            after(s)


def _eval(net, dbatch):
    net.eval()
    random.seed(9)
    with torch.no_grad():
        out = net(*dbatch)
    net.train()
    return [t.detach().clone() for t in out]


def test_model_trains_the_same_and_validates_on_the_average(golden, tmp_path):
    from vbg import ops
    from vbg.optim import WeightAverage
    dbatch = to_dev(_e2e_inputs(golden("e2e.npz")), dev())
    with ops.deterministic_scope(True):
        # run A: an average kept after every step, applied for a validation pass after the second
        na = _net(tmp_path, "a", dev())
        avg = WeightAverage(na, kind="ema", decay=DECAY)
        snaps = []

        def after(s):
            avg.update()
            snaps.append([g.pflat.clone() for g in avg.groups])

        oa = _torch_opts(na)
        _train(na, dbatch, oa, (0, 1), after)
        with avg.applied():
            out_avg = _eval(na, dbatch)
        asd = avg.averaged_state_dict()
        ckpt = {"module." + k: v.cpu() for k, v in asd.items()}          # (train_SROIE.py saves the DDP wrapper's keys)
        _train(na, dbatch, oa, (2, 3), after)
        # run B: the same four steps and a validation pass on the live weights, no WeightAverage at all
        nb = _net(tmp_path, "b", dev())
        ob = _torch_opts(nb)
        _train(nb, dbatch, ob, (0, 1))
        out_live = _eval(nb, dbatch)
        _train(nb, dbatch, ob, (2, 3))
        # a fresh net loaded with the averaged checkpoint the way eval_SROIE.py:335-337 does
        fresh = build_product(tmp_path / "c", "resnet_18_fpn", e2e_cfg("resnet_18_fpn")).to(dev())
        res = fresh.load_state_dict({k.replace("module.", ""): v for k, v in ckpt.items()}, strict=False)
        assert not res.unexpected_keys and all(k.endswith(("position_ids", "token_type_ids")) for k in res.missing_keys), res
        out_fresh = _eval(fresh, dbatch)
    torch.cuda.synchronize()
    # 1. the exchange gave the live weights back exactly, and steps 3-4 saw no stale plane, transposed-plane or filter image
    pa, pb = dict(na.named_parameters()), dict(nb.named_parameters())
    assert len(avg.groups) == 2 and set(pa) == set(pb)
    for k in pa:
        assert torch.equal(bits(pa[k]), bits(pb[k])), k
    # 2. the forward inside applied() used the averaged weights, and the checkpoint is the model's format
    live_sd = na.state_dict()
    assert list(asd) == list(live_sd)
    for k, v in live_sd.items():                                       # the model's shapes and layouts (channels_last filters kept)
        assert asd[k].shape == v.shape and asd[k].stride() == v.stride() and asd[k].dtype == v.dtype, k
    assert asd["bert_model.embeddings.word_embeddings.weight"].data_ptr() == \
        asd["BERTgrid_generator.model.embeddings.word_embeddings.weight"].data_ptr()
    assert len(out_avg) == len(out_fresh) == 5
    for a, b in zip(out_avg, out_fresh):
        assert torch.equal(a, b)
    # 3. (a condition, not a measurement) ... which are not the live weights: the loss and the logits of the two passes differ
    assert not torch.equal(out_avg[0], out_live[0]) and not torch.equal(out_avg[4], out_live[4])
    assert abs(float(out_avg[0]) - float(out_live[0])) > 1e-6 * abs(float(out_live[0])), (float(out_avg[0]), float(out_live[0]))
    # 4. the average is torch.lerp replayed over the per-step parameters
    assert len(snaps) == 4
    for gi, (g, s) in enumerate(zip(avg.groups, avg.shadows)):
        want = snaps[0][gi].clone()
        for step in snaps[1:]:
            want = torch.lerp(want, step[gi], 1.0 - DECAY)
        assert torch.equal(bits(s), bits(want)), gi
        assert not torch.equal(bits(s), bits(g.pflat))
    # 5.
    assert avg.n_averaged == 4 and avg.calls == 4 and not avg.is_applied


def test_checkpoint_of_the_average_resumes_bit_for_bit(golden, tmp_path):
    from vbg.optim import WeightAverage
    dbatch = to_dev(_e2e_inputs(golden("e2e.npz")), dev())
    na = _net(tmp_path, "a", dev())
    avg = WeightAverage(na, kind="ema", decay=0.9, buffers="average")
    _train(na, dbatch, _torch_opts(na), (0, 1), lambda s: avg.update())
    sd = avg.state_dict()
    assert sd["n_averaged"] == 2 and set(sd["shadow"]) == {n for g in avg.groups for n in g.names}
    assert any(k.endswith("running_mean") for k in sd["shadow_buffers"]) and not any("num_batches" in k for k in sd["shadow_buffers"])
    # resume: a fresh net, one training forward so that it is homed, the model weights, a new WeightAverage
    nb = _net(tmp_path, "b", dev())
    random.seed(100)
    nb(*dbatch)
    nb.load_state_dict(na.state_dict())
    avg2 = WeightAverage(nb, kind="ema", decay=0.5, buffers="average")
    avg2.load_state_dict(sd)
    assert (avg2.n_averaged, avg2.calls, avg2.decay, avg2.every, avg2.start) == (2, 2, 0.9, 1, 0)

    def same():
        torch.cuda.synchronize()
        assert len(avg.groups) == len(avg2.groups) == 2
        for g, s, g2, s2 in zip(avg.groups, avg.shadows, avg2.groups, avg2.shadows):
            assert g is not g2 and g.names == g2.names and torch.equal(bits(s), bits(s2)) and torch.equal(bits(g.pflat), bits(g2.pflat))
        assert avg._buf_names == avg2._buf_names and all(torch.equal(bits(x), bits(y)) for x, y in zip(avg._buf_avg, avg2._buf_avg))

    same()
    for net, w in ((na, avg), (nb, avg2)):                             # one more identical synthetic parameter change on both
        _nudge_model(net)
        w.update()
    same()
    assert avg.n_averaged == avg2.n_averaged == 3
    assert not torch.equal(bits(avg.shadows[0]), bits(avg.groups[0].pflat))


def _nudge_model(net):
    with torch.no_grad():
        for i, p in enumerate(q for q in net.parameters() if hasattr(q, "_vbg_flat")):
            p.mul_(1.0 + 1e-3 * ((i % 7) - 3))
        for b in net.buffers():
            if b.is_floating_point():
                b.mul_(1.01)
