"""The crf mode's training step through the length-stable loss (ops.set_crf_stable), end to end on the tiny net of
tests/test_gpu_crf_posterior_model.py in train mode: ViBERTgridNet.forward -> CRFFieldTypeClassification.forward -> CRF.nll ->
Fn.CrfNllStableFn.  Needs a real MI355X."""
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_crf_posterior_model import FIELDS, build_crf_net
from test_gpu_model import to_dev
from test_oracle_golden import _e2e_inputs, modes_state

KEY = "crf:nll_stable"


@pytest.fixture(scope="module")
def crf_train_net(golden, tmp_path_factory):
    g = golden("e2e_modes.npz")
    cfg, sd = modes_state(g, "crf")
    tags = {"O": 0}
    for k, f in enumerate(FIELDS[1:], start=1):
        tags["B-" + f] = k
    net = build_crf_net(tmp_path_factory.mktemp("crf_train_net"), cfg, tags)
    assert not net.load_state_dict(sd, strict=False).unexpected_keys
    dev = torch.device("cuda")
    return net.to(dev).train(), to_dev(_e2e_inputs(golden("e2e.npz")), dev)


def step(net, batch, stable):
    """one forward + backward -> (loss, dispatch log, emissions seen by the crf layer, gout handed to the stable backward or None)"""
    from vbg import ops
    head = net.field_type_classification_head
    seen, gouts = [], []
    hook = head.category_classification_net.register_forward_hook(lambda m, a, out: seen.append(out.detach().clone()))
    real_bwd = ops.crf_nll_stable_bwd

    def spy(dem_unit, dtrans_unit, doc_off, gout, dtrans):
        gouts.append(gout.detach().clone())
        return real_bwd(dem_unit, dtrans_unit, doc_off, gout, dtrans)

    before = ops.crf_stable_enabled()
    net.zero_grad(set_to_none=True)
    ops.set_crf_stable(stable)
    ops.crf_nll_stable_bwd = spy
    log = ops.dispatch_log(True)
    try:
        random.seed(7)
        loss = net(*batch)
        loss.backward()
        torch.cuda.synchronize()
    finally:
        ops.dispatch_log(False)
        ops.crf_nll_stable_bwd = real_bwd
        ops.set_crf_stable(before)
        hook.remove()
    assert len(seen) == 1
    return loss, dict(log), seen[0], (gouts[0] if gouts else None)


def test_switch_on_takes_the_stable_route(crf_train_net):
    from vbg import ops
    net, batch = crf_train_net
    loss, log, em, gout = step(net, batch, True)
    assert log.get(KEY) == 1
    assert "fatomic:crf_nll_bwd" not in log and "det:crf_nll_bwd" not in log
    assert bool(torch.isfinite(loss).all())
    head = net.field_type_classification_head
    crf = head.crf_layer
    got = crf.transitions.grad
    assert got is not None and bool(torch.isfinite(got).all()) and bool(got.any())
    # the same two launches by hand, on the emissions the layer was given
    classes = batch[2]
    lens = [int(c.shape[0]) for c in classes]
    tags = torch.cat([c.reshape(-1) for c in classes]).to(em.device).int()
    doc_off = head._doc_off(lens, em.device)
    s, e = crf._ends()
    assert gout is not None and tuple(gout.shape) == (len(lens),)
    _, _, du, tu = ops.crf_nll_stable(em.float().contiguous(), tags, doc_off, crf.transitions.detach().contiguous(), s, e, True)
    want = torch.zeros_like(got)
    ops.crf_nll_stable_bwd(du, tu, doc_off, gout, want)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_switch_off_takes_todays_route(crf_train_net):
    net, batch = crf_train_net
    loss, log, _, gout = step(net, batch, False)
    assert KEY not in log and log.get("fatomic:crf_nll_bwd") == 1 and gout is None
    assert bool(torch.isfinite(loss).all())
