"""The frozen-BatchNorm epilogue at model level (vbg.ops.set_bn_epilogue): inference() and the eval forward take ONE launch per
conv + BatchNorm node, every call in which a backward can come keeps the two launches, the results stay inside the fixtures' existing
tolerances, deterministic mode holds, and the amax word of a fused layer is published and consumed."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vbg_oracle as O
from test_gpu_model import build_product, build_product_mode, load_synth, to_dev
from test_oracle_golden import _e2e_inputs, e2e_cfg

T = torch.from_numpy


class _switch:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from vbg import ops
        self.prev = ops.bn_epilogue_enabled()
        ops.set_bn_epilogue(self.on)
        self.log = ops.dispatch_log(True)
        return self.log

    def __exit__(self, *exc):
        from vbg import ops
        ops.dispatch_log(False)
        ops.set_bn_epilogue(self.prev)


def _net(tmp_path, backbone, dev):
    cfg = e2e_cfg(backbone)
    net = build_product(tmp_path, backbone, cfg)
    sd = load_synth(net, cfg, 1200)
    return net.to(dev), cfg, sd


@pytest.mark.parametrize("backbone", ["resnet_18_fpn", "resnet_18_D_fpn"])
def test_inference_switch_on_vs_golden(golden, tmp_path, backbone):
    """inference() with the switch on: the existing test's tolerance against the reference's class probabilities (e2e.npz holds them for
    resnet_18_fpn; for the D trunk, which the fixture does not carry, the CPU oracle on the same weights stands in, as in the other D tests),
    rows sum to 1, and the dispatch log shows every eval-mode BatchNorm apply replaced by an epilogue -- the same count"""
    g = golden("e2e.npz")
    dev = torch.device("cuda")
    net, cfg, sd = _net(tmp_path, backbone, dev)
    net.eval()
    batch = _e2e_inputs(g)
    imgs, segs, classes, coors, corpus, mask = to_dev(batch, dev)
    if backbone == "resnet_18_fpn":
        ref = T(g["r18_pred"])
    else:
        random.seed(7)
        with torch.no_grad():
            ref = O.forward({k: v.clone() for k, v in sd.items()}, cfg, *batch, training=False)[4]
    with _switch(False) as off, torch.no_grad():
        p_off = net.inference(imgs, segs, coors, corpus, mask)
        off = dict(off)
    with _switch(True) as on, torch.no_grad():
        p_on = net.inference(imgs, segs, coors, corpus, mask)
        on = dict(on)
    n = off.get("bn:apply", 0)
    assert n > 0 and "bn:epilogue" not in off, off
    assert on.get("bn:epilogue", 0) == n and "bn:apply" not in on, on
    assert on.get("bn:epilogue_gemm", 0) + on.get("bn:epilogue_conv3", 0) == n, on
    print(f"{backbone}: {n} BatchNorm applies fused; on torch.equal off: {torch.equal(p_on, p_off)}; "
          f"max |on - off| = {float((p_on - p_off).abs().max()):.3e}")
    for p in (p_on, p_off):
        assert torch.allclose(p.cpu(), ref, rtol=1e-4, atol=1e-5), float((p.cpu() - ref).abs().max())
        assert torch.allclose(p.sum(1).cpu(), torch.ones(p.shape[0]), atol=1e-5)


@pytest.mark.parametrize("mode", ["simp", "full"])
def test_eval_forward_on_vs_off(golden, tmp_path, mode):
    """net.eval() under no_grad (the validation loop's forward, 5-tuple): loss and predictions with the switch on against off, inside the
    fixtures' own tolerances (2e-4 of the loss; rtol 1e-4 / atol 1e-5 on the predictions; 1e-3 / 2e-4 on the segmentation maps)"""
    dev = torch.device("cuda")
    batch = _e2e_inputs(golden("e2e.npz"))
    if mode == "simp":
        net, cfg, sd = _net(tmp_path, "resnet_18_fpn", dev)
    else:
        from test_oracle_golden import modes_state
        cfg, sd = modes_state(golden("e2e_modes.npz"), mode)
        net = build_product_mode(tmp_path, mode, cfg)
        assert not net.load_state_dict(sd, strict=False).unexpected_keys
        net = net.to(dev)
    dbatch = to_dev(batch, dev)
    net.eval()
    outs = {}
    for on in (False, True):
        with _switch(on) as log, torch.no_grad():
            random.seed(7)
            outs[on] = net(*dbatch)
            assert ("bn:epilogue" in log) == on and ("bn:apply" in log) == (not on), dict(log)
    (l0, pm0, ps0, gt0, pr0), (l1, pm1, ps1, gt1, pr1) = outs[False], outs[True]
    print(f"{mode}: loss off {float(l0):.8f} on {float(l1):.8f}; pred equal: {torch.equal(pr0, pr1)}")
    assert torch.equal(gt0, gt1)
    assert abs(float(l1) - float(l0)) <= 2e-4 * abs(float(l0))
    assert torch.allclose(pr1, pr0, rtol=1e-4, atol=1e-5)
    assert torch.allclose(ps1, ps0, rtol=1e-3, atol=2e-4) and torch.allclose(pm1, pm0, rtol=1e-3, atol=2e-4)


def test_calls_that_can_have_a_backward_keep_two_launches(golden, tmp_path):
    """switch on, BatchNorm modules frozen (eval()) inside a training step, and an eval-mode call made with grad enabled: no epilogue
    launch, and every gradient arrives finite"""
    dev = torch.device("cuda")
    net, cfg, _ = _net(tmp_path, "resnet_18_fpn", dev)
    dbatch = to_dev(_e2e_inputs(golden("e2e.npz")), dev)

    def finite_grads():
        seen = 0
        for name, p in net.named_parameters():
            if p.grad is not None:
                assert torch.isfinite(p.grad).all(), name
                seen += 1
        assert seen > 100

    net.train()
    for m in net.modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            m.eval()
    with _switch(True) as log:
        random.seed(7)
        loss = net(*dbatch)
        loss.backward()
        assert "bn:epilogue" not in log and log.get("bn:apply", 0) > 0, dict(log)
    assert torch.isfinite(loss).all()
    finite_grads()
    net.eval()
    with _switch(True) as log:
        random.seed(7)
        loss = net(*dbatch)[0]
        assert "bn:epilogue" not in log and log.get("bn:apply", 0) > 0, dict(log)
        assert loss.requires_grad
        loss.backward()
    assert torch.isfinite(loss).all()
    finite_grads()


def test_deterministic_mode_with_the_switch_on(golden, tmp_path):
    """the epilogues add no float atomics: inference() twice is bit-identical in deterministic mode, with no fatomic:* key in the log"""
    from vbg import ops
    dev = torch.device("cuda")
    net, cfg, _ = _net(tmp_path, "resnet_18_fpn", dev)
    net.eval()
    imgs, segs, classes, coors, corpus, mask = to_dev(_e2e_inputs(golden("e2e.npz")), dev)
    with ops.deterministic_scope(True), _switch(True) as log, torch.no_grad():
        a = net.inference(imgs, segs, coors, corpus, mask)
        b = net.inference(imgs, segs, coors, corpus, mask)
        assert log.get("bn:epilogue", 0) > 0 and not [k for k in log if k.startswith("fatomic:")], sorted(log)
    assert torch.equal(a, b)


def test_amax_word_of_a_fused_layer_is_published_and_consumed():
    """one channel of a fused layer's output far outside fp16's range (max |y| > 65520): the next 3 x 3 convolution -- the fp16-pair form,
    which scales its activation operand by the producer's amax word -- must stay finite and agree with the two-launch route.

    Bound on |out_on - out_off|, derived: the two routes' y differ by d = |y_on - y_off| (each within the kernel gate of the same fp64
    value), which the convolution carries to at most conv(d, |w|); each route's own convolution error is at most (2^-21 + K 2^-24) of
    conv(|y|, |w|) -- two operands split to 2^-23 each and the dropped lo x lo products (< 2^-21 of a product in all), and K = 576 fp32
    accumulation steps of 2^-24 in the worst case."""
    from vbg import functions as Fn
    from vbg import ops
    import torch.nn.functional as F
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(3)
    x = torch.randn((1, 16, 32, 64), generator=g).to(dev)
    w1 = (torch.randn((64, 64, 1, 1), generator=g) / 8).to(dev)
    w2 = (torch.randn((128, 64, 3, 3), generator=g) / 24).to(dev).contiguous(memory_format=torch.channels_last)
    gamma = (0.5 + torch.rand(64, generator=g)).to(dev)
    gamma[3] *= 1e6                                                   # one channel of y far above 65520
    beta, rm = torch.randn(64, generator=g).to(dev), (0.1 * torch.randn(64, generator=g)).to(dev)
    rv = (0.5 + torch.rand(64, generator=g)).to(dev)
    assert ops.conv3_f16_enabled() and ops.conv3_ok(1, 16, 32, 64, 128, 3, 3, 1, 1, fwd=True)
    res = {}
    for on in (False, True):
        with _switch(on) as log, torch.no_grad():
            y = Fn.ConvBnFn.apply(x, w1, gamma, beta, rm, rv, None, 1, 0, True, False, 0.1, 1e-5, False)
            slot = Fn._amax_tag(y)
            assert slot is not None, "the fused layer must tag its output with the amax slot"
            out = Fn.ConvFn.apply(y, w2, None, 1, 1)
            assert ("bn:epilogue" in log) == on and log.get("conv3:f16x2", 0) == 1, dict(log)
            ymax = y.abs().max()
            assert float(ymax) > 65520.0
            assert int(slot.view(ops.AMAX_WORDS, ops.AMAX_STRIDE)[:, 0].max()) == int(ymax.view(torch.int32))
            assert torch.isfinite(out).all()
            res[on] = (y.double().cpu(), out.double().cpu())
    (y0, o0), (y1, o1) = res[False], res[True]
    w64 = w2.double().cpu().abs()
    conv = lambda t: F.conv2d(t.permute(0, 3, 1, 2), w64, padding=1).permute(0, 2, 3, 1)
    bound = conv((y1 - y0).abs()) + 2 * (2.0 ** -21 + 576 * 2.0 ** -24) * conv(y0.abs())
    ratio = float(((o1 - o0).abs() / bound.clamp(min=1e-300)).max())
    print(f"y on == off: {torch.equal(y0, y1)}; max |out_on - out_off| / bound = {ratio:.3e}")
    assert ratio <= 1.0
