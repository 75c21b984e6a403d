"""Rectangular RoIAlign bins (roi_shape=(h, w)) on the GPU: the kernels against the restatement of the published algorithm
(tests/roi_align_restate.py), and ViBERTgridNet built with a rectangular roi_shape against fp64 restatements of its RoI chain."""
import os
import pathlib
import random
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import roi_align_restate as R
import vbg_oracle as O
from test_gpu_model import load_synth, make_bert_dir, to_dev
from test_oracle_golden import _e2e_inputs, e2e_cfg
from vbg import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda")
SHAPES = [(7, 7), (3, 21), (4, 16), (2, 5), (1, 1), (8, 32), (14, 14)]


def _case(C, seed=3):
    rng = np.random.default_rng(seed)
    B, H, W = 2, 40, 48
    boxes, doc = R.cfg2_like_boxes(rng, B, 24, H, W)
    feat = rng.standard_normal((B, H, W, C)).astype(np.float32)
    return feat, boxes, doc


def _close(got, ref, rtol=1e-5, atol=3e-5):
    got = got.double().cpu().numpy()
    err = np.abs(got - ref)
    assert float((err - (atol + rtol * np.abs(ref))).max()) <= 0, float(err.max())


@pytest.mark.parametrize("C", [256, 40])
@pytest.mark.parametrize("shape", SHAPES)
def test_roi_align_shapes_vs_restatement(shape, C):
    feat, boxes, doc = _case(C)
    B, H, W, _ = feat.shape
    f = torch.from_numpy(feat).to(DEV)
    bx, bd = torch.from_numpy(boxes).to(DEV), torch.from_numpy(doc).to(DEV)
    y = ops.roi_align_fwd(f, bx, bd, shape, 0.25)
    assert tuple(y.shape) == (len(boxes),) + shape + (C,)
    _close(y, R.roi_align_fwd(feat, boxes, doc, shape, 0.25))
    dy = np.random.default_rng(9).standard_normal(tuple(y.shape)).astype(np.float32)
    ref = R.roi_align_adjoint(dy, (B, H, W, C), boxes, doc, shape, 0.25)
    dyt = torch.from_numpy(dy).to(DEV)
    log = ops.dispatch_log(True)
    df = torch.zeros((B, H, W, C), device=DEV)
    ops.roi_align_bwd(dyt, (B, H, W, C), bx, bd, shape, 0.25, df)
    ops.dispatch_log(False)
    _close(df, ref)
    oh, ow = shape
    assert log.get("roi:sep" if oh * ow <= 64 and oh <= 8 and ow <= 32 else "roi:tap") == 1, log
    if shape == (8, 32):
        assert "roi:tap" in log and "roi:sep" not in log
    # deterministic backward: the adjoint, bitwise equal over two launches
    outs = []
    for _ in range(2):
        d2 = torch.zeros((B, H, W, C), device=DEV)
        with ops.deterministic_scope(True):
            ops.roi_align_bwd(dyt, (B, H, W, C), bx, bd, shape, 0.25, d2)
        torch.cuda.synchronize()
        outs.append(d2)
    assert torch.equal(outs[0], outs[1])
    _close(outs[0], ref)


@pytest.mark.parametrize("C", [256, 40])
def test_square_through_the_hw_entries_equals_the_int_entries(C):
    feat, boxes, doc = _case(C, seed=4)
    B, H, W, _ = feat.shape
    f = torch.from_numpy(feat).to(DEV)
    bx, bd = torch.from_numpy(boxes).to(DEV), torch.from_numpy(doc).to(DEV)
    assert torch.equal(ops.roi_align_fwd(f, bx, bd, 7, 0.25), ops.roi_align_fwd(f, bx, bd, (7, 7), 0.25))
    dy = torch.randn((len(boxes), 7, 7, C), device=DEV)
    with ops.deterministic_scope(True):
        a, b = torch.zeros((B, H, W, C), device=DEV), torch.zeros((B, H, W, C), device=DEV)
        ops.roi_align_bwd(dy, (B, H, W, C), bx, bd, 7, 0.25, a)
        ops.roi_align_bwd(dy, (B, H, W, C), bx, bd, (7, 7), 0.25, b)
    assert torch.equal(a, b)
    # the default backward adds with float atomics: equal up to the order of the additions
    a, b = torch.zeros((B, H, W, C), device=DEV), torch.zeros((B, H, W, C), device=DEV)
    ops.roi_align_bwd(dy, (B, H, W, C), bx, bd, 7, 0.25, a)
    ops.roi_align_bwd(dy, (B, H, W, C), bx, bd, (7, 7), 0.25, b)
    assert torch.allclose(a, b, rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------------------
LIN = "late_fusion_net.ROI_embedding_net.linear.weight"


def _build(roi_shape, mode="simp"):
    from transformers import BertTokenizer
    from model.ViBERTgrid_net import ViBERTgridNet
    cfg = e2e_cfg("resnet_18_fpn")
    tmp = pathlib.Path(tempfile.mkdtemp(prefix="vbg_roi_"))
    d = make_bert_dir(tmp, layers=2, vocab=1200, dropout=0.0)
    cwd = os.getcwd()
    os.chdir(str(tmp))
    try:
        net = ViBERTgridNet(num_classes=cfg.num_classes, image_mean=list(cfg.image_mean), image_std=list(cfg.image_std),
                            image_min_size=list(cfg.image_min_size), image_max_size=cfg.image_max_size,
                            test_image_min_size=cfg.test_image_min_size, bert_model="bert-base-uncased",
                            tokenizer=BertTokenizer(os.path.join(d, "vocab.txt")), backbone="resnet_18_fpn", grid_mode=cfg.grid_mode,
                            loss_weights=None, num_hard_positive_main_1=cfg.num_hard_positive_main_1,
                            num_hard_negative_main_1=cfg.num_hard_negative_main_1, num_hard_positive_main_2=cfg.num_hard_positive_main_2,
                            num_hard_negative_main_2=cfg.num_hard_negative_main_2,
                            loss_aux_sample_list=None if cfg.loss_aux_sample_list is None else list(cfg.loss_aux_sample_list),
                            num_hard_positive_aux=cfg.num_hard_positive_aux, num_hard_negative_aux=cfg.num_hard_negative_aux,
                            loss_control_lambda=cfg.loss_control_lambda, add_pos_neg=True, classifier_mode=mode,
                            ohem_random=cfg.ohem_random, layer_mode="single", work_mode="eval", roi_shape=roi_shape,
                            tag_to_idx={f"c{i}": i for i in range(cfg.num_classes)} if mode == "crf" else None)
    finally:
        os.chdir(cwd)
    return net, cfg


def _load(net, cfg):
    """the oracle's synthetic weights; the RoI linear (sized by h * w) gets seeded weights of its own"""
    shapes = O.state_shapes(cfg, vocab=1200)
    own = net.state_dict()
    sd = {k: v for k, v in O.synth_state_dict(shapes).items() if k in own and tuple(own[k].shape) == tuple(v.shape)}
    lin = own[LIN]
    g = torch.Generator().manual_seed(1234)
    sd[LIN] = torch.randn(tuple(lin.shape), generator=g) * (1.0 / float(np.sqrt(lin.shape[1])))
    net.load_state_dict(sd, strict=False)
    return net


def _batch():
    g = np.load(os.path.join(ROOT, "tests", "golden", "e2e.npz"))
    return to_dev(_e2e_inputs(g), DEV)


class _Capture:
    def __init__(self, net):
        self.d = {}
        self.h = [net.grid_roi_align_net.register_forward_hook(self._roi, with_kwargs=True),
                  net.late_fusion_net.register_forward_hook(self._fuse)]

    def _roi(self, mod, args, kwargs, out):
        packed = kwargs.get("packed")
        self.d.update(p_fuse=args[0].detach().clone(), boxes=packed[0].clone(), box_doc=packed[2].clone(), roi=out.detach().clone())

    def _fuse(self, mod, args, out):
        self.d.update(roi_in=args[0].detach().clone(), bert=(args[1] if isinstance(args[1], torch.Tensor) else torch.cat(list(args[1]))).detach().clone(),
                      fuse=out.detach().clone())
        if out.requires_grad:
            out.register_hook(lambda g: self.d.__setitem__("dfuse", g.detach().clone()))

    def close(self):
        for h in self.h:
            h.remove()


def _chain64(net, roi, bert, train):
    """fp64 CPU restatement of ROIEmbedding + the fusion linear from the module's own parameters -> (fuse, {name: leaf})"""
    F = torch.nn.functional
    lf = net.late_fusion_net
    e = lf.ROI_embedding_net
    P = {n: p.detach().double().cpu().clone().requires_grad_(True) for n, p in e.named_parameters()}
    x = roi.double().cpu().permute(0, 3, 1, 2)

    def bn(x, name):
        m = getattr(e, name)
        if train:
            mean, var = x.mean((0, 2, 3)), x.var((0, 2, 3), unbiased=False)
        else:
            mean, var = m.running_mean.double().cpu(), m.running_var.double().cpu()
        xh = (x - mean[None, :, None, None]) / torch.sqrt(var[None, :, None, None] + m.eps)
        return xh * P[name + ".weight"][None, :, None, None] + P[name + ".bias"][None, :, None, None]

    x = F.relu(bn(F.conv2d(x, P["conv_1.weight"], None, 1, 1), "bn_1"))
    x = F.relu(bn(F.conv2d(x, P["conv_2.weight"], None, 1, 1), "bn_2"))
    x = F.linear(x.flatten(1), P["linear.weight"], P["linear.bias"])
    q = lf.fuse_embedding_net.linear
    out = F.linear(torch.cat((x, bert.double().cpu()), 1), q.weight.detach().double().cpu(), q.bias.detach().double().cpu())
    return out, P


def _roi_restated(d, net):
    fm = d["p_fuse"].double().cpu().numpy()
    shape = net.grid_roi_align_net.output_size
    return R.roi_align_fwd(fm, d["boxes"].cpu().numpy(), d["box_doc"].cpu().numpy(), shape, net.grid_roi_align_net.spatial_scale)


def test_model_rectangular_roi_eval_and_train_vs_restatement():
    net, cfg = _build((3, 21))
    assert tuple(net.state_dict()[LIN].shape) == (1024, 256 * 63)
    _load(net, cfg)
    net = net.to(DEV)
    batch = _batch()
    cap = _Capture(net)
    try:
        # eval: running statistics
        net.eval()
        random.seed(1)
        with torch.no_grad():
            net(*batch)
        d = dict(cap.d)
        assert tuple(d["roi"].shape[1:3]) == (3, 21)
        _close(d["roi"], _roi_restated(d, net))
        ref, _ = _chain64(net, d["roi_in"], d["bert"], False)
        _close(d["fuse"], ref.detach().numpy(), rtol=1e-4, atol=1e-5)
        # one training step: batch statistics, and the RoI-embedding gradients against the fp64 VJP
        net.train()
        net.zero_grad(set_to_none=True)
        random.seed(7)
        loss = net(*batch)
        loss.backward()
        torch.cuda.synchronize()
        assert torch.isfinite(loss).all()
        d = dict(cap.d)
        _close(d["roi"], _roi_restated(d, net))
        ref, P = _chain64(net, d["roi_in"], d["bert"], True)
        _close(d["fuse"], ref.detach().numpy(), rtol=1e-4, atol=1e-5)
        ref.backward(d["dfuse"].double().cpu())
        for n, p in net.late_fusion_net.ROI_embedding_net.named_parameters():
            a, b = p.grad.double().cpu(), P[n].grad
            rel = float((a - b).norm() / b.norm().clamp_min(1e-30))
            assert rel <= 1e-4, (n, rel)
    finally:
        cap.close()


@pytest.mark.parametrize("mode", ["simp", "full", "crf"])
def test_model_rectangular_roi_heads_train_and_infer(mode):
    net, cfg = _build((3, 21), mode)
    _load(net, cfg)
    net = net.to(DEV).train()
    batch = _batch()
    random.seed(3)
    loss = net(*batch)
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all(), mode
    assert net.late_fusion_net.ROI_embedding_net.linear.weight.grad is not None
    if mode == "simp":
        random.seed(3)
        with torch.autocast("cuda", dtype=torch.float16):
            la = net(*batch)
        assert torch.isfinite(la).all()
        net.eval()
        imgs, segs, classes, coors, corpus, mask = batch
        with torch.no_grad():
            probs = net.inference(imgs, segs, coors, corpus, mask)
        n = sum(int(c.shape[0]) for c in classes)
        assert tuple(probs.shape) == (n, cfg.num_classes)
        assert torch.allclose(probs.sum(1), torch.ones(n, device=DEV), atol=1e-5)


def _det_step(roi_shape, log=None):
    net, cfg = _build(roi_shape)
    if isinstance(roi_shape, tuple) and roi_shape != (7, 7):
        _load(net, cfg)
    else:
        load_synth(net, cfg, 1200)
    net = net.to(DEV).train()
    batch = _batch()
    with ops.deterministic_scope(True):
        if log is not None:
            lg = ops.dispatch_log(True)
        random.seed(5)
        torch.manual_seed(5)
        loss = net(*batch)
        loss.backward()
        torch.cuda.synchronize()
        if log is not None:
            log.update(lg)
            ops.dispatch_log(False)
    return loss.detach().clone(), {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}


def test_model_rectangular_roi_deterministic():
    log = {}
    l1, g1 = _det_step((3, 21), log)
    l2, g2 = _det_step((3, 21))
    assert torch.equal(l1, l2)
    assert g1.keys() == g2.keys() and all(torch.equal(g1[k], g2[k]) for k in g1)
    assert "det:roi_align_bwd" in log and "fatomic:roi_align_bwd" not in log, sorted(log)
    # the square shape as a tuple runs the same kernels as the int
    la, ga = _det_step(7)
    lb, gb = _det_step((7, 7))
    assert torch.equal(la, lb)
    assert ga.keys() == gb.keys() and all(torch.equal(ga[k], gb[k]) for k in ga)


def test_model_roi_shape_list_is_a_type_error():
    with pytest.raises(TypeError):
        _build([3, 21])
