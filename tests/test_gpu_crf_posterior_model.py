"""The crf mode's scored prediction path, end to end on a tiny net: ViBERTgridNet.inference_posterior -> vbg.decode.decode_tags /
crf_field_strings.  Needs a real MI355X.

The net is the one tests/test_gpu_model.py builds for its crf case (synthetic weights, the fixture's transitions), with a tag
dictionary in the reference's format so that vbg.decode.tag_table reads it."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import crf_posterior_restate as R
from test_gpu_model import build_product, make_bert_dir, to_dev
from test_oracle_golden import _e2e_inputs, e2e_cfg, modes_state

FIELDS = ["others", "company", "date", "address", "total"]


def build_crf_net(tmp_path, cfg, tag_to_idx):
    import os
    from transformers import BertTokenizer
    from model.ViBERTgrid_net import ViBERTgridNet
    d = make_bert_dir(tmp_path, layers=2, vocab=1200, dropout=0.0)
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        return ViBERTgridNet(num_classes=cfg.num_classes, image_mean=list(cfg.image_mean), image_std=list(cfg.image_std),
                             image_min_size=list(cfg.image_min_size), image_max_size=cfg.image_max_size,
                             test_image_min_size=cfg.test_image_min_size, bert_model="bert-base-uncased",
                             tokenizer=BertTokenizer(os.path.join(d, "vocab.txt")), backbone=cfg.backbone, grid_mode=cfg.grid_mode,
                             loss_weights=None, num_hard_positive_main_1=cfg.num_hard_positive_main_1,
                             num_hard_negative_main_1=cfg.num_hard_negative_main_1, num_hard_positive_main_2=cfg.num_hard_positive_main_2,
                             num_hard_negative_main_2=cfg.num_hard_negative_main_2,
                             loss_aux_sample_list=None if cfg.loss_aux_sample_list is None else list(cfg.loss_aux_sample_list),
                             num_hard_positive_aux=cfg.num_hard_positive_aux, num_hard_negative_aux=cfg.num_hard_negative_aux,
                             loss_control_lambda=1, add_pos_neg=True, classifier_mode="crf", ohem_random=cfg.ohem_random,
                             layer_mode=cfg.layer_mode, work_mode="eval", tag_to_idx=tag_to_idx)
    finally:
        os.chdir(cwd)


@pytest.fixture(scope="module")
def crf_net(golden, tmp_path_factory):
    g = golden("e2e_modes.npz")
    cfg, sd = modes_state(g, "crf")
    assert cfg.num_classes == len(FIELDS)
    tags = {"O": 0}
    for k, f in enumerate(FIELDS[1:], start=1):
        tags["B-" + f] = k
    net = build_crf_net(tmp_path_factory.mktemp("crf_net"), cfg, tags)
    assert not net.load_state_dict(sd, strict=False).unexpected_keys
    dev = torch.device("cuda")
    net = net.to(dev).eval()
    imgs, segs, _, coors, corpus, mask = to_dev(_e2e_inputs(golden("e2e.npz")), dev)
    return net, (imgs, segs, coors, corpus, mask)


def one(inputs, b):
    imgs, segs, coors, corpus, mask = inputs
    return imgs[b:b + 1], segs[b:b + 1], coors[b:b + 1], corpus[b:b + 1], mask[b:b + 1]


def test_path_is_inference_s(crf_net):
    net, inputs = crf_net
    for b in range(2):
        with torch.no_grad():
            tags = net.inference(*one(inputs, b))
            post = net.inference_posterior(*one(inputs, b))
        n = tags.shape[0]
        assert n > 0 and tuple(post.marginals.shape) == (n, len(FIELDS) + 2) and tuple(post.logz.shape) == (1,)
        assert torch.equal(post.path, tags.reshape(-1).int())
        assert float((post.marginals.sum(1) - 1).abs().max()) <= 64 * 2.0 ** -23
        assert float(post.logz[0]) >= float(post.score[0])


def test_two_documents_equal_two_calls(crf_net):
    net, inputs = crf_net
    with torch.no_grad():
        both = net.inference_posterior(*inputs)
        singles = [net.inference_posterior(*one(inputs, b)) for b in range(2)]
    n0 = singles[0].path.shape[0]
    assert both.path.shape[0] == n0 + singles[1].path.shape[0] and tuple(both.logz.shape) == (2,)
    for b, (lo, hi) in enumerate([(0, n0), (n0, both.path.shape[0])]):
        assert torch.equal(both.path[lo:hi], singles[b].path)
        assert torch.equal(both.marginals[lo:hi].view(torch.int32), singles[b].marginals.view(torch.int32))
        assert torch.equal(both.logz[b:b + 1].view(torch.int32), singles[b].logz.view(torch.int32))
        assert torch.equal(both.score[b:b + 1].view(torch.int32), singles[b].score.view(torch.int32))


@pytest.mark.parametrize("thresh", [None, 0.6])
def test_field_strings_equal_the_restatement(crf_net, thresh):
    from vbg import decode as D
    net, inputs = crf_net
    head = net.field_type_classification_head
    table = D.tag_table(head.tag_to_idx, FIELDS)
    assert table.tag_class == [0, 1, 2, 3, 4, 0, 0] and table.tag_begin == [0] * 7
    with torch.no_grad():
        post = net.inference_posterior(*one(inputs, 0))
    n = post.path.shape[0]
    texts = [f"[{i}]" for i in range(n)]
    got = D.crf_field_strings(post, table, len(FIELDS), (texts,), thresh=thresh, join="concat")
    _, _, win = R.decode_tags(post.marginals.cpu().numpy(), post.path.cpu().tolist(), table.tag_class, table.tag_begin, len(FIELDS), thresh)
    want = ["" if w is None else "".join(texts[w[0]:w[0] + w[1]]) for w in win]
    assert got == want and any(want)
    # the batch form: row ranges on the host, one launch for both documents
    with torch.no_grad():
        both = net.inference_posterior(*inputs)
    off = [0, n, both.path.shape[0]]
    table2 = D.decode_tags(both, table, len(FIELDS), thresh=thresh, doc_off=off)
    alone = D.decode_tags(post, table, len(FIELDS), thresh=thresh)
    assert table2.best.shape == (2, len(FIELDS))
    _, _, win1 = R.decode_tags(both.marginals.cpu().numpy()[n:], both.path.cpu().tolist()[n:], table.tag_class, table.tag_begin, len(FIELDS), thresh)
    assert [(-1 if w is None else w[0]) for w in win1] == table2.best["start"][1].tolist()
    assert alone.best["start"][0].tolist() == [(-1 if w is None else w[0]) for w in win]


def test_other_modes_raise(tmp_path):
    net = build_product(tmp_path, "resnet_18_fpn", e2e_cfg("resnet_18_fpn"))          # classifier_mode "simp"
    with pytest.raises(ValueError):
        net.inference_posterior(None, None, None, None, None)
