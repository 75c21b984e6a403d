"""ViBERTgridNet.inference_entities end to end on a tiny net: every decoded field of every document with its span posterior (crf
mode), or every run of the class scores (simp mode).  Needs a real MI355X.

The crf net and its inputs are tests/test_gpu_crf_posterior_model.py's."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import crf_posterior_restate as R
import crf_span_restate as S
from test_gpu_crf_posterior_model import FIELDS, crf_net, one                         # noqa: F401  (crf_net is a fixture)
from test_gpu_model import build_product, load_synth, to_dev
from test_oracle_golden import _e2e_inputs, e2e_cfg


def table_of(net):
    from vbg import decode as D
    return D.tag_table(net.field_type_classification_head.tag_to_idx, FIELDS)


def same_runs(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()


@pytest.mark.parametrize("thresh", [None, 0.6])
def test_equals_its_pieces_and_the_restatement(crf_net, thresh):
    from vbg import decode as D
    net, inputs = crf_net
    table = table_of(net)
    crf = net.field_type_classification_head.crf_layer
    with torch.no_grad():
        got = net.inference_entities(*inputs, thresh=thresh, table=table)
        em, doc_off, lens = net._crf_emissions(*inputs)
        post = net.inference_posterior(*inputs)
    assert isinstance(got, D.FieldRuns) and len(got.runs) == 2 and got.doc_off == [0, lens[0], lens[0] + lens[1]]
    assert got.doc_off == doc_off.cpu().tolist() and all(n > 0 for n in lens)
    lm, lc = crf.path_logp(em, doc_off, post.path)
    hand = D.list_crf_fields(post, (lm, lc), table, len(FIELDS), thresh=thresh, doc_off=got.doc_off)
    same_runs(got.runs, hand.runs)
    assert torch.equal(got.cls, hand.cls) and torch.equal(got.score.view(torch.int32), hand.score.view(torch.int32))
    # the restatement, fed the net's emissions (fp64 from there on) and the device's marginals for the class scores
    start, stop = crf._ends()
    e64, t64 = em.cpu().numpy().astype(np.float64), crf.transitions.detach().cpu().numpy().astype(np.float64)
    path, marg = post.path.cpu().tolist(), post.marginals.cpu().numpy()
    for d in range(2):
        lo, hi = got.doc_off[d], got.doc_off[d + 1]
        wlm, wlc = S.path_logp(e64[lo:hi], t64, start, stop, path[lo:hi])
        cls, score = R.class_scores(marg[lo:hi], path[lo:hi], table.tag_class, thresh)
        want = S.list_runs(cls, score, [bool(table.tag_begin[t]) for t in path[lo:hi]], wlm, wlc, True)
        runs = got.runs[d]
        assert len(want) >= 1
        assert runs["start"].tolist() == [w[0] for w in want] and runs["len"].tolist() == [w[1] for w in want]
        assert runs["cls"].tolist() == [w[2] for w in want]
        assert np.array_equal(runs["mean"].view(np.int64), np.array([w[3] for w in want]).view(np.int64))
        err = np.abs(runs["logp"] - np.array([w[4] for w in want]))
        print("document", d, "runs", len(want), "max |logp - fp64| per row", float((err / runs["len"]).max()))
        assert bool((err <= 1e-4 * runs["len"]).all())
        assert bool((runs["logp"] <= 1e-4).all())


def test_two_documents_equal_two_calls(crf_net):
    net, inputs = crf_net
    table = table_of(net)
    with torch.no_grad():
        both = net.inference_entities(*inputs, table=table)
        singles = [net.inference_entities(*one(inputs, b), table=table) for b in range(2)]
    same_runs(both.runs, [singles[0].runs[0], singles[1].runs[0]])
    n0 = singles[0].doc_off[1]
    assert torch.equal(both.cls[:n0], singles[0].cls) and torch.equal(both.cls[n0:], singles[1].cls)


def test_entity_strings(crf_net):
    from vbg import decode as D
    net, inputs = crf_net
    with torch.no_grad():
        got = net.inference_entities(*one(inputs, 0), table=table_of(net))
    runs = got.runs[0]
    texts = [f"[{i}]" for i in range(got.doc_off[1])]
    for rule, sep in (("concat", ""), ("space_before", " ")):
        ents = D.entity_strings(runs, texts, join=rule, keep_background=True)
        assert len(ents) == len(runs)
        for (c, text, mean, prob), r in zip(ents, runs):
            s, ln = int(r["start"]), int(r["len"])
            assert c == int(r["cls"]) and text == sep.join(texts[s:s + ln]) and mean == float(r["mean"])
            assert prob == float(np.exp(r["logp"])) and 0.0 < prob <= 1.0 + 1e-4
    fields = D.entity_strings(runs, texts)
    assert [e[0] for e in fields] == [int(c) for c in runs["cls"] if c != 0]
    with pytest.raises(ValueError):
        D.entity_strings(runs, texts, join="tab")
    with pytest.raises(ValueError):
        D.entity_strings(runs, texts[:-1], keep_background=True)


def test_crf_without_a_table_raises(crf_net):
    net, inputs = crf_net
    with pytest.raises(ValueError):
        net.inference_entities(*inputs)


def test_a_simp_net_lists_the_runs_of_its_scores(golden, tmp_path):
    from vbg import decode as D
    cfg = e2e_cfg("resnet_18_fpn")                                                     # classifier_mode "simp"
    net = build_product(tmp_path, "resnet_18_fpn", cfg)
    load_synth(net, cfg, 1200)
    dev = torch.device("cuda")
    net = net.to(dev).eval()
    imgs, segs, _, coors, corpus, mask = to_dev(_e2e_inputs(golden("e2e.npz")), dev)
    with torch.no_grad():
        got = net.inference_entities(imgs, segs, coors, corpus, mask, thresh=0.3)
        pred = net.inference(imgs, segs, coors, corpus, mask)
    off = [0]
    for c in coors:
        off.append(off[-1] + int(c.shape[0]))
    assert got.doc_off == off and off[-1] == pred.shape[0]
    hand = D.list_fields(pred, thresh=0.3, doc_off=off)
    assert len(got.runs) == len(hand.runs) == len(coors)
    same_runs(got.runs, hand.runs)
    assert all(len(a) >= 1 for a in got.runs)
    texts = [f"[{i}]" for i in range(off[1])]
    ents = D.entity_strings(got.runs[0], texts, join="concat", keep_background=True)
    assert len(ents) == len(got.runs[0]) and all(e[3] is None for e in ents)
