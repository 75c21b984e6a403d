"""Field decoding on the device: the opt-in replacement of the per-segment loop that follows `inference()` / `validate`'s forward in
the reference (pipeline/train_val_utils.py:440-493, eval_SROIE.py:119-169, eval_EPHOIE.py, deployment/inference_SROIE.py:65-124,
deployment/inference_EPHOIE.py:31-81).  Classes, runs, run means and the winner of every class come from ONE launch
(ops.field_decode -> vbg_field_decode) and ONE device-to-host copy of the [ndoc, C] table of winners; the strings are joined here, on the
host, for the winning runs only.

    pred_key_list = field_strings(pred_label, num_classes, ocr_text, thresh=strcmp_tresh, join="space_before")

`pred_label` is the 2-D float32 device tensor the classifier returns ([N, C] scores; the reference applies softmax to it once more,
and so does the kernel).  Rows that hold NaN or infinities are outside the contract: their document's records are meaningless (nothing
faults or hangs).  C <= 64 and fewer than 2^20 segments per document, or the library reports an argument error.

The crf mode returns tags, not scores, and the reference has no such loop for it.  Its counterpart here takes the posterior of the
CRF (ViBERTgridNet.inference_posterior / CRF.posterior: Viterbi path + marginals, one launch) and gives the same table:

    table = tag_table(tag_to_idx, category_list)
    pred_key_list = crf_field_strings(net.inference_posterior(...), table, num_classes, ocr_text, thresh=strcmp_tresh)

A segment's class is the class of its Viterbi tag, its score the posterior of that CLASS (the sum of the marginals of the class's
tags); runs also break in front of a begin tag, means are exact (fixed-point sums), every run is filed under its own class -- the
last-run quirk of the score loop is not carried over -- and a run whose scores all round to 0 leaves no record (decode_tags ->
vbg_field_decode_tags, include/vbg.h).  Two launches and one device-to-host copy per document or batch.

Both tables keep ONE run per class: the SROIE / EPHOIE protocol, where a key occurs once per receipt.  A page with dozens of
question / answer / header entities needs every run -- list_fields / list_crf_fields (vbg_field_runs / vbg_field_runs_tags), and in
the crf mode each with the probability that its tags hold jointly, P(y_s .. y_e = the decoded tags | x), from CRF.path_logp:

    runs = net.inference_entities(image, seg_indices, coors, corpus, mask, table=tag_table(tag_to_idx, category_list))
    for cls, text, mean, prob in entity_strings(runs.runs[0], ocr_text[0]): ..."""
from collections import namedtuple

import numpy as np
import torch

from . import ops

# one record of the table: first segment of the run (relative to its document; -1: the class has no record), its length, its mean score
REC = np.dtype([("start", "<i4"), ("len", "<i4"), ("mean", "<f8")])

# cls int32 [N], score fp32 [N]: device tensors; best: numpy record array [ndoc, C] of REC (host); doc_off: the host row ranges
FieldDecode = namedtuple("FieldDecode", ["cls", "score", "best", "doc_off"])


def _join_space_before(texts):
    """validate (language "eng") and eval_SROIE: `" " + t`, no space after a trailing hyphen"""
    s = texts[0]
    for t in texts[1:]:
        s += t if s.endswith("-") else " " + t
    return s


def _join_concat(texts):
    """validate (language "chn"), eval_EPHOIE and deployment/inference_EPHOIE: plain concatenation"""
    return "".join(texts)


def _join_space_after(texts):
    """deployment/inference_SROIE: `t + " "`, no space after a segment appended behind a trailing hyphen"""
    s = texts[0]
    for t in texts[1:]:
        s += t if s.endswith("-") else t + " "
    return s


JOIN = {"space_before": _join_space_before, "concat": _join_concat, "space_after": _join_space_after}


def _check_pred_label(pred_label):
    if not (torch.is_tensor(pred_label) and pred_label.dim() == 2 and pred_label.dtype == torch.float32 and pred_label.is_cuda):
        what = (tuple(pred_label.shape), pred_label.dtype, pred_label.device) if torch.is_tensor(pred_label) else type(pred_label)
        raise TypeError(f"pred_label must be a 2-D float32 device tensor of class scores [N, C], got {what}")


def _segment_texts(ocr_text, n, join):
    """the n segment texts of a document (ocr_text itself, or entry 0 of the reference's batch tuple), and the join rule checked"""
    if join not in JOIN:
        raise ValueError(f"join must be one of {sorted(JOIN)}, got {join!r}")
    texts = ocr_text[0] if len(ocr_text) > 0 and not isinstance(ocr_text[0], str) else ocr_text
    if len(texts) != n:
        raise ValueError(f"{len(texts)} segment texts for {n} rows")
    return texts


def decode_fields(pred_label, thresh=None, doc_off=None):
    """-> FieldDecode.  thresh: the reference's `strcmp_tresh` (a Python float, compared in double; None at the deployment sites);
    doc_off: HOST row ranges of a batch of documents (ndoc + 1 ints; None: all rows are one document)."""
    _check_pred_label(pred_label)
    n, c = pred_label.shape
    off = [0, n] if doc_off is None else [int(v) for v in doc_off]
    cls, score, best = ops.field_decode(pred_label, off, thresh)
    table = best.cpu().numpy().view(REC).reshape(len(off) - 1, c)         # the one device-to-host copy
    return FieldDecode(cls, score, table, off)


def join_winners(table, texts, join="space_before"):
    """one document's row of winners (REC [C]) + its segment texts -> one string per class, "" for a class without a record"""
    rule = JOIN[join]
    return [rule(texts[int(r["start"]):int(r["start"]) + int(r["len"])]) if r["start"] >= 0 else "" for r in table]


def field_strings(pred_label, num_classes, ocr_text, thresh=None, join="space_before"):
    """The reference's `pred_key_list` of one document: one string per class (class 0 included; callers skip it).  ocr_text: the
    document's segment texts, or the reference's batch tuple whose entry 0 holds them (`ocr_text[0][seg_index]`)."""
    _check_pred_label(pred_label)
    if int(num_classes) != pred_label.shape[1]:
        raise ValueError(f"num_classes {num_classes} != pred_label.shape[1] {pred_label.shape[1]}")
    texts = _segment_texts(ocr_text, pred_label.shape[0], join)
    return join_winners(decode_fields(pred_label, thresh).best[0], texts, join)


# ---- the crf mode: tags + posterior marginals
# tag_class[k]: class of tag k; tag_begin[k]: 1 where tag k opens a new run even behind a row of its class (host lists of ntag ints)
TagTable = namedtuple("TagTable", ["tag_class", "tag_begin"])

_ENDS = ("<START>", "<STOP>")


def tag_table(tag_to_idx, category_list):
    """Dictionaries in the reference's format -> TagTable.  "O" and <START> / <STOP> map to class 0; "B-x" and "I-x" to the index of x
    in category_list.  A "B-x" tag is a begin tag exactly when the dictionary also has "I-x":
    the plain TAG_TO_IDX sets label every segment of a field "B-x", and there a B- tag says nothing about where a field starts.
    Indices must be 0 .. ntag - 1, each once; unknown names raise ValueError."""
    ntag = len(tag_to_idx)
    cats = list(category_list)
    tag_class, tag_begin = [None] * ntag, [0] * ntag
    for name, k in tag_to_idx.items():
        if not (isinstance(k, int) and 0 <= k < ntag) or tag_class[k] is not None:
            raise ValueError(f"tag indices must be 0 .. {ntag - 1}, each once: {name!r} -> {k!r}")
        if name == "O" or name in _ENDS:
            tag_class[k] = 0
            continue
        field = name[2:]
        if name[:2] not in ("B-", "I-") or field not in cats:
            raise ValueError(f"tag {name!r} is neither 'O', <START> / <STOP> nor 'B-x' / 'I-x' with x in category_list {cats}")
        tag_class[k] = cats.index(field)
        tag_begin[k] = int(name[:2] == "B-" and ("I-" + field) in tag_to_idx)
    return TagTable(tag_class, tag_begin)


def _posterior_parts(posterior):
    marginals, path = (posterior.marginals, posterior.path) if hasattr(posterior, "marginals") else posterior
    if not (torch.is_tensor(marginals) and marginals.dim() == 2 and marginals.dtype == torch.float32 and marginals.is_cuda):
        raise TypeError("marginals must be a 2-D float32 device tensor [N, ntag] (CRF.posterior's)")
    if not (torch.is_tensor(path) and path.dim() == 1 and path.dtype == torch.int32 and path.shape[0] == marginals.shape[0]):
        raise TypeError(f"path must be a 1-D int32 device tensor of {marginals.shape[0]} tags (CRF.posterior's)")
    return marginals, path


def decode_tags(posterior, table, num_classes, thresh=None, doc_off=None):
    """posterior: a CrfPosterior or (marginals, path); table: tag_table's -> FieldDecode, as decode_fields gives it for scores.
    One launch, one device-to-host copy."""
    marginals, path = _posterior_parts(posterior)
    n = marginals.shape[0]
    off = [0, n] if doc_off is None else [int(v) for v in doc_off]
    cls, score, best = ops.field_decode_tags(marginals, path, table.tag_class, table.tag_begin, num_classes, off, thresh)
    rec = best.cpu().numpy().view(REC).reshape(len(off) - 1, int(num_classes))     # the one device-to-host copy
    return FieldDecode(cls, score, rec, off)


def crf_field_strings(posterior, table, num_classes, ocr_text, thresh=None, join="space_before"):
    """`pred_key_list` of one document in the crf mode: one string per class, joined by the rules of field_strings"""
    marginals, _ = _posterior_parts(posterior)
    texts = _segment_texts(ocr_text, marginals.shape[0], join)
    return join_winners(decode_tags(posterior, table, num_classes, thresh).best[0], texts, join)


# ---- every run, not the winners: pages with many fields per class (FUNSD-style question / answer / header)
# one record of the listing: first segment of the run (relative to its document), its length, its class, its mean score and, in the
# crf mode, the log posterior of its tags holding jointly (the score modes have none: NaN in list_fields' records)
RUN = np.dtype([("start", "<i4"), ("len", "<i4"), ("cls", "<i4"), ("pad", "<i4"), ("mean", "<f8"), ("logp", "<f8")])

# cls int32 [N], score fp32 [N]: device tensors; runs: one RUN array per document, its runs in row order (host); doc_off: host row ranges
FieldRuns = namedtuple("FieldRuns", ["cls", "score", "runs", "doc_off"])


def _split_runs(runs, off, has_logp):
    rec = runs.cpu().numpy().view(RUN).reshape(-1)                          # the one device-to-host copy
    if not has_logp:
        rec["logp"] = np.nan                                                # (the kernel writes 0.0: log 1, which no score claims)
    out = []
    for lo, hi in zip(off[:-1], off[1:]):
        doc = rec[lo:hi]
        out.append(doc[doc["len"] > 0])
    return out


def list_fields(pred_label, thresh=None, doc_off=None):
    """decode_fields' classes, scores and runs with EVERY run listed -> FieldRuns (`logp` is NaN: class scores carry no joint
    probability).  Every run stands under its own class, the last one included.  One launch, one device-to-host copy."""
    _check_pred_label(pred_label)
    n = pred_label.shape[0]
    off = [0, n] if doc_off is None else [int(v) for v in doc_off]
    cls, score, runs = ops.field_runs(pred_label, off, thresh)
    return FieldRuns(cls, score, _split_runs(runs, off, False), off)


def list_crf_fields(posterior, path_logp, table, num_classes, thresh=None, doc_off=None):
    """posterior: a CrfPosterior or (marginals, path); path_logp: the (lm, lc) pair of CRF.path_logp for that path; table: tag_table's
    -> FieldRuns: decode_tags' classes, scores and runs with EVERY run listed, `logp` = log P(the run's tags | x) -- the constrained
    forward-backward confidence of the field.  One launch, one device-to-host copy."""
    marginals, path = _posterior_parts(posterior)
    lm, lc = path_logp
    n = marginals.shape[0]
    for name, v in (("lm", lm), ("lc", lc)):
        if not (torch.is_tensor(v) and v.dtype == torch.float32 and tuple(v.shape) == (n,) and v.is_cuda):
            raise TypeError(f"{name} must be a float32 device tensor of {n} values (CRF.path_logp's)")
    off = [0, n] if doc_off is None else [int(v) for v in doc_off]
    cls, score, runs = ops.field_runs_tags(marginals, path, lm, lc, table.tag_class, table.tag_begin, num_classes, off, thresh)
    return FieldRuns(cls, score, _split_runs(runs, off, True), off)


def entity_strings(doc_runs, texts, join="space_before", keep_background=False):
    """one document's RUN array + its segment texts -> [(cls, text, mean, prob)] in row order, prob = exp(logp), None where logp is
    NaN (the runs of list_fields; a crf document whose lm / lc held NaN); class-0 runs are left out unless keep_background."""
    if join not in JOIN:
        raise ValueError(f"join must be one of {sorted(JOIN)}, got {join!r}")
    rule = JOIN[join]
    out = []
    for r in doc_runs:
        c, s, ln = int(r["cls"]), int(r["start"]), int(r["len"])
        if c == 0 and not keep_background:
            continue
        if s < 0 or s + ln > len(texts):
            raise ValueError(f"run {s} .. {s + ln} does not fit {len(texts)} segment texts")
        out.append((c, rule(texts[s:s + ln]), float(r["mean"]), None if np.isnan(r["logp"]) else float(np.exp(r["logp"]))))
    return out
