"""Field decoding on the device: the opt-in replacement of the per-segment loop that follows `inference()` / `validate`'s forward in
the reference (pipeline/train_val_utils.py:440-493, eval_SROIE.py:119-169, eval_EPHOIE.py, deployment/inference_SROIE.py:65-124,
deployment/inference_EPHOIE.py:31-81).  Classes, runs, run means and the winner of every class come from ONE launch
(ops.field_decode -> vbg_field_decode) and ONE device-to-host copy of the [ndoc, C] table of winners; the strings are joined here, on the
host, for the winning runs only.

    pred_key_list = field_strings(pred_label, num_classes, ocr_text, thresh=strcmp_tresh, join="space_before")

`pred_label` is the 2-D float32 device tensor the classifier returns ([N, C] scores; the reference applies softmax to it once more,
and so does the kernel).  The tag vector of the crf mode is not an input of these functions.  Rows that hold NaN or infinities are
outside the contract: their document's records are meaningless (nothing faults or hangs).  C <= 64 and fewer than 2^20 segments per
document, or the library reports an argument error."""
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
    if join not in JOIN:
        raise ValueError(f"join must be one of {sorted(JOIN)}, got {join!r}")
    if int(num_classes) != pred_label.shape[1]:
        raise ValueError(f"num_classes {num_classes} != pred_label.shape[1] {pred_label.shape[1]}")
    texts = ocr_text[0] if len(ocr_text) > 0 and not isinstance(ocr_text[0], str) else ocr_text
    if len(texts) != pred_label.shape[0]:
        raise ValueError(f"{len(texts)} segment texts for {pred_label.shape[0]} rows")
    return join_winners(decode_fields(pred_label, thresh).best[0], texts, join)
