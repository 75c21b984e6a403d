"""Validation metrics on the device: the token-level and entity-level scores of `validate` (pipeline/train_val_utils.py:348-665 of the
reference; pipeline/criteria.py token_F1_criteria, token_classification_criteria, BIO_F1_criteria) without keeping a tensor per
document and without a host read per document.  Every forward adds a few dozen integers to one device table in ONE launch
(ops.seq_metrics -> vbg_seq_metrics, csrc/metrics.hip); the epoch ends with one small all_reduce and ONE device-to-host copy.

    m = SequenceMetrics(num_classes, tag_to_idx=TAG_TO_IDX)
    for batch in loader:
        ...
        m.update(pred_label, gt_label)          # in place of pred_gt_list.append(...)
    m.all_reduce()
    p, r, f = m.entity_scores("micro"); print(m.report()); d = m.token_f1()

Entities follow seqeval's default mode (get_entities on IOB / IOBES tags, precision_recall_fscore_support); the package itself is not
needed.  Not offered: seqeval's `scheme=` / strict mode, `suffix=True`, and the byte layout of its report.  token_f1() reproduces the
reference's literal counts (`pred_label.int()` truncates the SCORES; on softmax outputs nearly every cell is zero): confusion() is the
useful token-level quantity."""
from collections import namedtuple

import numpy as np
import torch

from . import ops
from .lib import TagTable

MAX_CLASSES = 64
MAX_TYPES = 64
PREFIX = {"O": 0, "B": 1, "I": 2, "E": 3, "S": 4}         # include/vbg.h VBG_TAG_*

# entity int64 [T, 3] (n_true, n_pred, n_correct per type), confusion int64 [C, C] (gt, predicted), token int64 [C, 4] (TP, TN, FP, FN)
Counts = namedtuple("Counts", ["entity", "confusion", "token"])


def split_tag(tag):
    """seqeval's reading of a tag: its first letter and its type, `_` without one ("B-PER" -> ("B", "PER"), "O" -> ("O", "_"))"""
    return tag[0], tag[1:].split("-", 1)[-1] or "_"


def parse_tags(tag_to_idx, num_classes):
    """the reference's tag dict -> (type names in sorted order, prefix code per class, type id per class)"""
    tag_of = {int(v): str(k) for k, v in tag_to_idx.items()}
    missing = [k for k in range(num_classes) if k not in tag_of]
    if missing:
        raise ValueError(f"tag_to_idx has no tag for class index {missing[0]}")
    parts = []
    for k in range(num_classes):
        tag = tag_of[k]
        if not tag or tag[0] not in PREFIX:
            raise ValueError(f"tag {tag!r} of class {k}: the prefix must be one of O, B, I, E, S")
        parts.append(split_tag(tag))
    types = sorted({ty for _, ty in parts})
    if len(types) > MAX_TYPES:
        raise ValueError(f"{len(types)} entity types, at most {MAX_TYPES}")
    return types, [PREFIX[p] for p, _ in parts], [types.index(ty) for _, ty in parts]


def _ratio(num, den):
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    return np.divide(num, den, out=np.zeros(np.broadcast(num, den).shape), where=den != 0)


class SequenceMetrics:
    def __init__(self, num_classes, tag_to_idx=None, device=None):
        self.num_classes = int(num_classes)
        if not 1 <= self.num_classes <= MAX_CLASSES:
            raise ValueError(f"num_classes {num_classes} outside 1 .. {MAX_CLASSES}")
        self.types, self._table = [], TagTable()
        if tag_to_idx is not None:
            self.types, prefix, type_id = parse_tags(tag_to_idx, self.num_classes)
            for k in range(self.num_classes):
                self._table.prefix[k], self._table.type[k] = prefix[k], type_id[k]
        self._has_tags = tag_to_idx is not None
        c, t = self.num_classes, len(self.types)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self._counts = torch.zeros(3 * t + c * c + 4 * c, dtype=torch.int64, device=self.device)
        self._host = None

    # ---- accumulation: device only ------------------------------------------------------------------------------------------------
    def update(self, pred_label, gt_label, doc_off=None):
        """One launch on the current stream, no host read.  pred_label: the 2-D float32 device tensor of class scores [N, C], or a 1-D
        integer device tensor of predicted tags (the crf head); gt_label: a 1-D integer device tensor [N].  doc_off: HOST row ranges of
        the sequences (ndoc + 1 ints, as vbg.decode.decode_fields takes them); None: all rows are ONE sequence, which is what validate
        hands seqeval per batch."""
        int_types = (torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64)
        if not (torch.is_tensor(pred_label) and pred_label.is_cuda and ((pred_label.dim() == 2 and pred_label.dtype == torch.float32) or
                                                                        (pred_label.dim() == 1 and pred_label.dtype in int_types))):
            what = (tuple(pred_label.shape), pred_label.dtype, pred_label.device) if torch.is_tensor(pred_label) else type(pred_label)
            raise TypeError(f"pred_label must be a 2-D float32 device tensor of class scores [N, C] or a 1-D integer device tensor of tags, got {what}")
        if not (torch.is_tensor(gt_label) and gt_label.is_cuda and gt_label.dim() == 1 and gt_label.dtype in int_types):
            what = (tuple(gt_label.shape), gt_label.dtype, gt_label.device) if torch.is_tensor(gt_label) else type(gt_label)
            raise TypeError(f"gt_label must be a 1-D integer device tensor [N], got {what}")
        n = pred_label.shape[0]
        if gt_label.shape[0] != n:
            raise ValueError(f"{gt_label.shape[0]} gt labels for {n} rows")
        if pred_label.dim() == 2 and pred_label.shape[1] != self.num_classes:
            raise ValueError(f"pred_label.shape[1] {pred_label.shape[1]} != num_classes {self.num_classes}")
        off = [0, n] if doc_off is None else [int(v) for v in doc_off]
        gt = self._labels_i32(gt_label)
        scores = pred_label.contiguous() if pred_label.dim() == 2 else None
        tags = self._labels_i32(pred_label) if pred_label.dim() == 1 else None
        ops.seq_metrics(gt, off, self.num_classes, len(self.types), self._table, self._counts, scores=scores, pred_tags=tags)
        self._host = None

    def _labels_i32(self, labels):
        """int32 labels for the kernel.  A 64-bit label outside [0, C) becomes -1 on the device before the cast, which would otherwise
        wrap it (2^32 + 1 -> 1) into a class that counts; narrower dtypes fit int32 as they are.  No host read."""
        if labels.dtype == torch.int64:
            labels = torch.where((labels < 0) | (labels >= self.num_classes), -1, labels)
        return labels.to(torch.int32).contiguous()

    def all_reduce(self, group=None):
        """one dist.all_reduce(SUM) of the table; nothing without an initialised process group"""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(self._counts, op=dist.ReduceOp.SUM, group=group)
            self._host = None

    def reset(self):
        self._counts.zero_()
        self._host = None

    # ---- the one copy, and arithmetic on the host ---------------------------------------------------------------------------------
    def counts(self):
        """-> Counts of numpy int64 arrays: the one device-to-host copy (kept until the next update / all_reduce / reset)"""
        if self._host is None:
            flat = self._counts.cpu().numpy()
            c, t = self.num_classes, len(self.types)
            self._host = Counts(flat[:3 * t].reshape(t, 3), flat[3 * t:3 * t + c * c].reshape(c, c), flat[3 * t + c * c:].reshape(c, 4))
        return self._host

    def load_counts(self, flat):
        """replace the table (a saved one, or one merged elsewhere): VBG_METRICS_COUNTS(T, C) integers in the layout of include/vbg.h"""
        flat = torch.as_tensor(np.asarray(flat, dtype=np.int64).reshape(-1))
        if flat.numel() != self._counts.numel():
            raise ValueError(f"{flat.numel()} counts, the table of {len(self.types)} types and {self.num_classes} classes has {self._counts.numel()}")
        self._counts.copy_(flat)
        self._host = None

    def confusion(self):
        """[C, C] rows by gt class and predicted class"""
        return self.counts().confusion.copy()

    def accuracy(self):
        """token_classification_criteria's (num_correct, num_entities) summed over the updates"""
        conf = self.counts().confusion
        return float(np.trace(conf)), int(conf.sum())

    def token_f1(self):
        """the dict token_F1_criteria returns, key for key, from the literal counts (updates with scores only)"""
        out = {}
        for k, (tp, tn, fp, fn) in enumerate(self.counts().token.tolist()):
            precision = tp / (tp + fp + 1e-8)
            recall = tp / (tp + fn + 1e-8)
            out[k] = {"TP": tp, "TN": tn, "FP": fp, "FN": fn, "precision": precision, "recall": recall,
                      "F1": 2 * precision * recall / (precision + recall + 1e-8)}
        out["num_classes"] = self.num_classes
        return out

    def _entity_table(self):
        if not self._has_tags:
            raise ValueError("entity scores need the tag table: SequenceMetrics(num_classes, tag_to_idx=...)")
        ent = self.counts().entity
        used = [i for i in range(len(self.types)) if ent[i, 0] or ent[i, 1]]          # the types that occur in true or pred
        return [self.types[i] for i in used], ent[used, 0], ent[used, 1], ent[used, 2]

    def entity_scores(self, average="micro"):
        """(precision, recall, f1) as seqeval's precision_recall_fscore_support gives them, a zero denominator giving 0: "micro" from the
        summed counts, "macro" the plain mean over the types that occur in true or pred, "weighted" by n_true (0 without any), None:
        three arrays over those types, sorted by name"""
        if average not in ("micro", "macro", "weighted", None):
            raise ValueError(f"average must be 'micro', 'macro', 'weighted' or None, got {average!r}")
        _, n_true, n_pred, n_ok = self._entity_table()
        if average == "micro":
            n_true, n_pred, n_ok = n_true.sum(keepdims=True), n_pred.sum(keepdims=True), n_ok.sum(keepdims=True)
        p, r = _ratio(n_ok, n_pred), _ratio(n_ok, n_true)
        f = _ratio(2 * p * r, p + r)
        if average is None:
            return p, r, f
        if average == "micro":
            return float(p[0]), float(r[0]), float(f[0])
        if average == "macro":
            weight = np.ones(len(p))
        else:
            weight = n_true.astype(np.float64)
        total = float(weight.sum())
        if total == 0.0:
            return 0.0, 0.0, 0.0
        return float((p * weight).sum() / total), float((r * weight).sum() / total), float((f * weight).sum() / total)

    def report_dict(self):
        """{type: {precision, recall, f1-score, support}} plus "micro avg", "macro avg", "weighted avg" """
        names, n_true, _, _ = self._entity_table()
        p, r, f = self.entity_scores(None)
        out = {name: {"precision": float(p[i]), "recall": float(r[i]), "f1-score": float(f[i]), "support": int(n_true[i])}
               for i, name in enumerate(names)}
        for avg in ("micro", "macro", "weighted"):
            ap, ar, af = self.entity_scores(avg)
            out[f"{avg} avg"] = {"precision": ap, "recall": ar, "f1-score": af, "support": int(n_true.sum())}
        return out

    def report(self, digits=2):
        """a text table per type and the three averages (the columns of seqeval's classification_report, not its byte layout)"""
        d = self.report_dict()
        width = max([len(k) for k in d] + [12])
        lines = [f"{'':>{width}} {'precision':>10} {'recall':>10} {'f1-score':>10} {'support':>10}", ""]
        for name, row in d.items():
            if name == "micro avg":
                lines.append("")
            lines.append(f"{name:>{width}} {row['precision']:>10.{digits}f} {row['recall']:>10.{digits}f} {row['f1-score']:>10.{digits}f} {row['support']:>10d}")
        return "\n".join(lines) + "\n"
