"""Plain-Python restatement of what vbg_seq_metrics counts (csrc/metrics.hip; vbg/metrics.py): seqeval's default-mode entity walk as
published (get_entities / start_of_chunk / end_of_chunk) in its SEQUENTIAL form, the per-type set intersection of
precision_recall_fscore_support, and the literal counts of the reference's pipeline/criteria.py token_F1_criteria.  Lists and ints
only; imports neither vbg nor torch."""


def split_tag(tag):
    """first letter, and the type behind the first '-' ('_' without one)"""
    return tag[0], tag[1:].split("-", 1)[-1] or "_"


def end_of_chunk(pt, t, pty, ty):
    if pt in ("E", "S"):
        return True
    if pt in ("B", "I") and t in ("B", "S", "O"):
        return True
    return pt != "O" and pty != ty


def start_of_chunk(pt, t, pty, ty):
    if t in ("B", "S"):
        return True
    if pt in ("E", "S", "O") and t in ("E", "I"):
        return True
    return t != "O" and pty != ty


def get_entities(tags):
    """one sequence of tag strings -> [(type, first row, last row)]; a virtual 'O' follows the last row, an 'O' stands in front"""
    out = []
    pt, pty, begin = "O", "_", 0
    for i, tag in enumerate(list(tags) + ["O"]):
        t, ty = split_tag(tag)
        if end_of_chunk(pt, t, pty, ty):
            out.append((pty, begin, i - 1))
        if start_of_chunk(pt, t, pty, ty):
            begin = i
        pt, pty = t, ty
    return out


def entity_counts(true_seqs, pred_seqs):
    """lists of sequences -> {type: [n_true, n_pred, n_correct]}; sequences carry nothing into each other"""
    out = {}
    for s, (tr, pr) in enumerate(zip(true_seqs, pred_seqs)):
        assert len(tr) == len(pr)
        et = {(ty, s, a, b) for ty, a, b in get_entities(tr)}
        ep = {(ty, s, a, b) for ty, a, b in get_entities(pr)}
        for ty in {e[0] for e in et | ep}:
            row = out.setdefault(ty, [0, 0, 0])
            row[0] += sum(1 for e in et if e[0] == ty)
            row[1] += sum(1 for e in ep if e[0] == ty)
            row[2] += sum(1 for e in et & ep if e[0] == ty)
    return out


def trunc(v):
    """`tensor.int()` of one finite float: toward zero"""
    return int(v)


def token_counts(rows, gt, num_classes):
    """token_F1_criteria's literal counts: rows = lists of class scores, gt = class per row -> [[TP, TN, FP, FN]] per class"""
    out = []
    for c in range(num_classes):
        tp = sum(1 for x, g in zip(rows, gt) if g == c and trunc(x[c]) == 1)
        tn = sum(1 for x, g in zip(rows, gt) if g != c and trunc(x[c]) == 0)
        fp = sum(1 for x, g in zip(rows, gt) if g != c and trunc(x[c]) == 1)
        fn = sum(1 for x, g in zip(rows, gt) if g == c and trunc(x[c]) == 0)
        out.append([tp, tn, fp, fn])
    return out


def token_f1(counts):
    """the rest of token_F1_criteria's dict from the counts"""
    out = {}
    for c, (tp, tn, fp, fn) in enumerate(counts):
        p = tp / (tp + fp + 1e-8)
        r = tp / (tp + fn + 1e-8)
        out[c] = {"TP": tp, "TN": tn, "FP": fp, "FN": fn, "precision": p, "recall": r, "F1": 2 * p * r / (p + r + 1e-8)}
    out["num_classes"] = len(counts)
    return out


def confusion(pred_cls, gt, num_classes):
    out = [[0] * num_classes for _ in range(num_classes)]
    for p, g in zip(pred_cls, gt):
        out[g][p] += 1
    return out
