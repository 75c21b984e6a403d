"""Field decoding restated in plain Python from its definition (include/vbg.h vbg_field_decode), independent of the kernel, of torch
and of the reference's loop: the reference interleaves classification, string building and filing in one pass with carried
variables; here the steps are separate and each is written as what it MEANS.

Stage 1 (rows):     p = softmax(x[i]) in fp64; cls[i] = first index of max p; score[i] = p[cls[i]]; a threshold t sends a row with
                    score[i] < t to class 0 (the score stays).
Stage 2 (records):  a run is a maximal stretch of equal cls -- (start, len, mean), mean = the sum of its scores, added left to right
                    in double, over len.  Every run is filed under its own class, except the LAST one, which the reference files
                    under the class of row N - 2 (for N == 1: class C - 1, Python's index -1).  Filing order = order of start.  The
                    winner of a class is the first filed record with the strictly greatest mean; a class without a record has none.
Strings:            the winner's segment texts joined by one of the three rules of the reference's call sites."""
import math


def stage1(x, thresh=None):
    """x: rows of C numbers -> (cls list, score list), fp64"""
    cls, score = [], []
    for row in x:
        v = [float(a) for a in row]
        m = max(v)
        e = [math.exp(a - m) for a in v]
        s = math.fsum(e)
        p = [a / s for a in e]
        top = max(p)
        cls.append(p.index(top))
        score.append(top)
    return threshold(cls, score, thresh), score


def threshold(cls, score, thresh):
    """a row whose score, AS A DOUBLE, is below the double `thresh` goes to class 0 (None: no threshold)"""
    if thresh is None:
        return [int(c) for c in cls]
    return [0 if float(s) < float(thresh) else int(c) for c, s in zip(cls, score)]


def runs(cls):
    """-> [(start, len)] of the maximal stretches of equal class"""
    n = len(cls)
    starts = [i for i in range(n) if i == 0 or cls[i] != cls[i - 1]]
    return [(s, (starts[k + 1] if k + 1 < len(starts) else n) - s) for k, s in enumerate(starts)]


def stage2(cls, score, C):
    """(cls, score) of one document -> winners: a list of C entries, (start, len, mean) or None"""
    cls = [int(c) for c in cls]
    n = len(cls)
    filed = [[] for _ in range(C)]
    rs = runs(cls)
    for k, (s, ln) in enumerate(rs):
        total = 0.0
        for v in score[s:s + ln]:
            total += float(v)
        if k + 1 < len(rs):
            where = cls[s]
        else:
            where = C - 1 if n == 1 else cls[n - 2]
        filed[where].append((s, ln, total / ln))
    winners = []
    for recs in filed:
        top = None
        for r in recs:
            if top is None or r[2] > top[2]:
                top = r
        winners.append(top)
    return winners


def join(texts, rule):
    if rule == "concat":
        return "".join(texts)
    out = texts[0]
    for t in texts[1:]:
        if out.endswith("-"):
            out += t
        elif rule == "space_before":
            out += " " + t
        elif rule == "space_after":
            out += t + " "
        else:
            raise ValueError(rule)
    return out


def strings(winners, texts, rule):
    return ["" if w is None else join(list(texts[w[0]:w[0] + w[1]]), rule) for w in winners]


def decode(x, C, texts, thresh=None, rule="concat"):
    cls, score = stage1(x, thresh)
    return strings(stage2(cls, score, C), texts, rule)
