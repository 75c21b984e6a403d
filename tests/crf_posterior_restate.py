"""The posterior of the linear-chain CRF and the field decoding over tags, restated in numpy fp64 from their definitions (include/vbg.h
vbg_crf_posterior, vbg_field_decode_tags), independent of the kernels and of torch.

trans[i, j] is the score of the transition j -> i.  A path y_0 .. y_{n-1} has the score
    trans[y_0, START] + sum_t em[t, y_t] + sum_{t >= 1} trans[y_t, y_{t-1}] + trans[STOP, y_{n-1}],
Z is the sum of exp(score) over all paths and the marginal p(y_t = i | x) the share of Z held by the paths with y_t = i.

forward_backward   the two recursions in the linear domain, each vector divided by its sum at every step (the sums' logs add up
                   to log Z), each row of marginals divided by its own sum;
brute_force        every path enumerated, for tiny cases;
viterbi            first maximum on ties, as torch.max takes it;
tag_table          the rule of vbg.decode.tag_table;
decode_tags        classes, class posteriors, runs, exact means (int64 sums of rint(score * 2^30)), winners."""
import itertools
import math

import numpy as np

FIX = float(2 ** 30)


def forward_backward(em, trans, start, stop):
    """em [n, T], trans [T, T] -> (logz, marginals [n, T]) in fp64; n == 0: (trans[stop, start], empty)"""
    em = np.asarray(em, dtype=np.float64)
    trans = np.asarray(trans, dtype=np.float64)
    n, T = em.shape
    if n == 0:
        return float(trans[stop, start]), np.zeros((0, T))
    # linear-domain factors with the row / step maxima taken out; what is taken out is added back to log Z
    tmax = trans.max()
    E = np.exp(trans - tmax)                                # E[i, j]: j -> i
    alpha = np.zeros((n, T))
    logz = 0.0
    prev = np.zeros(T)
    prev[start] = 1.0
    for t in range(n):
        emax = em[t].max()
        a = np.exp(em[t] - emax) * (E @ prev)
        s = a.sum()
        alpha[t] = a / s
        prev = alpha[t]
        logz += math.log(s) + emax + tmax
    end = E[stop] @ prev
    logz += math.log(end) + tmax
    beta = np.zeros((n, T))
    nxt = E[stop].copy()
    beta[n - 1] = nxt / nxt.sum()
    for t in range(n - 2, -1, -1):
        w = np.exp(em[t + 1] - em[t + 1].max()) * beta[t + 1]
        b = E.T @ w                                         # b[j] = sum_i E[i, j] w[i]
        beta[t] = b / b.sum()
    m = alpha * beta
    return logz, m / m.sum(axis=1, keepdims=True)


def path_score(em, trans, start, stop, y):
    s, p = 0.0, start
    for t, k in enumerate(y):
        s += float(trans[k, p]) + float(em[t, k])
        p = k
    return s + float(trans[stop, p])


def brute_force(em, trans, start, stop):
    """-> (logz, marginals, best path, best score) over all T^n paths (fp64); ties in the best score take the first path found"""
    em = np.asarray(em, dtype=np.float64)
    trans = np.asarray(trans, dtype=np.float64)
    n, T = em.shape
    paths = list(itertools.product(range(T), repeat=n))
    sc = np.array([path_score(em, trans, start, stop, y) for y in paths])
    mx = sc.max()
    w = np.exp(sc - mx)
    z = w.sum()
    m = np.zeros((n, T))
    for y, wy in zip(paths, w):
        for t, k in enumerate(y):
            m[t, k] += wy
    k = int(sc.argmax())
    return mx + math.log(z), m / z, list(paths[k]), float(sc[k])


def viterbi(em, trans, start, stop):
    """-> (path, score): max over the previous tag with the FIRST maximum on ties, then + em (model/crf.py:99-145)"""
    em = np.asarray(em, dtype=np.float64)
    trans = np.asarray(trans, dtype=np.float64)
    n, T = em.shape
    prev = np.full(T, -10000.0)
    prev[start] = 0.0
    back = []
    for t in range(n):
        v = prev[None, :] + trans                           # v[i, j]
        bj = v.argmax(axis=1)                               # numpy takes the first maximum
        back.append(bj)
        prev = v[np.arange(T), bj] + em[t]
    term = prev + trans[stop]
    cur = int(term.argmax())
    score = float(term[cur])
    path = []
    for bj in reversed(back):
        path.append(cur)
        cur = int(bj[cur])
    return path[::-1], score


def tag_table(tag_to_idx, category_list):
    """-> (tag_class, tag_begin): "O", <START>, <STOP> -> class 0; "B-x" / "I-x" -> index of x; B-x begins a run iff I-x exists"""
    ntag = len(tag_to_idx)
    if sorted(tag_to_idx.values()) != list(range(ntag)):
        raise ValueError("indices")
    cls, beg = [0] * ntag, [0] * ntag
    for name, k in tag_to_idx.items():
        if name in ("O", "<START>", "<STOP>"):
            continue
        if name[:2] not in ("B-", "I-") or name[2:] not in category_list:
            raise ValueError(name)
        cls[k] = list(category_list).index(name[2:])
        beg[k] = 1 if name[:2] == "B-" and "I-" + name[2:] in tag_to_idx else 0
    return cls, beg


def class_scores(marginals, path, tag_class, thresh=None):
    """marginals: fp32 array [n, T] -> (cls list, score list of np.float32): the class of the row's tag; the fp32 sum in increasing tag
    order of the row's marginals over that class's tags; a score that, as a double, is below thresh sends the row to class 0"""
    m = np.asarray(marginals, dtype=np.float32)
    cls, score = [], []
    for r, tag in enumerate(path):
        c = int(tag_class[int(tag)])
        s = np.float32(0.0)
        for k in range(m.shape[1]):
            if tag_class[k] == c:
                s = np.float32(s + m[r, k])
        if thresh is not None and float(s) < float(thresh):
            c = 0
        cls.append(c)
        score.append(s)
    return cls, score


def runs(cls, begin_rows):
    """-> [(start, len)]: a run starts at row 0, where the class changes, and at every row of begin_rows"""
    n = len(cls)
    starts = [i for i in range(n) if i == 0 or cls[i] != cls[i - 1] or begin_rows[i]]
    return [(s, (starts[k + 1] if k + 1 < len(starts) else n) - s) for k, s in enumerate(starts)]


def winners(cls, score, begin_rows, C):
    """-> C entries, (start, len, mean) or None.  Sums are int64 sums of rint(score * 2^30); mean = sum / 2^30 / len, rounded once;
    every run is filed under its own class; a run whose sum is 0 leaves no record; largest mean, then earliest start"""
    out = [None] * C
    for s, ln in runs(cls, begin_rows):
        total = 0
        for v in score[s:s + ln]:
            total += int(np.rint(float(v) * FIX))
        if total == 0:
            continue
        mean = float(total) / FIX / ln
        c = cls[s]
        if out[c] is None or mean > out[c][2]:
            out[c] = (s, ln, mean)
    return out


def decode_tags(marginals, path, tag_class, tag_begin, C, thresh=None):
    """one document -> (cls, score, winners)"""
    cls, score = class_scores(marginals, path, tag_class, thresh)
    begin_rows = [bool(tag_begin[int(t)]) for t in path]
    return cls, score, winners(cls, score, begin_rows, C)
