"""The log posteriors of a given tag path under the linear-chain CRF and the listing of every run, restated in numpy fp64 from their
definitions (include/vbg.h vbg_crf_path_logp, vbg_field_runs, vbg_field_runs_tags), independent of the kernels and of torch.  Built
on tests/crf_posterior_restate.py (path scores, brute force, runs, the exact sums of the tags form) and tests/decode_restate.py.

With trans[i, j] the score of j -> i and beta_t[j] = log of the summed weight of everything behind row t given y_t = j
(beta_{n-1}[j] = trans[STOP, j]; beta_{t-1}[j] = log sum_i exp(trans[i, j] + em[t, i] + beta_t[i])), the chain's conditionals are
    log p(y_t = i | y_{t-1} = j, x) = trans[i, j] + em[t, i] + beta_t[i] - beta_{t-1}[j]
and the marginal of row t is exp(alpha_t + beta_t) over its sum.  A span's log posterior is the marginal of its first row plus the
conditionals of the rest: the chain is Markov given x.

path_logp    (lm, lc) of a path, both recursions in log space in fp64;
span_logp    lm[s] + sum of lc[s+1 .. e];
brute_span   the same by enumeration of every path, for tiny cases;
list_runs    every run (start, len, cls, mean, logp) of one document in row order, every run under its own class;
best_of      the best run per class taken from such a list: largest mean, earliest start, runs whose mean is 0 dropped."""
import itertools
import math

import numpy as np

import crf_posterior_restate as R


def _lse(v, axis=None):
    m = np.max(v, axis=axis, keepdims=True)
    out = m + np.log(np.sum(np.exp(v - m), axis=axis, keepdims=True))
    return out.reshape(()) if axis is None else np.squeeze(out, axis=axis)


def path_logp(em, trans, start, stop, y):
    """em [n, T], trans [T, T], y: n tags -> (lm [n], lc [n]) in fp64.  lc[0] = lm[0].  A tag outside [0, T) gives -inf on its row
    (lm and lc) and on the next row's lc."""
    em = np.asarray(em, dtype=np.float64)
    trans = np.asarray(trans, dtype=np.float64)
    n, T = em.shape
    lm, lc = np.full(n, -np.inf), np.full(n, -np.inf)
    if n == 0:
        return lm, lc
    alpha = np.zeros((n, T))
    prev = np.full(T, -10000.0)
    prev[start] = 0.0
    for t in range(n):
        alpha[t] = em[t] + _lse(trans + prev[None, :], axis=1)           # over the previous tag j of trans[i, j] + prev[j]
        prev = alpha[t]
    beta = np.zeros((n, T))
    beta[n - 1] = trans[stop]
    for t in range(n - 1, 0, -1):
        beta[t - 1] = _lse(trans + (em[t] + beta[t])[:, None], axis=0)   # over the tag i of row t of trans[i, j] + em[t, i] + beta[t, i]
    inside = [0 <= int(k) < T for k in y]
    for t in range(n):
        if not inside[t]:
            continue
        k = int(y[t])
        ab = alpha[t] + beta[t]
        lm[t] = ab[k] - float(_lse(ab))
        if t == 0:
            lc[t] = lm[t]
        elif inside[t - 1]:
            j = int(y[t - 1])
            lc[t] = trans[k, j] + em[t, k] + beta[t, k] - beta[t - 1, j]
    return lm, lc


def span_logp(lm, lc, s, e):
    """log P(y_s .. y_e = the path's tags | x), rows s .. e inclusive"""
    total = float(lm[s])
    for t in range(s + 1, e + 1):
        total += float(lc[t])
    return total


def brute_span(em, trans, start, stop, y, s, e):
    """the same probability from every one of the T^n paths (fp64): the share of Z held by the paths that agree with y on s .. e"""
    em = np.asarray(em, dtype=np.float64)
    trans = np.asarray(trans, dtype=np.float64)
    n, T = em.shape
    paths = list(itertools.product(range(T), repeat=n))
    sc = np.array([R.path_score(em, trans, start, stop, p) for p in paths])
    mx = sc.max()
    w = np.exp(sc - mx)
    hit = np.array([all(p[t] == y[t] for t in range(s, e + 1)) for p in paths])
    return math.log(w[hit].sum()) - math.log(w.sum())


def list_runs(cls, score, begin_rows, lm, lc, tags):
    """one document -> [(start, len, cls, mean, logp)] in row order.  tags=True: runs also break at begin_rows, mean = the int64 sum of
    rint(score * 2^30) / 2^30 / len (crf_posterior_restate.winners' rule), logp = span_logp; tags=False: runs of equal class, mean =
    the sequential fp64 sum / len (decode_restate.stage2's rule), logp = 0.0.  Every run under its own class."""
    cls = [int(c) for c in cls]
    out = []
    for s, ln in R.runs(cls, begin_rows if tags else [False] * len(cls)):
        if tags:
            total = 0
            for v in score[s:s + ln]:
                total += int(np.rint(float(v) * R.FIX))
            mean = float(total) / R.FIX / ln
            logp = span_logp(lm, lc, s, s + ln - 1)
        else:
            total = 0.0
            for v in score[s:s + ln]:
                total += float(v)
            mean = total / ln
            logp = 0.0
        out.append((s, ln, cls[s], mean, logp))
    return out


def best_of(run_list, C):
    """-> C entries, (start, len, mean) or None: per class the largest mean, then the earliest start; a run whose mean is 0 (its sum
    is 0) leaves no record"""
    out = [None] * C
    for s, ln, c, mean, _ in run_list:
        if mean == 0:
            continue
        if out[c] is None or mean > out[c][2]:
            out[c] = (s, ln, mean)
    return out
