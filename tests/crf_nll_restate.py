"""The training loss of the linear-chain CRF and its gradient at marginal scale, restated in numpy fp64 from their definitions
(include/vbg.h vbg_crf_nll_stable), independent of the kernels and of torch.

trans[i, j] is the score of the transition j -> i; a path's score, Z and the marginals are those of tests/crf_posterior_restate.py.
For one document of n rows with the gold path `tags`:
    nll          (log Z - score(tags)) / n                                     (0 for n == 0)
    dem_unit     [n, T]: p(y_t = i | x) - [tags[t] == i]                       = d (n * nll) / d em[t, i]
    dtrans_unit  [T, T]: sum_t p(y_{t-1} = j, y_t = i | x) with y_{-1} = START, plus on row STOP p(y_{n-1} = j | x), minus the number
                 of times the gold path (START in front, STOP behind) takes j -> i  = d (n * nll) / d trans[i, j]

nll_and_grads   the two recursions in log space in fp64, every marginal as exp(alpha + beta - log Z): at fp64 the magnitudes of a
                document of a thousand rows cost 1e-12, not what they cost in fp32;
brute_force     every path enumerated, for tiny cases."""
import itertools
import math

import numpy as np

from crf_posterior_restate import path_score


def _lse(v, axis):
    m = v.max(axis=axis, keepdims=True)
    return np.squeeze(m, axis=axis) + np.log(np.exp(v - m).sum(axis=axis))


def gold_counts(tags, T, start, stop):
    c = np.zeros((T, T))
    p = start
    for k in tags:
        c[int(k), p] += 1.0
        p = int(k)
    c[stop, p] += 1.0
    return c


def nll_and_grads(em, tags, trans, start, stop):
    """em [n, T], tags [n] -> (nll, logz, dem_unit [n, T], dtrans_unit [T, T]) in fp64"""
    em = np.asarray(em, dtype=np.float64)
    trans = np.asarray(trans, dtype=np.float64)
    n, T = em.shape
    if n == 0:
        return 0.0, float(trans[stop, start]), np.zeros((0, T)), np.zeros((T, T))
    init = np.full(T, -10000.0)
    init[start] = 0.0
    alpha = np.zeros((n, T))
    prev = init
    for t in range(n):
        alpha[t] = em[t] + _lse(prev[None, :] + trans, axis=1)
        prev = alpha[t]
    logz = float(_lse(alpha[n - 1] + trans[stop], axis=0))
    beta = np.zeros((n, T))
    beta[n - 1] = trans[stop]
    for t in range(n - 2, -1, -1):
        beta[t] = _lse(trans + (em[t + 1] + beta[t + 1])[:, None], axis=0)          # over the tag i of row t + 1
    marg = np.exp(alpha + beta - logz)
    pair = np.zeros((T, T))
    for t in range(n):
        a = init if t == 0 else alpha[t - 1]
        pair += np.exp(a[None, :] + trans + (em[t] + beta[t])[:, None] - logz)
    pair[stop] += marg[n - 1]
    ind = np.zeros((n, T))
    ind[np.arange(n), np.asarray(tags, dtype=np.int64)] = 1.0
    nll = (logz - path_score(em, trans, start, stop, [int(k) for k in tags])) / n
    return nll, logz, marg - ind, pair - gold_counts(tags, T, start, stop)


def brute_force(em, tags, trans, start, stop):
    """the same four values from all T^n paths (n >= 1)"""
    em = np.asarray(em, dtype=np.float64)
    trans = np.asarray(trans, dtype=np.float64)
    n, T = em.shape
    paths = list(itertools.product(range(T), repeat=n))
    sc = np.array([path_score(em, trans, start, stop, y) for y in paths])
    mx = sc.max()
    w = np.exp(sc - mx)
    z = w.sum()
    logz = mx + math.log(z)
    marg = np.zeros((n, T))
    pair = np.zeros((T, T))
    for y, wy in zip(paths, w / z):
        marg[np.arange(n), list(y)] += wy
        pair += wy * gold_counts(y, T, start, stop)
    ind = np.zeros((n, T))
    ind[np.arange(n), np.asarray(tags, dtype=np.int64)] = 1.0
    nll = (logz - path_score(em, trans, start, stop, [int(k) for k in tags])) / n
    return nll, logz, marg - ind, pair - gold_counts(tags, T, start, stop)
