"""Device sampling and OHEM selection restated in plain numpy, independent of the library (no import of vbg), from the contract in
include/vbg.h (a13b) and the hash of csrc/vbg_common.h as tests/row_restate.py states it.

sample_select.  Category c of a label array = {i : (labels[i] == value_c) == bool(eq_c)}, n_c elements.  The key of element i is the
whole 64-bit hash rng_state(seed, stream0 + c, i); keys of distinct i are distinct (idx * odd + const mod 2^64 is injective, the
finaliser is a bijection).  n_c > k_c: the k_c elements with the smallest keys, in ascending key order.  n_c <= k_c: every element,
in ascending element index.  keep_c = min(k_c, n_c).

Seeds.  Plan number `counter` of a process takes counter * 0x9E3779B1 + (torch seed & 0xFFFFFFFF) + rank * 0x85EBCA6B; the stream id of
category c is 0x10000 + c.

OHEM.  si = the positions of a list ordered by (loss descending, position ascending), where "descending" is the order of the radix
sort's keys: the ascending code of a float is its bits with the sign bit set (sign clear) or all bits flipped (sign set), so a NaN
with a clear sign bit stands before +inf, and +0 before -0.  The reference keeps `sorted_loss[sorted_index[:k]]`, i.e. the elements at
positions si[si[r]], r < k, when the list is longer than k, and the whole list otherwise."""
import numpy as np

from row_restate import U64, rng_state

STREAM0 = 0x10000
MASK64 = 0xFFFFFFFFFFFFFFFF


def step_seed(counter, torch_seed, rank=0):
    return counter * 0x9E3779B1 + (torch_seed & 0xFFFFFFFF) + rank * 0x85EBCA6B


def members(labels, value, eq):
    labels = np.asarray(labels)
    return np.nonzero((labels == value) == bool(eq))[0].astype(np.int64)


def keys_of(seed, stream, idx):
    return rng_state(seed & MASK64, stream, np.asarray(idx).astype(U64))


def sample_select(labels, cats, seed, stream0=STREAM0):
    """cats: [(value, eq, k)] -> ([list of element indices per category, order included], keep [ncat], n [ncat])"""
    lists, keep, n = [], [], []
    for c, (value, eq, k) in enumerate(cats):
        m = members(labels, value, eq)
        if len(m) > k:
            key = keys_of(seed, stream0 + c, m)
            m = m[np.argsort(key, kind="stable")[:k]]
        lists.append(m)
        keep.append(len(m))
        n.append(int(((np.asarray(labels) == value) == bool(eq)).sum()))
    return lists, keep, n


def desc_code(loss_f32):
    """uint32 whose ASCENDING order is the descending order of the radix keys"""
    b = np.asarray(loss_f32, np.float32).view(np.uint32)
    asc = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))
    return ~asc


def sort_desc_positions(loss_f32):
    """si: si[r] = position of rank r (stable: ties keep ascending position)"""
    return np.argsort(desc_code(loss_f32), kind="stable")


def ohem_choice(loss_f32, k):
    """positions (into the list) the reference keeps, in its order; the whole list when it has at most k entries"""
    m = len(loss_f32)
    if m <= k:
        return np.arange(m)
    si = sort_desc_positions(loss_f32)
    return si[si[:k]]
