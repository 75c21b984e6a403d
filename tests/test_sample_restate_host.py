"""CPU checks of tests/sample_restate.py -- the numpy statement of vbg_sample_select and of vbg_ohem_topk's permutation that the GPU
tests compare the kernels with (tests/test_gpu_sample_select.py, tests/test_gpu_ohem_device.py)."""
import numpy as np
import pytest

import sample_restate as S
from row_restate import rng_state, rng_u32

M64 = (1 << 64) - 1


def hash_by_hand(seed, sid, idx):
    """csrc/vbg_common.h rng_u64 in python integers"""
    z = (seed + 0x9E3779B97F4A7C15 * (sid + 1) + idx * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 30
    z = z * 0xBF58476D1CE4E5B9 & M64
    z ^= z >> 27
    z = z * 0x94D049BB133111EB & M64
    z ^= z >> 31
    return z


def test_known_answers_n8():
    """seed 7, labels [1 0 1 1 2 1 0 1]; category 0 = (== 1), k 3, stream 0x10000; category 1 = (!= 1), k 2, stream 0x10001.
    Keys (top 16 bits) of category 0's members 0 2 3 5 7: c11c 748a 7a85 88b6 f5cb -> the three smallest in key order: 2 3 5.
    Keys of category 1's members 1 4 6: ca93 a263 9882 -> 6 4."""
    labels = [1, 0, 1, 1, 2, 1, 0, 1]
    assert [hash_by_hand(7, 0x10000, i) >> 48 for i in (0, 2, 3, 5, 7)] == [0xc11c, 0x748a, 0x7a85, 0x88b6, 0xf5cb]
    assert [hash_by_hand(7, 0x10001, i) >> 48 for i in (1, 4, 6)] == [0xca93, 0xa263, 0x9882]
    for i in range(8):
        assert int(rng_state(7, 0x10000, i)) == hash_by_hand(7, 0x10000, i)
        assert int(rng_u32(7, 0x10000, i)) == (hash_by_hand(7, 0x10000, i) >> 16) & 0xFFFFFFFF          # rng_u32 = bits 16 ... 47
    lists, keep, n = S.sample_select(labels, [(1, 1, 3), (1, 0, 2)], 7)
    assert [l.tolist() for l in lists] == [[2, 3, 5], [6, 4]] and keep == [3, 2] and n == [5, 3]


@pytest.mark.parametrize("k", [1, 4, 32])
@pytest.mark.parametrize("delta", ["empty", -1, 0, 1])
def test_sizes_around_k_and_order_rules(k, delta):
    """n_c in {0, k-1, k, k+1}: everything in ascending index up to k, the k smallest keys in key order beyond"""
    nc = 0 if delta == "empty" else k + delta
    rng = np.random.default_rng(100 * k + nc)
    labels = np.full(97, 5, np.int32)
    pos = np.sort(rng.choice(97, nc, replace=False))
    labels[pos] = 2
    (got,), (keep,), (n,) = S.sample_select(labels, [(2, 1, k)], seed=99)
    assert n == nc and keep == min(k, nc) == len(got)
    if nc <= k:
        assert got.tolist() == pos.tolist()                                            # ascending element index
    else:
        keys = [hash_by_hand(99, S.STREAM0, int(i)) for i in pos]
        want = [int(i) for _, i in sorted(zip(keys, pos))][:k]
        assert got.tolist() == want                                                    # ascending key
        assert got.tolist() != sorted(want) or k == 1


def test_eq0_and_foreign_labels():
    labels = np.array([3, 0, 0, 9, -4, 0, 7], np.int32)
    lists, keep, n = S.sample_select(labels, [(0, 0, 16), (0, 1, 16), (8, 1, 16)], seed=1)
    assert lists[0].tolist() == [0, 3, 4, 6] and lists[1].tolist() == [1, 2, 5] and lists[2].tolist() == []
    assert keep == [4, 3, 0] == n


def test_keys_distinct_over_a_million_indices():
    for seed, sid in ((0, S.STREAM0), (S.step_seed(41, 1234, 3), S.STREAM0 + 3)):
        z = rng_state(seed & M64, sid, np.arange(1_000_000, dtype=np.uint64))
        assert np.unique(z).size == z.size


def _reference_quirk(loss, k):
    """pipeline/custom_loss.py:165-190 of the reference, line by line, on one category's losses (stable sort flavour):
        sorted_loss, sorted_index = torch.sort(loss, descending=True); keep = sorted_loss[sorted_index[:k]]
    -> the positions (into `loss`) of the values it keeps"""
    order = sorted(range(len(loss)), key=lambda p: (-float(loss[p]), p))          # descending, ties by position
    sorted_index = order
    if len(loss) <= k:
        return list(range(len(loss)))
    return [sorted_index[j] for j in sorted_index[:k]]          # sorted_loss[j] is the loss at position sorted_index[j]


def test_quirk_permutation_with_ties():
    rng = np.random.default_rng(5)
    for m, k in ((9, 4), (33, 32), (64, 7), (5, 5), (4, 6)):
        loss = rng.integers(0, 4, m).astype(np.float32) * 0.5          # many exact ties, some +0
        assert S.ohem_choice(loss, k).tolist() == _reference_quirk(loss, k)
    # a NaN (label out of range) sorts first, like the radix key order; +0 ties keep their positions' order
    loss = np.array([0.0, 2.0, np.nan, 0.0, 2.0], np.float32)
    assert S.sort_desc_positions(loss).tolist() == [2, 1, 4, 0, 3]
    assert S.ohem_choice(loss, 2).tolist() == [4, 1]


def test_step_seed_rule():
    assert S.step_seed(0, 0x1_0000_0005) == 5 and S.step_seed(2, 1, rank=3) == 2 * 0x9E3779B1 + 1 + 3 * 0x85EBCA6B


def test_uniform_inclusion_over_600_step_seeds():
    """labels arange(4096) % 3, category == 1 (1365 elements), k = 100, the seeds of plans 0 ... 599 under torch seed 0.  Every element is
    included with probability p = k / n per draw; with the finite-population correction (n - 1) / n the statistic
    sum (x_i - T p)^2 / (T p (1 - p)) has mean n - 1 = 1364 and variance ~ 2 * 1364.  |z| <= 4 is a condition on these fixed inputs
    (z = 2.13 here; 1.31 and 0.45 under torch seeds 1234 and 12345)."""
    labels = np.arange(4096) % 3
    T, k, n = 600, 100, 1365
    cnt = np.zeros(4096, np.int64)
    for t in range(T):
        (l,), (keep,), _ = S.sample_select(labels, [(1, 1, k)], S.step_seed(t, 0))
        assert keep == k and np.unique(l).size == k
        cnt[l] += 1
    assert cnt[labels != 1].sum() == 0                                  # nothing outside the category is ever drawn
    p = k / n
    chi2 = float(((cnt[labels == 1] - T * p) ** 2).sum() / (T * p * (1 - p)) * (n - 1) / n)
    z = (chi2 - (n - 1)) / np.sqrt(2 * (n - 1))
    print(f"chi2 {chi2:.1f} z {z:.2f}")
    assert abs(z) <= 4
