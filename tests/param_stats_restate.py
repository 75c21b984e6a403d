"""Per-parameter statistics restated on the host (include/vbg.h vbg_stats_rec / vbg_stats_total; csrc/stats.hip), written from the
definitions, not from the kernel: the record of a run of elements, the finish over a parameter's rows, the running table, the
hand-written values the restatement itself is pinned on, and brute-force helpers for the row table."""
import math

import numpy as np

BINS = 64
F16_OVER_BITS = 0x477FF000          # 65520.0f


def unscaled(x, scale):
    """what the pass classifies: x itself (scale None) or the one rounded fp32 product x * inv, inv = float32(1 / double(scale))"""
    x = np.asarray(x, dtype=np.float32)
    if scale is None:
        return x
    inv = np.float32(1.0 / float(np.float32(scale)))
    with np.errstate(all="ignore"):
        return (x * inv).astype(np.float32)


def bin_of(v):
    """the binade bin of finite non-zero fp32 values, from the exponent FIELD: e = field - 127 (a subnormal's field is 0: -127),
    bin = clamp(e + 46, 0, 63)"""
    field = (np.asarray(v, dtype=np.float32).view(np.uint32) >> 23) & 0xFF
    return np.clip(field.astype(np.int64) - 127 + 46, 0, BINS - 1)


def record(x, scale=None):
    """the record of the elements x (any count): dict of sumsq (exact: math.fsum of the exact double squares of the finite elements),
    amax_bits, nonfinite, zeros, over_f16, hist[64]"""
    v = unscaled(np.asarray(x, dtype=np.float32).reshape(-1), scale)
    a = v.view(np.uint32) & 0x7FFFFFFF
    finite = a < 0x7F800000
    nonzero = finite & (a != 0)
    d = v[finite].astype(np.float64)
    hist = np.bincount(bin_of(v[nonzero]), minlength=BINS).astype(np.int64) if nonzero.any() else np.zeros(BINS, dtype=np.int64)
    return {"sumsq": math.fsum((d * d).tolist()), "amax_bits": int(a[finite].max()) if finite.any() else 0,
            "nonfinite": int((~finite).sum()), "zeros": int((finite & (a == 0)).sum()),
            "over_f16": int((finite & (a >= F16_OVER_BITS)).sum()), "hist": hist}


def exact_sumsq(x):
    """the sum of the squares of the finite fp32 values x, rounded ONCE to double -- math.fsum's result, at numpy speed for vectors
    of millions: |x| = m * 2^e with an integer m < 2^24 (np.frexp), so x^2 = m^2 * 2^(2e) with m^2 < 2^48; per exponent the m^2 are
    summed as integers (their high and low 24 bits apart, so that 2^24 of them stay exact), the per-exponent sums are
    combined as Python integers, and the one division that is left is Python's correctly rounded integer division"""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    x = x[np.isfinite(x) & (x != 0)]
    if not len(x):
        return 0.0
    assert len(x) <= 1 << 24
    frac, exp = np.frexp(x.astype(np.float64))                     # |frac| in [0.5, 1): frac * 2^24 is the integer m
    m = np.abs(frac * float(1 << 24)).astype(np.uint64)
    assert np.array_equal(np.ldexp(m.astype(np.float64), exp - 24), np.abs(x).astype(np.float64))
    sq = m * m
    lo_e = int(exp.min())
    # (np.bincount adds in double: at most 2^24 terms below 2^24 each stay below 2^48, so every partial sum is an exact integer)
    hi = np.bincount(exp - lo_e, weights=(sq >> np.uint64(24)).astype(np.float64))
    lo = np.bincount(exp - lo_e, weights=(sq & np.uint64((1 << 24) - 1)).astype(np.float64))
    total = 0
    for k in range(len(hi)):
        total += ((int(hi[k]) << 24) + int(lo[k])) << (2 * k)
    shift = 2 * (lo_e - 24)                                         # total * 2^shift is the sum
    return total * (1 << shift) / 1 if shift >= 0 else total / (1 << -shift)


def finish(recs):
    """the records of one parameter's rows -> the parameter's record: sums (sumsq exactly, by fsum), amax the max"""
    return {"sumsq": math.fsum(r["sumsq"] for r in recs), "amax_bits": max([r["amax_bits"] for r in recs] + [0]),
            "nonfinite": sum(r["nonfinite"] for r in recs), "zeros": sum(r["zeros"] for r in recs),
            "over_f16": sum(r["over_f16"] for r in recs), "hist": sum((r["hist"] for r in recs), np.zeros(BINS, dtype=np.int64))}


def fold(total, last):
    """the running table of one parameter after one more update: counts and bins add, amax the max, sumsq the last value"""
    if total is None:
        total = {"sumsq": 0.0, "amax_bits": 0, "nonfinite": 0, "zeros": 0, "over_f16": 0, "updates": 0, "steps_nonfinite": 0,
                 "hist": np.zeros(BINS, dtype=np.int64)}
    return {"sumsq": last["sumsq"], "amax_bits": max(total["amax_bits"], last["amax_bits"]),
            "nonfinite": total["nonfinite"] + last["nonfinite"], "zeros": total["zeros"] + last["zeros"],
            "over_f16": total["over_f16"] + last["over_f16"], "updates": total["updates"] + 1,
            "steps_nonfinite": total["steps_nonfinite"] + (1 if last["nonfinite"] > 0 else 0), "hist": total["hist"] + last["hist"]}


def below(x):
    """the largest fp32 below the positive fp32 x"""
    return np.nextafter(np.float32(x), np.float32(0), dtype=np.float32)


def hand_values():
    """the hand-written list, fp32: +-2^e for every e in -149 .. 127, the largest fp32 below each power of two, the fp16 edges (65504,
    the largest fp32 below 65520, 65520, 65536; 2^-14 and its predecessor; 2^-25 and its neighbours), +-0, +-inf, NaNs of both signs,
    fp32 subnormals"""
    vals = []
    for e in range(-149, 128):
        p = np.float32(2.0 ** e)
        vals += [p, -p]
        if e > -149:
            vals.append(below(p))
    vals += [np.float32(65504.0), below(65520.0), np.float32(65520.0), np.float32(65536.0), below(65536.0)]
    vals += [np.float32(2.0 ** -14), below(2.0 ** -14), np.float32(2.0 ** -25), below(2.0 ** -25),
             np.nextafter(np.float32(2.0 ** -25), np.float32(1), dtype=np.float32)]
    vals += [np.float32(0.0), np.float32(-0.0), np.float32(np.inf), np.float32(-np.inf)]
    out = np.array(vals, dtype=np.float32)
    special = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFA00001, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00400000],
                       dtype=np.uint32).view(np.float32)          # NaNs of both signs (quiet and signalling), subnormals
    return np.concatenate([out, special])


def mixed_values(n, seed):
    """n fp32 values: normal draws over a few binades with the hand-written values planted at random places (all of them when n allows)"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * np.exp2(rng.integers(-30, 4, size=n))).astype(np.float32)
    hv = hand_values()
    k = min(n // 2, len(hv))
    if k:
        x[rng.choice(n, size=k, replace=False)] = hv[rng.choice(len(hv), size=k, replace=False)] if k < len(hv) else hv
    return x


def layout(numels):
    """offsets of parameters of `numels` elements in slots padded to 8 elements, and the buffer's length rounded up to 32
    (vbg.optim.FlatGroup's rule)"""
    offsets, o = [], 0
    for s in numels:
        offsets.append(o)
        o += (s + 7) // 8 * 8
    return offsets, (o + 31) // 32 * 32


def brute_rows(offsets, numels, chunk):
    """the row table by a plain loop -> ([(start, length, parameter)], row_ptr)"""
    rows, row_ptr = [], [0]
    for i, (off, n) in enumerate(zip(offsets, numels)):
        done = 0
        while done < n:
            length = min(chunk, n - done)
            rows.append((off + done, length, i))
            done += length
        row_ptr.append(len(rows))
    return rows, row_ptr
