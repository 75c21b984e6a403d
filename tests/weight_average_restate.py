"""Weight averaging restated on the host: torch's lerp statement (ATen/native/Lerp.h) in numpy fp32 with every operation rounded on
its own, the fp64 reference and the derived bound the kernel is held to, the operand builder the tests share, and a six-parameter
stand-in model over the LAYOUT of tests/test_optim_groups_host.py."""
import numpy as np
import torch

FLT_MAX = float(np.finfo(np.float32).max)
DENORMAL = float(np.float32(3e-45))          # 2 * 2^-149

# (a, p) pairs planted into both operands: a denormal against a normal (both ways), -0.0, a == p exactly (small, and at the top of the
# range), +-FLT_MAX whose difference overflows fp32 (both signs), FLT_MAX against a small value, an inf and a NaN
PLANTED = [(DENORMAL, 1.0), (-0.0, -0.0), (FLT_MAX, -FLT_MAX), (1.2345, 1.2345), (float("inf"), 1.0), (2.0, float("nan")),
           (-FLT_MAX, FLT_MAX), (1.0, DENORMAL), (FLT_MAX, FLT_MAX), (FLT_MAX, 1.0)]
OVERFLOWING = (2, 6)                          # the PLANTED pairs whose difference p - a is not an fp32 number


def lerp_restate(a, p, w):
    """avg <- lerp(avg, p, w): both branches of torch's statement, fp32, one rounding per operation"""
    a, p, w = np.asarray(a, np.float32), np.asarray(p, np.float32), np.float32(w)
    with np.errstate(all="ignore"):
        d = p - a
        if abs(w) < np.float32(0.5):
            return a + w * d
        return p - d * (np.float32(1) - w)


def lerp_f64(a, p, w):
    """a + w (p - a) in double, with the weight the kernel sees: double(float32(w))"""
    a, p = np.asarray(a, np.float64), np.asarray(p, np.float64)
    with np.errstate(all="ignore"):
        return a + float(np.float32(w)) * (p - a)


def lerp_bound(a, p):
    """|out - lerp_f64| <= 4 * 2^-24 * (|a| + |p|) + 2^-149 for w in [0, 1].  Derived, not measured: at most four roundings (the
    difference, 1 - w, the product, the sum), each at most 2^-24 relative on a quantity that is at most |a| + |p|; one ulp of the
    smallest denormal covers a result rounded below the normal range.  A fused product-sum has fewer roundings and stays inside."""
    a, p = np.asarray(a, np.float64), np.asarray(p, np.float64)
    return 4.0 * 2.0 ** -24 * (np.abs(a) + np.abs(p)) + 2.0 ** -149


def planted_positions(n):
    """{position: index into PLANTED}.  Short ranges: pair i at position i.  From 1023 elements on: every pair once in the body
    (5 + 97 i), and -- when the range has them -- once behind the first sweep of the capped grid (2048 blocks x 256 threads x 4
    elements) and in the last three elements, which the scalar tail owns"""
    if n < 1023:
        return {i: i for i in range(min(n, len(PLANTED)))}
    pos = {5 + 97 * i: i for i in range(len(PLANTED))}
    sweep = 2048 * 256 * 4
    if n > sweep + 4 * len(PLANTED):
        pos.update({sweep + 4 * i + 1: i for i in range(len(PLANTED))})
        pos.update({n - 1: 2, n - 2: 0, n - 3: 5})
    return pos


def operands(n, seed=0):
    """(a, p, positions): two fp32 vectors of n normal deviates with the PLANTED pairs in place"""
    from test_gpu_small_kernels import rnd
    a, p = rnd(n, seed=1000 + 2 * seed), rnd(n, seed=1001 + 2 * seed)
    pos = planted_positions(n)
    for i, k in pos.items():
        a[i], p[i] = PLANTED[k]
    return a, p, pos


class SixModel(torch.nn.Module):
    """parameters of test_optim_groups_host.LAYOUT (dots in the names replaced), registered in the REVERSE of the flat order, which is
    what vbg.optim.FlatGroup turns back into LAYOUT's offsets"""

    def __init__(self, layout, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        values = [(n.replace(".", "_"), torch.randn(*s, generator=g)) for n, s, _ in layout]
        for n, v in values[::-1]:
            self.register_parameter(n, torch.nn.Parameter(v))


def homed_six(layout, device, seed=0):
    """(model, its FlatGroup) on `device`"""
    from vbg.optim import FlatGroup
    model = SixModel(layout, seed).to(device)
    return model, FlatGroup(list(model.named_parameters()), device)
