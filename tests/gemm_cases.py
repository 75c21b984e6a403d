"""Case table of the generic GEMM / implicit-GEMM convolution kernel family (csrc/gemm.hip), shared by the host test
(tests/test_gemm_variant_host.py: every case reaches the kernel instance it names) and the GPU test (tests/test_gpu_gemm_variants.py:
every case against an fp64 reference).  A plain module, like the *_restate.py files: torch on the CPU only, no library call.

A case names the operand-kind pair, the shapes and leading dimensions, pointer offsets, the convolution geometry, the arithmetic form
and tile it asks for, the epilogue / alpha / accumulate / split, segments or groups, and `expect`: the tuple vbg_gemm_variant must
report for it, { BM, BN, BK, vec, prec, splitk in effect, staged store, accumulate in effect }.  The table derives `expect` from what
the case ASKS for with rules written out below (never from the library), so a change of the dispatch heuristic that moves a case to
another instance fails the host test instead of thinning the GPU test out.

Shapes are the smallest that still hold the edge: M and N are one tile of the instance under test plus a ragged tail, reductions sit
off the k-tile depth, operand rows are padded with NaN (the kernel's contract: reduction chunks at or beyond K are never touched, rows
outside the operand read as zero), C carries two spare rows and four spare columns of a sentinel.

Not in scope: non-square filters (kh != kw) and asymmetric padding -- no wrapper of vbg/ops.py produces them.
"""
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

f32, f64 = torch.float32, torch.float64

# include/vbg.h operand kinds (tests/test_gemm_variant_host.py checks them against vbg.lib)
DENSE_K, DENSE_R, CONV_K, CONV_R, WT_R = 0, 1, 2, 3, 4
EPI_NONE, EPI_RELU, EPI_GELU_DUAL = 0, 1, 2
# pair name -> (a_kind, b_kind): dense forward / data gradient / weight gradient, convolution forward / data gradient / weight gradient
PAIRS = {"KK": (DENSE_K, DENSE_K), "KR": (DENSE_K, DENSE_R), "RR": (DENSE_R, DENSE_R),
         "CK": (CONV_K, DENSE_K), "CW": (CONV_K, WT_R), "RC": (DENSE_R, CONV_R)}

# ---- the instantiation list of launch_pair (csrc/gemm.hip), written out: (BM, BN, BK, vec, prec) ------------------------------------
SCALAR = (64, 64, 16, 0, 0)
FP32_TILES = [(64, 64, 16, 1, 0), (128, 64, 16, 1, 0), (128, 128, 16, 1, 0), (64, 64, 32, 1, 0), (128, 64, 32, 1, 0), (128, 128, 32, 1, 0)]
AMP_TILES = [(64, 64, 32, 1, 1), (128, 128, 32, 1, 1)]
SPLIT_TILES = [(64, 64, 32, 1, 3), (128, 128, 16, 1, 3), (128, 128, 32, 1, 3)]
F16_TILE = (64, 64, 32, 1, 2)
INSTANCES = {p: [SCALAR] + FP32_TILES + AMP_TILES + SPLIT_TILES + ([F16_TILE] if p in ("KK", "CK") else []) for p in PAIRS}
# instances no descriptor reaches
UNREACHABLE = {
    ("CW", SCALAR): "the scalar-load path needs a_vec == 0 or b_vec == 0, and the dispatch forces both to 1 for this pair: A is the gathered "
                    "CONV_K operand, B the WT_R weights, whose base must be 16-byte aligned and whose row length N a multiple of 4 (argument "
                    "errors otherwise)",
}

SENTINEL = -777.25
# rows of sentinel behind C: the two the edge needs, and a whole 128-row tile more, so that a kernel that stores the tail rows of its last
# tile writes into the sentinel (and fails the test) instead of outside the allocation
SPARE_ROWS = 2 + 128
BOUND = 2e-6          # |got - ref| / (|a| @ |b|) for K <= 640: tests/test_gpu_kernels.py::test_split_form_is_fp32_grade's bound, unchanged


def bound_for(K):
    return BOUND if K <= 640 else BOUND * math.sqrt(K / 640.0)


def up4(n):
    return (n + 3) // 4 * 4


def request(v):
    """(form, tile, bk) that asks gemm_raw for instance v (vbg/ops.py: under the split and amp forms a requested bk = 16 is dropped, so the
    16-deep tiles of the fp32 form are asked for under form "fp32"; the six-product 128 x 128 tile runs 16 deep unless bk = 32)"""
    BM, BN, BK, vec, prec = v
    tile = BM * 1000 + BN
    if not vec:
        return "split", 0, 0          # whatever is asked for: unaligned operands take the scalar-load path first
    if prec == 0:
        return "fp32", tile, BK
    if prec == 1:
        return "amp", tile, 0
    if prec == 2:
        return "f16", tile, 0
    return "split", tile, 32 if (BM, BK) == (128, 32) else 0


def stages(v):
    """does the instance store its tile through LDS?  Every bf16 / fp16 form does; of the fp32 form, the 16-deep k-tiles under a 128-row
    tile have no room (gemm_stages_tile, worked out for all six pairs: 128 * (BN + 4) floats against two buffers of 16-deep tiles)"""
    BM, BN, BK, vec, prec = v
    return not (prec == 0 and BM == 128 and BK == 16)


@dataclass(frozen=True)
class Case:
    name: str
    pair: str
    v: Tuple[int, int, int, int, int]          # the instance the case is built to reach
    M: int = 0
    N: int = 0
    K: int = 0
    lda: Optional[int] = None                  # None: the operand's row length rounded up to 4 (NaN in the padding)
    ldb: Optional[int] = None
    a_off: int = 0                             # pointer offsets (elements)
    b_off: int = 0
    c_off: int = 0
    ldc: Optional[int] = None                  # None: N rounded up to 4, plus 4
    form: Optional[str] = None                 # None: request(v); "fp32" / "amp" / "split" / "f16"
    tile: Optional[int] = None
    bk: Optional[int] = None
    epi: str = "none"                          # none / bias / bias_relu / gelu (GELU-dual, with bias)
    alpha: float = 1.0
    accumulate: bool = False
    splitk: int = 1                            # 0: the automatic split
    auto_splitk: int = 0                       # what the automatic split is expected to choose (splitk = 0)
    slab: bool = False                         # deterministic split: slabs + vbg_slab_reduce (bias, ReLU)
    c_nan: bool = False                        # C prefilled with NaN instead of the sentinel
    stats: bool = False
    a_relu_scale: Optional[float] = None
    conv: Optional[Tuple[int, ...]] = None     # (B, H, W, Cin, Cout, k, stride, pad): x [B, H, W, Cin], filter [Cout, k, k, Cin]
    segs: Optional[Tuple[Tuple[int, int], ...]] = None      # ((channels, shift), ...) of a DENSE_K A on the map seg_map = (B, H, W)
    seg_map: Optional[Tuple[int, int, int]] = None
    groups: Optional[Tuple[Tuple[int, int, int], ...]] = None          # ((M, N, K), ...)

    @property
    def request(self):
        f, t, b = request(self.v)
        return (self.form or f, t if self.tile is None else self.tile, b if self.bk is None else self.bk)

    @property
    def expect(self):
        sk = self.auto_splitk if self.splitk == 0 else self.splitk
        acc = int(self.accumulate or (self.splitk == 0 and sk > 1))
        ldc = self.ldc_eff
        staged = stages(self.v) and not (acc and sk > 1) and ldc % 4 == 0 and self.c_off % 4 == 0
        return tuple(self.v) + (max(sk, 1), int(staged), acc)

    @property
    def dims(self):
        """(M, N, K) of the product"""
        if self.conv is None:
            if self.groups:
                return max(g[0] for g in self.groups), max(g[1] for g in self.groups), max(g[2] for g in self.groups)
            return self.M, self.N, self.K
        B, H, W, Cin, Cout, k, st, pd = self.conv
        Ho, Wo = (H + 2 * pd - k) // st + 1, (W + 2 * pd - k) // st + 1
        if self.pair == "CK":
            return B * Ho * Wo, Cout, k * k * Cin
        if self.pair == "CW":
            return B * H * W, Cin, k * k * Cout
        return Cout, k * k * Cin, B * Ho * Wo

    @property
    def ldc_eff(self):
        return up4(self.dims[1]) + 4 if self.ldc is None else self.ldc


# =====================================================================================================================================
# the table
# =====================================================================================================================================
def _mn(v, n_mult4=False):
    """one tile plus a ragged tail for the instance's own BM / BN"""
    return v[0] + 2, v[1] + (4 if n_mult4 else 1)


def _dense_cases():
    out = []
    for pair in ("KK", "KR", "RR"):
        for v in INSTANCES[pair]:
            M, N = _mn(v)
            tag = f"{pair}-{v[0]}x{v[1]}x{v[2]}-v{v[3]}p{v[4]}"
            for K in (6, 32, 70, 200):
                kw = {}
                if not v[3]:
                    # the scalar-load path: A's leading dimension is its row length as it is, no multiple of 4 (K = 6 and lda = K = 70 for a
                    # K-contiguous A, M = 66 for a row-contiguous one), or B / A start one float off
                    kw = {6: {"lda": 66 if pair == "RR" else 6}, 32: {"b_off": 1}, 70: {"lda": 66 if pair == "RR" else 70}, 200: {"a_off": 1}}[K]
                out.append(Case(f"{tag}-K{K}", pair, v, M=M, N=N, K=K, **kw))
            sc = {} if v[3] else {"b_off": 1}
            # output: every epilogue on the staged path (ldc % 4 == 0, aligned C) and on the per-lane path (ldc % 4 != 0; C one float off)
            if pair == "KK":
                for epi in ("none", "bias", "bias_relu", "gelu"):
                    out.append(Case(f"{tag}-{epi}-staged", pair, v, M=M, N=N, K=70, epi=epi, **sc))
                    out.append(Case(f"{tag}-{epi}-ldc", pair, v, M=M, N=N, K=70, epi=epi, ldc=up4(N) + 5, **sc))
                    out.append(Case(f"{tag}-{epi}-coff", pair, v, M=M, N=N, K=70, epi=epi, c_off=1, **sc))
            # alpha, accumulate, splits: K = 200 is 7 k-tiles of 32 (3 + 3 + 1; six splits: 2 2 2 1 0 0) and 13 of 16 (5 + 5 + 3; six
            # splits: 3 3 3 3 1 0) -- a k-tile count no multiple of 3, and a last split that owns no k-tile
            out.append(Case(f"{tag}-alpha", pair, v, M=M, N=N, K=200, alpha=-0.5, epi="bias", **sc))
            out.append(Case(f"{tag}-alpha-acc", pair, v, M=M, N=N, K=200, alpha=-0.5, accumulate=True, **sc))
            out.append(Case(f"{tag}-acc", pair, v, M=M, N=N, K=200, accumulate=True, epi="bias", **sc))
            out.append(Case(f"{tag}-acc-ldc", pair, v, M=M, N=N, K=200, accumulate=True, ldc=up4(N) + 6, **sc))
            out.append(Case(f"{tag}-acc-split3", pair, v, M=M, N=N, K=200, accumulate=True, splitk=3, epi="bias", **sc))
            out.append(Case(f"{tag}-acc-split6", pair, v, M=M, N=N, K=200, accumulate=True, splitk=6, alpha=-0.5, **sc))
            # a_prologue max(a, 0) * a_scale: K-contiguous (KK, KR) and row-contiguous (RR) A; under amp the reference rounds after it
            if pair in ("KK", "RR"):
                out.append(Case(f"{tag}-prologue", pair, v, M=M, N=N, K=70, a_relu_scale=0.375, **sc))
    # M < 4 and N = 1, dense forward pair: default forms and the scalar path
    for v in (F16_TILE, (64, 64, 16, 1, 0), (128, 128, 32, 1, 3), SCALAR):
        sc = {} if v[3] else {"b_off": 1}
        tag = f"KK-{v[0]}x{v[1]}x{v[2]}-v{v[3]}p{v[4]}"
        out.append(Case(f"{tag}-M3", "KK", v, M=3, N=v[1] + 1, K=70, epi="bias", **sc))
        out.append(Case(f"{tag}-N1", "KK", v, M=v[0] + 2, N=1, K=70, epi="bias", **sc))
        out.append(Case(f"{tag}-N1-coff", "KK", v, M=v[0] + 2, N=1, K=70, epi="gelu", c_off=1, **sc))
    # automatic split (splitk = 0): one 64 x 64 tile over 48 k-tiles of 32 -> min(1024 tiles' worth, 48 / 12, 8) = 4 splits; the
    # library zeroes exactly the N columns of a NaN-filled C, the pad columns keep their NaN
    for v in (F16_TILE, (64, 64, 32, 1, 0), (64, 64, 32, 1, 1)):
        out.append(Case(f"KK-auto-split-p{v[4]}", "KK", v, M=64, N=64, K=1536, ldc=72, splitk=0, auto_splitk=4, c_nan=True, tile=0, bk=0))
    out.append(Case("KR-auto-split-bias", "KR", (64, 64, 32, 1, 3), M=64, N=64, K=1536, ldc=72, splitk=0, auto_splitk=4, c_nan=True, tile=0, epi="bias"))
    # slab split: NaN-filled slabs, vbg_slab_reduce with bias and ReLU
    for v in (F16_TILE, (64, 64, 32, 1, 0), (128, 128, 32, 1, 3)):
        out.append(Case(f"KK-slab2-p{v[4]}-{v[0]}", "KK", v, M=v[0] + 2, N=v[1] + 4, K=256, splitk=2, slab=True, epi="bias_relu"))
        out.append(Case(f"KK-slab3-p{v[4]}-{v[0]}", "KK", v, M=v[0] + 2, N=v[1] + 4, K=576, splitk=3, slab=True, epi="bias_relu"))
    # fused statistics: the tail rows of M = BM + 2 must not be counted; 64- and 128-row tiles
    for pair in ("KK", "CK"):
        for v in ((64, 64, 16, 1, 0), (64, 64, 32, 1, 0), (128, 64, 32, 1, 0), (128, 128, 32, 1, 0), (64, 64, 32, 1, 1), (128, 128, 32, 1, 1),
                  (64, 64, 32, 1, 3), (128, 128, 16, 1, 3), (128, 128, 32, 1, 3), F16_TILE):
            M, N = _mn(v, True)
            if pair == "KK":
                out.append(Case(f"KK-stats-{v[0]}x{v[1]}x{v[2]}-p{v[4]}", pair, v, M=M, N=N, K=70, stats=True, epi="bias"))
            else:
                out.append(Case(f"CK-stats-{v[0]}x{v[1]}x{v[2]}-p{v[4]}", pair, v, conv=(5, 7, 9, 32, N, 3, 1, 1), stats=True))
    # the fp32 form's 16-deep k-tiles under a 128-row tile cannot stage their tile and the statistics live on the staged path: the
    # dispatch hands such a product to the 64 x 64 tile of the same depth (it used to launch the instance asked for, which stored C
    # and left the statistics untouched)
    for tile in (128064, 128128):
        out.append(Case(f"KK-stats-fp32-{tile}x16-falls-to-64", "KK", (64, 64, 16, 1, 0), M=130, N=132, K=70, stats=True, form="fp32", tile=tile, bk=16))
    return out


def _segment_cases():
    out = []
    # four segments at shifts 2, 1, 0, 0 on a [3, 8, 12] map: 96 pixels per image, so a 64-row tile straddles images
    for v in (F16_TILE, (64, 64, 32, 1, 3), (128, 128, 32, 1, 3), (128, 128, 16, 1, 3), (64, 64, 32, 1, 0), (128, 128, 32, 1, 0), (64, 64, 16, 1, 0),
              (128, 64, 16, 1, 0), (64, 64, 32, 1, 1), (128, 128, 32, 1, 1)):
        out.append(Case(f"KK-seg32-{v[0]}x{v[1]}x{v[2]}-p{v[4]}", "KK", v, M=288, N=v[1] + 4, K=128, segs=((32, 2), (32, 1), (32, 0), (32, 0)),
                        seg_map=(3, 8, 12), epi="bias_relu"))
    # a 16-channel segment forces 16-deep k-tiles: the split, fp16-pair and amp forms then run as the fp32 form (64 x 64 x 16 under the
    # automatic tile; the tile asked for otherwise)
    for form in ("f16", "split", "amp", "fp32"):
        out.append(Case(f"KK-seg16-{form}", "KK", (64, 64, 16, 1, 0), M=288, N=68, K=112, segs=((32, 2), (16, 1), (32, 0), (32, 0)),
                        seg_map=(3, 8, 12), form=form, tile=0, bk=0))
    out.append(Case("KK-seg16-split-128128", "KK", (128, 128, 16, 1, 0), M=288, N=132, K=112, segs=((32, 2), (16, 1), (32, 0), (32, 0)),
                    seg_map=(3, 8, 12), form="split", tile=128128, bk=0))
    out.append(Case("KK-seg16-prologue", "KK", (64, 64, 16, 1, 0), M=288, N=68, K=112, segs=((32, 2), (16, 1), (32, 0), (32, 0)),
                    seg_map=(3, 8, 12), form="fp32", tile=64064, bk=16, a_relu_scale=1.5))
    # one unaligned segment: the scalar-load path walks the segments too
    out.append(Case("KK-seg32-scalar", "KK", SCALAR, M=288, N=65, K=128, segs=((32, 2), (32, 1), (32, 0), (32, 0)), seg_map=(3, 8, 12), a_off=1))
    return out


def _group_cases():
    # grouped problems (the attention products): a negative offA, a group with M = N = 0, groups of different K.  Grouped launches keep
    # the fp32 form outside amp (vbg/ops.py), 32 deep unless asked otherwise
    g = ((66, 65, 70), (0, 0, 32), (30, 68, 32), (64, 64, 200))
    out = [Case("KK-groups-fp32x32", "KK", (64, 64, 32, 1, 0), groups=g, form="split", tile=0, bk=0, epi="bias"),
           Case("KK-groups-fp32x16", "KK", (64, 64, 16, 1, 0), groups=g, form="split", tile=0, bk=16, alpha=-0.5),
           Case("KK-groups-amp", "KK", (64, 64, 32, 1, 1), groups=g, form="amp", tile=0, bk=0, epi="bias"),
           Case("KK-groups-acc", "KK", (64, 64, 32, 1, 0), groups=g, form="fp32", tile=0, bk=0, accumulate=True),
           Case("KR-groups-fp32x32", "KR", (64, 64, 32, 1, 0), groups=g, form="split", tile=0, bk=0),
           Case("KK-groups-scalar", "KK", SCALAR, groups=g, form="split", tile=0, bk=0, b_off=1, epi="bias")]
    return out


GEOS = ((3, 1, 1), (3, 2, 1), (1, 2, 0), (7, 2, 3))          # (k, stride, pad): 3x3/s1/p1, 3x3/s2/p1, 1x1/s2/p0, 7x7/s2/p3


def _conv_fwd_cases():
    out = []
    for v in INSTANCES["CK"]:
        tag = f"CK-{v[0]}x{v[1]}x{v[2]}-v{v[3]}p{v[4]}"
        Cout = v[1] + 4 if v[3] else v[1] + 1
        sc = {} if v[3] else {"b_off": 1}          # scalar path: the weights one float off
        # 16 and 48 channels force 16-deep k-tiles: only the fp32 form's 16-deep instances and the scalar path take them as asked
        chans = (16, 32, 48, 64) if (v[2] == 16 and v[4] == 0) else (32, 64)
        for (k, st, pd) in GEOS:
            for Cin in chans:
                # [5, 7, 9]: 63 pixels per image, a 128-row tile holds pieces of three images
                out.append(Case(f"{tag}-k{k}s{st}-c{Cin}", "CK", v, conv=(5, 7, 9, Cin, Cout, k, st, pd), epi="bias", **sc))
        out.append(Case(f"{tag}-k3s1-map268", "CK", v, conv=(2, 6, 8, chans[0], Cout, 3, 1, 1), epi="bias_relu", **sc))
        out.append(Case(f"{tag}-k1s2-map268", "CK", v, conv=(2, 6, 8, chans[-1], Cout, 1, 2, 0), **sc))
        # four splits of 64-channel taps: 18 k-tiles of 32 (5 5 5 3) or 36 of 16 (9 9 9 9), so splits start in the MIDDLE of a filter tap
        out.append(Case(f"{tag}-k3s1-split4", "CK", v, conv=(5, 7, 9, 64, Cout, 3, 1, 1), accumulate=True, splitk=4, epi="bias", **sc))
    # under amp / split / fp16-pair, 16 and 48 channels fall back to the fp32 form, 16 deep; the reference follows the reported prec
    for form in ("amp", "split", "f16"):
        for Cin in (16, 48):
            out.append(Case(f"CK-{form}-c{Cin}-falls-to-fp32", "CK", (64, 64, 16, 1, 0), conv=(5, 7, 9, Cin, 68, 3, 1, 1), form=form, tile=0, bk=0, epi="bias"))
        out.append(Case(f"CK-{form}-c48-128128-falls-to-fp32", "CK", (128, 128, 16, 1, 0), conv=(5, 7, 9, 48, 132, 3, 2, 1), form=form, tile=128128, bk=0))
    return out


def _conv_dgrad_cases():
    out = []
    for v in INSTANCES["CW"]:
        if ("CW", v) in UNREACHABLE:
            continue
        tag = f"CW-{v[0]}x{v[1]}x{v[2]}-v{v[3]}p{v[4]}"
        couts = (16, 32) if (v[2] == 16 and v[4] == 0) else (32,)
        cins = (20, 68) if v[1] == 64 else (20, 68, 132)          # N: % 4 and tile tails
        for (k, st, pd) in GEOS:
            for Cout in couts:
                for Cin in cins:
                    # x of odd size [3, 7, 9]; the 3x3/s2 cases accumulate into a non-zero dx
                    out.append(Case(f"{tag}-k{k}s{st}-ci{Cin}-co{Cout}", "CW", v, conv=(3, 7, 9, Cin, Cout, k, st, pd), accumulate=(k, st) == (3, 2)))
        # four splits of 64-filter taps: 18 k-tiles of 32 (5 5 5 3) or 36 of 16, so splits start in the MIDDLE of a filter tap
        out.append(Case(f"{tag}-k3s2-split4", "CW", v, conv=(3, 7, 9, 68, 64, 3, 2, 1), accumulate=True, splitk=4, alpha=-0.5))
    for form in ("amp", "split"):
        out.append(Case(f"CW-{form}-co16-falls-to-fp32", "CW", (64, 64, 16, 1, 0), conv=(3, 7, 9, 68, 16, 3, 2, 1), form=form, tile=0, bk=0))
    return out


def _conv_wgrad_cases():
    out = []
    for v in INSTANCES["RC"]:
        tag = f"RC-{v[0]}x{v[1]}x{v[2]}-v{v[3]}p{v[4]}"
        Cout = v[0] + 4 if v[3] else 6          # an M tail (68 on the 64-row tiles); the scalar path: Cout = 6, lda % 4 != 0
        Cin = 16 if (v[2] == 16 and v[4] == 0) else 32
        lda = {} if v[3] else {"lda": 6}
        # maps against the k-tile depth: Wr % BK == 0 (fast path one, Wr = 32), BK % Wr == 0 and Hr * Wr % BK == 0 (fast path two, 8 x 8),
        # neither (the general walk: 7 x 9 at stride 1, the 4 x 5 output of stride 2)
        for name, conv in (("wr32", (2, 3, 32, Cin, Cout, 3, 1, 1)), ("8x8", (2, 8, 8, Cin, Cout, 3, 1, 1)), ("7x9", (3, 7, 9, Cin, Cout, 3, 1, 1)),
                           ("4x5", (3, 7, 9, Cin, Cout, 3, 2, 1)), ("4x5-k1", (3, 7, 9, Cin, Cout, 1, 2, 0)), ("4x5-k7", (3, 7, 9, Cin, Cout, 7, 2, 3)),
                           ("wr32-s2", (2, 5, 64, Cin, Cout, 3, 2, 1))):
            out.append(Case(f"{tag}-{name}", "RC", v, conv=conv, **lda))
            # three splits: a split starts in the middle of an image (and of a pixel row)
            out.append(Case(f"{tag}-{name}-split3", "RC", v, conv=conv, accumulate=True, splitk=3, **lda))
        out.append(Case(f"{tag}-7x9-split6-alpha", "RC", v, conv=(3, 7, 9, Cin, Cout, 3, 1, 1), accumulate=True, splitk=6, alpha=-0.5, **lda))
    out.append(Case("RC-split-c16-falls-to-fp32", "RC", (64, 64, 16, 1, 0), conv=(3, 7, 9, 16, 68, 3, 1, 1), form="split", tile=64064, bk=0))
    return out


CASES = _dense_cases() + _segment_cases() + _group_cases() + _conv_fwd_cases() + _conv_dgrad_cases() + _conv_wgrad_cases()
assert len({c.name for c in CASES}) == len(CASES), "case names are the test ids: unique"
BY_PAIR = {p: [c for c in CASES if c.pair == p] for p in PAIRS}


# =====================================================================================================================================
# operands, call arguments and the fp64 reference of a case
# =====================================================================================================================================
def _gen(case):
    return torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(case.name)) % (2 ** 31))


def _store(vals, ld, off, guard=2):
    """a [rows, cols] matrix as the kernel finds it in memory: flat buffer, `off` floats in front, row stride ld, `guard` rows behind;
    everything that is not an element of the matrix is NaN.  Returns the flat buffer (the operand starts at element `off`)"""
    rows, cols = vals.shape
    assert ld >= cols
    buf = torch.full((off + (rows + guard) * ld,), float("nan"), dtype=f32)
    buf[off:off + rows * ld].view(rows, ld)[:, :cols] = vals
    return buf


class Problem:
    """one case, materialised: tensors on `device` (CPU for the host test: only their addresses' alignment is looked at), the
    arguments of ops.gemm_raw / ops.gemm_variant, and what the fp64 reference needs"""

    def __init__(self, case, device, ops):
        self.case, self.ops, self.device = case, ops, device
        c = case
        g = _gen(c)
        a_kind, b_kind = PAIRS[c.pair]
        M, N, K = c.dims
        self.M, self.N, self.K = M, N, K
        self.a_ptr_off, self.c_rows = c.a_off, M
        kw = {}
        if c.groups:
            self._init_groups(g, a_kind, b_kind, kw)
        elif c.conv is not None:
            self._init_conv(g, kw)
        else:
            A = torch.randn(M, K, generator=g)
            Bm = torch.randn(N, K, generator=g)              # C = A @ Bm^T
            self.A64, self.B64 = A.double(), Bm.double()
            if c.segs:
                self._init_segments(A, kw)
            else:
                a_st = A if a_kind == DENSE_K else A.t().contiguous()
                self.lda = up4(a_st.shape[1]) if c.lda is None else c.lda
                self.a_buf = _store(a_st, self.lda, c.a_off).to(device)
            b_st = Bm if b_kind == DENSE_K else Bm.t().contiguous()
            self.ldb = up4(b_st.shape[1]) if c.ldb is None else c.ldb
            self.b_buf = _store(b_st, self.ldb, c.b_off).to(device)
        self.ldc = c.ldc_eff
        # C: spare rows, spare columns, a sentinel (or NaN) everywhere; accumulate cases start from N(0, 1) inside [M, N]
        fill = float("nan") if c.c_nan else SENTINEL
        c_host = torch.full((c.c_off + (self.c_rows + SPARE_ROWS) * self.ldc + 4,), fill, dtype=f32)
        self.valid = self._valid_index()
        self.c0 = None
        if c.accumulate:
            self.c0 = torch.randn(self.valid.numel(), generator=g)
            c_host[self.valid] = self.c0
        self.c_host0 = c_host
        self.c_buf = c_host.to(device)
        self.c2_buf = c_host.clone().to(device) if c.epi == "gelu" else None
        self.bias = torch.randn(self._bias_len(), generator=g) if c.epi != "none" else None
        self.bias_dev = None if self.bias is None else self.bias.to(device)
        self.stats = torch.zeros(1, dtype=f64)
        if c.stats:
            self.stats = torch.zeros(ops.bn_slots() * 2 * N, dtype=f64, device=device)
            kw["stats"] = self.stats
        form, tile, bk = c.request
        self.form = form
        if c.slab:
            assert c.epi == "bias_relu" and not c.accumulate
            self.slabs = torch.full((c.splitk * M * N,), float("nan"), dtype=f32).to(device)
            kw.update(splitk=c.splitk, slab_stride=M * N)
            self.args = (M, N, K, self.a_buf, self.lda, a_kind, self.b_buf, self.ldb, b_kind, self.slabs, N)
        else:
            kw.update(splitk=c.splitk, accumulate=c.accumulate, alpha=c.alpha, c_ptr_off=c.c_off,
                      epi={"none": EPI_NONE, "bias": EPI_NONE, "bias_relu": EPI_RELU, "gelu": EPI_GELU_DUAL}[c.epi])
            if self.bias is not None:
                kw["bias"] = self.bias_dev
            if self.c2_buf is not None:
                kw["C2"] = self.c2_buf
            self.args = (M, N, K, self.a_buf, self.lda, a_kind, self.b_buf, self.ldb, b_kind, self.c_buf, self.ldc)
        kw.update(tile=tile, bk=bk, a_ptr_off=self.a_ptr_off, b_ptr_off=c.b_off, f16=(form == "f16"))
        if c.a_relu_scale is not None:
            kw["a_relu_scale"] = c.a_relu_scale
        self.kw = kw

    # ---- operand layouts ------------------------------------------------------------------------------------------------------
    def _init_segments(self, A, kw):
        """A [M, K] cut along K into segments, segment i stored at 1 / 2^shift resolution of the [B, H, W] map: the full-resolution values
        are the nearest-neighbour up-sampling of the stored ones, so A itself is REBUILT from what is stored"""
        c = self.case
        Bn, H, W = c.seg_map
        assert self.M == Bn * H * W
        segs, cols, k0 = [], [], 0
        self.seg_bufs = []
        for i, (ch, sh) in enumerate(c.segs):
            h, w = H >> sh, W >> sh
            small = A[:Bn * h * w, k0:k0 + ch].clone()                                   # [B*h*w, ch]: any values will do
            full = small.view(Bn, h, w, ch).repeat_interleave(1 << sh, 1).repeat_interleave(1 << sh, 2).reshape(self.M, ch)
            cols.append(full)
            ld = ch + 4
            off = c.a_off if i == 1 else 0                                               # (a_off: ONE unaligned segment)
            buf = _store(small, ld, off).to(self.device)
            self.seg_bufs.append(buf)
            k0 += ch
            segs.append((buf[off:], k0, ld, sh))
        assert k0 == self.K
        self.A64 = torch.cat(cols, 1).double()
        self.a_buf, self.lda = self.seg_bufs[0], c.segs[0][0] + 4
        kw.update(segs=segs, a_hw=(H, W))

    def _init_groups(self, g, a_kind, b_kind, kw):
        c = self.case
        self.lda = up4(max(k for _, _, k in c.groups)) + 4 if a_kind == DENSE_K else up4(max(m for m, _, _ in c.groups)) + 4
        self.ldb = up4(max(k for _, _, k in c.groups)) + 4 if b_kind == DENSE_K else up4(max(n for _, n, _ in c.groups)) + 4
        maxM, maxN, _ = c.dims
        a_parts, b_parts, self.g64, table = [], [], [], []
        a_pos, b_pos, c_pos, bias_pos = 8, 8, 0, 0
        self.grp_c = []
        ldc = c.ldc_eff
        for (m, n, k) in c.groups:
            A, Bm = torch.randn(m, k, generator=g), torch.randn(n, k, generator=g)
            self.g64.append((A.double(), Bm.double()))
            a_st = A if a_kind == DENSE_K else A.t().contiguous()
            b_st = Bm if b_kind == DENSE_K else Bm.t().contiguous()
            a_parts.append((a_pos, a_st)); b_parts.append((b_pos, b_st))
            table.append([m, n, k, a_pos, b_pos, c_pos, bias_pos, 0])
            self.grp_c.append((c_pos, bias_pos))
            a_pos += (a_st.shape[0] + 1) * self.lda
            b_pos += (b_st.shape[0] + 1) * self.ldb
            c_pos += (m + 1) * ldc
            bias_pos += n
        self.c_rows = c_pos // ldc
        self.bias_total = bias_pos

        def flat(parts, total, ld, off):
            buf = torch.full((off + total + 2 * ld,), float("nan"), dtype=f32)
            for pos, st in parts:
                buf[off + pos:off + pos + st.shape[0] * ld].view(st.shape[0], ld)[:, :st.shape[1]] = st
            return buf
        # the A pointer handed to the library is group 2's block, so groups 0 and 1 have NEGATIVE offA
        self.a_base = table[2][3]
        for row in table:
            row[3] -= self.a_base
        self.a_ptr_off += self.a_base
        self.a_buf = flat(a_parts, a_pos, self.lda, c.a_off).to(self.device)
        self.b_buf = flat(b_parts, b_pos, self.ldb, c.b_off).to(self.device)
        self.grp = torch.tensor(table, dtype=torch.int64).reshape(-1).to(self.device)
        kw.update(grp=self.grp, ngroups=len(c.groups), grp_max=(maxM, maxN))

    def _init_conv(self, g, kw):
        c = self.case
        B, H, W, Cin, Cout, k, st, pd = c.conv
        Ho, Wo = (H + 2 * pd - k) // st + 1, (W + 2 * pd - k) // st + 1
        Kred = self.K
        x = torch.randn(B, H, W, Cin, generator=g)
        w = torch.randn(Cout, k, k, Cin, generator=g) / math.sqrt(Kred)
        dy = torch.randn(B, Ho, Wo, Cout, generator=g)
        self.x, self.w, self.dy = x, w, dy
        ops = self.ops
        if c.pair == "CK":          # y[pixel, co] = sum over (tap, ci): A = x gathered, B = the filter rows [Cout][K], K-contiguous
            self.lda, self.ldb = Cin, Kred + 4
            self.a_buf = _store(x.reshape(-1, Cin), Cin, c.a_off).to(self.device)
            self.b_buf = _store(w.reshape(Cout, Kred), self.ldb, c.b_off).to(self.device)
            kw["geo"] = ops.conv_geo(H, W, Cin, Ho, Wo, k, k, st, pd, 0)
        elif c.pair == "CW":        # dx[pixel, ci] = sum over (tap, co): A = dy gathered, B = the filter read as [tap, co][ci]
            self.lda, self.ldb = Cout, Cin
            self.a_buf = _store(dy.reshape(-1, Cout), Cout, c.a_off).to(self.device)
            self.b_buf = _store(w.reshape(Cout * k * k, Cin), Cin, c.b_off).to(self.device)
            kw["geo"] = ops.conv_geo(Ho, Wo, Cout, H, W, k, k, st, pd, 1)
        else:                       # dw[co, (tap, ci)] = sum over pixels: A = dy [pixel][co] row-contiguous, B = x gathered
            self.lda = (Cout + 4 if Cout % 4 == 0 else Cout) if c.lda is None else c.lda
            self.ldb = Cin
            self.a_buf = _store(dy.reshape(-1, Cout), self.lda, c.a_off).to(self.device)
            self.b_buf = _store(x.reshape(-1, Cin), Cin, c.b_off).to(self.device)
            kw["geo"] = ops.conv_geo(H, W, Cin, Ho, Wo, k, k, st, pd, 0)

    # ---- output bookkeeping ----------------------------------------------------------------------------------------------------
    def _bias_len(self):
        return self.bias_total if self.case.groups else self.N

    def _valid_index(self):
        """flat indices into the C buffer of every element the launch owns, row-major over [M, N] (groups: one after the other)"""
        c = self.case
        if c.groups:
            idx = [c.c_off + cp + torch.arange(m)[:, None] * self.ldc + torch.arange(n)[None, :] for (m, n, _), (cp, _) in zip(c.groups, self.grp_c)]
            return torch.cat([i.reshape(-1) for i in idx])
        return (c.c_off + torch.arange(self.M)[:, None] * self.ldc + torch.arange(self.N)[None, :]).reshape(-1)

    # ---- the reference ---------------------------------------------------------------------------------------------------------
    def _operand(self, t, prec, prologue=False):
        t = t.float()
        if prologue and self.case.a_relu_scale is not None:
            t = torch.clamp(t, min=0) * self.case.a_relu_scale          # (fp32, as the kernel: max(a, 0) * a_scale)
        if prec == 1:
            t = t.bfloat16().float()          # amp: operands rounded to bf16 (nearest even), after the prologue
        return t.double()

    def reference(self, prec):
        """(ref, mag) over the valid elements, flat, fp64: the product of the operands as form `prec` sees them, with alpha, bias and
        the accumulate start, BEFORE ReLU / GELU; mag = |alpha| (|a| @ |b|) + |bias| + |c0|, the unit of the error"""
        c = self.case
        if c.groups:
            refs, mags = [], []
            for (A, Bm), (_, bp), (m, n, _) in zip(self.g64, self.grp_c, c.groups):
                a, b = self._operand(A, prec, True), self._operand(Bm, prec)
                r, mg = c.alpha * (a @ b.t()), abs(c.alpha) * (a.abs() @ b.abs().t())
                if self.bias is not None:
                    bb = self.bias[bp:bp + n].double()
                    r, mg = r + bb, mg + bb.abs()
                refs.append(r.reshape(-1)); mags.append(mg.reshape(-1))
            ref, mag = torch.cat(refs), torch.cat(mags)
        else:
            if c.conv is not None:
                prod, pmag = self._conv_reference(prec)
            else:
                a, b = self._operand(self.A64, prec, True), self._operand(self.B64, prec)
                prod, pmag = a @ b.t(), a.abs() @ b.abs().t()
            ref, mag = c.alpha * prod, abs(c.alpha) * pmag
            if self.bias is not None:
                ref, mag = ref + self.bias.double(), mag + self.bias.double().abs()
            ref, mag = ref.reshape(-1), mag.reshape(-1)
        if self.c0 is not None:
            ref, mag = ref + self.c0.double(), mag + self.c0.double().abs()
        return ref, mag

    def _conv_reference(self, prec):
        c = self.case
        B, H, W, Cin, Cout, k, st, pd = c.conv
        x, w, dy = self._operand(self.x, prec), self._operand(self.w, prec), self._operand(self.dy, prec)
        outs = []
        for ab in (False, True):          # the product, then the same reduction over absolute values
            xn = (x.abs() if ab else x).permute(0, 3, 1, 2).clone().requires_grad_(True)
            wn = (w.abs() if ab else w).permute(0, 3, 1, 2).clone().requires_grad_(True)
            y = F.conv2d(xn, wn, stride=st, padding=pd)
            if c.pair == "CK":
                outs.append(y.detach().permute(0, 2, 3, 1).reshape(-1, Cout))
                continue
            y.backward((dy.abs() if ab else dy).permute(0, 3, 1, 2))
            if c.pair == "CW":
                outs.append(xn.grad.permute(0, 2, 3, 1).reshape(-1, Cin))
            else:
                outs.append(wn.grad.permute(0, 2, 3, 1).reshape(Cout, -1))
        return outs[0], outs[1]

    def dgrad_unread(self):
        """flat positions (within the valid elements) of the dx pixels no output pixel reads (1x1 / stride 2): exact zeros"""
        B, H, W, Cin, Cout, k, st, pd = self.case.conv
        m = torch.ones(H, W, dtype=torch.bool)
        m[::st, ::st] = False
        return m[None, :, :, None].expand(B, H, W, Cin).reshape(-1)


class form_state:
    """the library state a case runs under: the arithmetic form it asks for, every other switch that reaches the descriptor pinned
    (no forced tile, deterministic mode off, the fp16-pair switch on), no autograd (gemm_raw turns splitk = 1 into the automatic
    split when a backward may follow).  Restores what it found."""

    def __init__(self, ops, form):
        self.ops, self.form = ops, form

    def __enter__(self):
        o = self.ops
        self.saved = (o.precision(), o._AMP[0], o._GEMM_F16[0], list(o._FORCE), o._DET[0])
        o.set_precision("fp32" if self.form == "fp32" else "split")
        o._AMP[0] = self.form == "amp"
        o._GEMM_F16[0] = True
        o._FORCE[0] = o._FORCE[1] = 0
        o._DET[0] = False
        self.ng = torch.no_grad()
        self.ng.__enter__()
        return self

    def __exit__(self, *exc):
        o = self.ops
        self.ng.__exit__(*exc)
        o.set_precision(self.saved[0])
        o._AMP[0], o._GEMM_F16[0] = self.saved[1], self.saved[2]
        o._FORCE[0], o._FORCE[1] = self.saved[3]
        o._DET[0] = self.saved[4]
