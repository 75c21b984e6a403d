"""Per-parameter gradient and weight statistics in one launch per flat buffer.

    ps = vbg.stats.ParamStats(model, what=("grad", "param"), scaler=None)
    ...
    loss.backward()                # (and reducer.finish() under data parallel)
    ps.update()                    # before optimizer.step() / zero_grad(); enqueues only, no host sync
    ...
    snap = ps.read()               # ONE device-to-host copy for everything; numpy from here on
    snap["grad"].offenders()       # names of the parameters whose gradient holds an inf or a NaN
    ps.log(logger, "grad", depth=4, step=it, snap=snap)

What `for p in model.parameters(): p.grad.norm(); p.grad.isfinite().all()` finds out with a few hundred tiny launches and a host read
per quantity comes from one streaming pass over each flat buffer (`vbg_param_stats_rows`, csrc/stats.hip) and one small finish per
buffer (`vbg_param_stats_finish`): per parameter the sum of squares (double, finite elements only), the largest magnitude, the counts
of non-finite elements, of zeros, of elements an fp16 piece turns into inf (|v| >= 65520), and a histogram over 64 binades from which
the fp16 subnormal share (|v| < 2^-14) and the share that rounds to zero in fp16 (|v| < 2^-25) follow exactly.  Besides the tables of
the last update() a running table adds the counts and bins of every update() since reset().
"""
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

from . import ops
from .optim import SEG_CHUNK, FlatGroup

HIST_BINS = 64
HIST_E0 = -46                    # bin k in 1..62 holds 2^(k + HIST_E0) <= |v| < 2^(k + HIST_E0 + 1)
SUB_F16_BINS = 32                # |v| < 2^-14: bins 0 .. 31
LOST_F16_BINS = 21               # |v| < 2^-25: bins 0 .. 20
F16_OVER = 65520.0

# include/vbg.h vbg_stats_rec / vbg_stats_total as numpy records
REC_DTYPE = np.dtype([("sumsq", "<f8"), ("amax_bits", "<u4"), ("nonfinite", "<i4"), ("zeros", "<i4"), ("over_f16", "<i4"),
                      ("hist", "<i4", (HIST_BINS,)), ("pad", "<i4", (2,))])
TOTAL_DTYPE = np.dtype([("sumsq", "<f8"), ("nonfinite", "<i8"), ("zeros", "<i8"), ("over_f16", "<i8"), ("updates", "<i8"),
                        ("steps_nonfinite", "<i8"), ("amax_bits", "<u4"), ("pad", "<i4"), ("hist", "<i8", (HIST_BINS,))])
assert REC_DTYPE.itemsize == ops.STATS_REC_BYTES and TOTAL_DTYPE.itemsize == ops.STATS_TOTAL_BYTES


def stats_rows(offsets: Sequence[int], numels: Sequence[int], chunk: int):
    """-> (rows [n, 3] int64: start, length, parameter index; row_ptr int64[nparams + 1]).  Parameter i occupies elements
    [offsets[i], offsets[i] + numels[i]) and is cut into rows of at most `chunk` elements, the last one as short as it has to be: a
    row never reaches into the slot padding behind the parameter, and neighbours are never merged (vbg.optim.run_table does both, which
    is right for an optimizer step and wrong for a count)."""
    if chunk < 4 or chunk % 4:
        raise ValueError("chunk length: a positive multiple of 4 elements")
    off, num = np.asarray(offsets, dtype=np.int64).reshape(-1), np.asarray(numels, dtype=np.int64).reshape(-1)
    if len(off) != len(num) or (num < 1).any() or (num >= 1 << 31).any() or (off % 4).any():
        raise ValueError("statistics rows: one offset (a multiple of 4) and one element count in [1, 2^31) per parameter")
    per = (num + chunk - 1) // chunk
    which = np.repeat(np.arange(len(off)), per)
    row_ptr = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
    k = np.arange(len(which)) - row_ptr[which]
    start = off[which] + k * chunk
    length = np.minimum(chunk, off[which] + num[which] - start)
    return np.stack([start, length, which], axis=1).reshape(-1, 3), row_ptr


class Snapshot:
    """One quantity's per-parameter tables on the host (numpy).  Arrays, one entry per parameter, in the order of `names`:
    numel, sumsq, norm (sqrt of sumsq, float64), amax (float32), nonfinite, zeros, over_f16, sub_f16 (|v| < 2^-14, non-zero), lost_f16
    (|v| < 2^-25, non-zero), hist [n, 64] -- all of the last update(); and from the running table since reset(): updates,
    steps_nonfinite (updates in which the parameter held an inf or a NaN), hist_total [n, 64], amax_total.  The sum of squares, the
    maximum and the bins cover the FINITE elements only.  On a snapshot that grouped() / by_module() aggregated, `updates` and
    `steps_nonfinite` are the largest of the members' values: the row was non-finite in AT LEAST that many updates."""

    def __init__(self, names, numel, sumsq, amax_bits, nonfinite, zeros, over_f16, hist, updates, steps_nonfinite, hist_total, amax_total_bits):
        self.names = list(names)
        self.numel = np.asarray(numel, dtype=np.int64)
        self.sumsq = np.asarray(sumsq, dtype=np.float64)
        self.amax_bits = np.asarray(amax_bits, dtype=np.uint32)
        self.nonfinite = np.asarray(nonfinite, dtype=np.int64)
        self.zeros = np.asarray(zeros, dtype=np.int64)
        self.over_f16 = np.asarray(over_f16, dtype=np.int64)
        self.hist = np.asarray(hist, dtype=np.int64).reshape(len(self.names), HIST_BINS)
        self.updates = np.asarray(updates, dtype=np.int64)
        self.steps_nonfinite = np.asarray(steps_nonfinite, dtype=np.int64)
        self.hist_total = np.asarray(hist_total, dtype=np.int64).reshape(len(self.names), HIST_BINS)
        self.amax_total_bits = np.asarray(amax_total_bits, dtype=np.uint32)

    @classmethod
    def from_records(cls, names, numel, last, total=None):
        """from vbg_stats_rec records (REC_DTYPE) and, when there is a running table, vbg_stats_total records (TOTAL_DTYPE)"""
        n = len(names)
        if total is None:
            total = np.zeros((n,), dtype=TOTAL_DTYPE)
        return cls(names, numel, last["sumsq"], last["amax_bits"], last["nonfinite"], last["zeros"], last["over_f16"], last["hist"],
                   total["updates"], total["steps_nonfinite"], total["hist"], total["amax_bits"])

    norm = property(lambda self: np.sqrt(self.sumsq))
    amax = property(lambda self: self.amax_bits.copy().view(np.float32))
    amax_total = property(lambda self: self.amax_total_bits.copy().view(np.float32))
    sub_f16 = property(lambda self: self.hist[:, :SUB_F16_BINS].sum(axis=1))
    lost_f16 = property(lambda self: self.hist[:, :LOST_F16_BINS].sum(axis=1))

    def __len__(self):
        return len(self.names)

    def total_norm(self) -> float:
        """the L2 norm over all parameters (finite elements)"""
        return float(np.sqrt(self.sumsq.sum()))

    def offenders(self) -> List[str]:
        """names of the parameters with an inf or a NaN in the last update, worst (most non-finite elements) first"""
        idx = [i for i in np.argsort(-self.nonfinite, kind="stable") if self.nonfinite[i] > 0]
        return [self.names[i] for i in idx]

    def grouped(self, fn: Callable[[str], str]) -> "Snapshot":
        """rows aggregated by key = fn(name), keys in order of first appearance: numel, the sum of squares, counts and bins add, amax
        takes the max.  Of the running table `updates` and `steps_nonfinite` take the max over the members: the number of updates in
        which SOME member was non-finite is not something the members' counts determine, so a group's `steps_nonfinite` reads "at
        least"; adding the members' values would count an update twice whenever two members overflowed together"""
        keys, index = [], {}
        for name in self.names:
            k = fn(name)
            if k not in index:
                index[k] = len(keys)
                keys.append(k)
        which = np.array([index[fn(name)] for name in self.names], dtype=np.int64)
        n = len(keys)

        def add(a):
            out = np.zeros((n,) + a.shape[1:], dtype=a.dtype)
            np.add.at(out, which, a)
            return out

        def top(a):
            out = np.zeros((n,), dtype=a.dtype)
            np.maximum.at(out, which, a)
            return out

        return Snapshot(keys, add(self.numel), add(self.sumsq), top(self.amax_bits), add(self.nonfinite), add(self.zeros), add(self.over_f16),
                        add(self.hist), top(self.updates), top(self.steps_nonfinite), add(self.hist_total), top(self.amax_total_bits))

    def by_module(self, depth: int) -> "Snapshot":
        """grouped() by the first `depth` components of the dotted name: 13 encoder rows instead of 200.  `steps_nonfinite` of a row
        is a lower bound (at least that many updates saw an inf or a NaN in the module), not a count: see grouped()"""
        if int(depth) < 1:
            raise ValueError("by_module: depth >= 1")
        return self.grouped(lambda name: ".".join(name.split(".")[:int(depth)]))

    def fp16_range(self) -> Dict[str, np.ndarray]:
        """per parameter, as shares of its elements: "over" (finite, |v| >= 65520: inf as an fp16 piece), "sub" (non-zero, |v| < 2^-14:
        fp16 subnormal, precision falls off) and "lost" (non-zero, |v| < 2^-25: rounds to zero in fp16) -- the range contract of the
        fp16-pair forms made visible; {"names": [...], "over": ..., "sub": ..., "lost": ...}"""
        n = np.maximum(self.numel, 1).astype(np.float64)
        return {"names": list(self.names), "over": self.over_f16 / n, "sub": self.sub_f16 / n, "lost": self.lost_f16 / n}


class _Bound:
    """what one FlatGroup needs for its passes"""

    def __init__(self, group, table, ext, recs, last, total):
        self.group, self.table, self.ext, self.recs, self.last, self.total = group, table, ext, recs, last, total


class ParamStats:
    """Per-parameter statistics of a model's gradients and / or weights over its flat storage (see the module docstring).

    what: any of "grad", "param".  scaler: a torch.amp.GradScaler whose device scale the "grad" pass divides by -- pass it exactly
    when the gradients still hold scaled values at update() (no `scaler.unscale_` before it), the rule vbg.optim.clip_in_step states;
    weights are never scaled.  seg_chunk: elements per row of the tables (default vbg.optim.SEG_CHUNK).

    Binding happens at the first update(): the groups are those the model's trainable parameters live in (the model homes them at its
    first training forward).  A trainable parameter with a gradient but no flat home (VBG_HOME=0) raises ValueError; a model with no
    homed parameter raises ValueError; a group whose parameters moved away since (Module.to, a fresh `.data`) raises RuntimeError at
    the next update().  Tables, names and output buffers are built once per binding.

    update() is one row pass per (flat buffer, quantity) and one finish per flat buffer, on the current stream, with no host sync.  The
    gradient pass reads the flat gradient buffer itself: a parameter whose `.grad` is None in a step is reported from the zeros its flat
    view holds (all zeros, norm 0).  read() is one device-to-host copy of every table of every group into pinned memory and returns
    {"grad": Snapshot, "param": Snapshot}; reset() zeroes the running tables.  Data parallel: after the all-reduce every rank sees the
    same gradients, so every rank's tables agree and no collective is added."""

    QUANTITIES = ("grad", "param")

    def __init__(self, model: torch.nn.Module, what: Sequence[str] = ("grad", "param"), scaler=None, seg_chunk: Optional[int] = None):
        what = (what,) if isinstance(what, str) else tuple(what)
        if not what or any(w not in self.QUANTITIES for w in what) or len(set(what)) != len(what):
            raise ValueError(f"what={what!r}: one or both of 'grad', 'param'")
        self.model, self.what, self.scaler = model, what, scaler
        self.seg_chunk = int(seg_chunk or SEG_CHUNK)
        if self.seg_chunk < 4 or self.seg_chunk % 4:
            raise ValueError("seg_chunk: a positive multiple of 4 elements")
        self.groups: List[FlatGroup] = None
        self.names: List[str] = None
        self.numel = None
        self._bound: List[_Bound] = None
        self._out = self._host = None
        self._slices = None
        self.copies = 0                  # device-to-host copies read() has made

    # ---- binding --------------------------------------------------------------------------------------------------------------
    def _bind(self):
        if self.groups is not None:
            return
        groups = []
        for name, p in self.model.named_parameters():
            if not p.requires_grad:
                continue
            g = getattr(p, "_vbg_flat", (None,))[0]
            if g is None:
                if p.grad is not None:
                    raise ValueError(f"ParamStats: parameter {name} is trained but does not live in flat storage (VBG_HOME=0, or no training "
                                     "forward on the device yet); there is no per-parameter route here")
                continue
            if all(g is not h for h in groups):
                groups.append(g)
        if not groups:
            raise ValueError("ParamStats: no parameter of the model lives in flat storage yet (the model homes its parameters at its first "
                             "training forward on the device)")
        self.groups = groups
        self._check_valid()
        model_name = {id(p): n for n, p in self.model.named_parameters()}
        nq = len(self.what)
        self.names, numel, at, plan = [], [], 0, []
        for g in groups:
            sizes = [p.numel() for p in g.params]
            rows, row_ptr = stats_rows(g.offsets, sizes, self.seg_chunk)
            self.names += [model_name.get(id(p), n) for p, n in zip(g.params, g.names)]
            numel += sizes
            npar = len(sizes)
            last_at = at
            at += (nq * npar * ops.STATS_REC_BYTES + 15) // 16 * 16
            total_at = at
            at += (nq * npar * ops.STATS_TOTAL_BYTES + 15) // 16 * 16
            plan.append((g, rows, row_ptr, npar, last_at, total_at))
        self.numel = np.asarray(numel, dtype=np.int64)
        dev = groups[0].pflat.device
        self._out = torch.zeros((at,), dtype=torch.uint8, device=dev)
        self._bound, self._slices = [], []
        for g, rows, row_ptr, npar, last_at, total_at in plan:
            d = g.pflat.device
            if d != dev:
                raise ValueError("ParamStats: the model's flat buffers live on different devices")
            table = ops.stats_table(rows, row_ptr, g.total, d)
            # the finish sees the quantities side by side: quantity q's rows and parameters follow quantity q - 1's
            ext_ptr = np.concatenate([row_ptr[:1]] + [row_ptr[1:] + q * len(rows) for q in range(nq)])
            ext = ops.StatsTable(table.rows, torch.from_numpy(ext_ptr.astype(np.int32)).to(d), nq * len(rows), nq * npar, g.total)
            recs = torch.empty((max(1, nq * len(rows)) * ops.STATS_REC_BYTES,), dtype=torch.uint8, device=d)
            last = self._out[last_at:last_at + nq * npar * ops.STATS_REC_BYTES]
            total = self._out[total_at:total_at + nq * npar * ops.STATS_TOTAL_BYTES]
            self._bound.append(_Bound(g, table, ext, recs, last, total))
            self._slices.append((npar, last_at, total_at))

    def _check_valid(self):
        for g in self.groups:
            if not g.valid():
                raise RuntimeError("ParamStats: the parameters moved away from the flat buffer these statistics are bound to (Module.to / a "
                                   "fresh .data); build a new ParamStats after moving the model")

    def _scale(self):
        s = self.scaler
        if s is None or not s.is_enabled():
            return None
        if s._scale is None:
            raise RuntimeError("ParamStats: the GradScaler has not scaled a loss yet, so the gradients cannot hold scaled values")
        return s._scale

    # ---- the passes -------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def update(self):
        self._bind()
        self._check_valid()
        scale = self._scale() if "grad" in self.what else None
        for b in self._bound:
            per = b.table.n * ops.STATS_REC_BYTES
            for q, w in enumerate(self.what):
                x = b.group.gflat if w == "grad" else b.group.pflat
                ops.param_stats_rows(x, b.table, b.recs[q * per:(q + 1) * per], scale if w == "grad" else None)
            ops.param_stats_finish(b.recs, b.ext, b.last, b.total)

    def reset(self):
        """zero the running tables (and the tables of the last update); one memset, no host sync"""
        if self._out is not None:
            self._out.zero_()

    def read(self) -> Dict[str, Snapshot]:
        """{quantity: Snapshot} of everything update() has left on the device: ONE device-to-host copy into pinned memory, then numpy"""
        if self._out is None:
            raise RuntimeError("ParamStats.read(): nothing has been measured yet (no update())")
        if self._host is None:
            self._host = torch.empty((self._out.numel(),), dtype=torch.uint8, pin_memory=True)
        self._host.copy_(self._out, non_blocking=True)
        self.copies += 1
        done = torch.cuda.Event()
        done.record()
        done.synchronize()
        raw = self._host.numpy().copy()
        nq = len(self.what)
        last = {w: [] for w in self.what}
        total = {w: [] for w in self.what}
        for npar, last_at, total_at in self._slices:
            l = raw[last_at:last_at + nq * npar * ops.STATS_REC_BYTES].view(REC_DTYPE)
            t = raw[total_at:total_at + nq * npar * ops.STATS_TOTAL_BYTES].view(TOTAL_DTYPE)
            for q, w in enumerate(self.what):
                last[w].append(l[q * npar:(q + 1) * npar])
                total[w].append(t[q * npar:(q + 1) * npar])
        return {w: Snapshot.from_records(self.names, self.numel, np.concatenate(last[w]), np.concatenate(total[w])) for w in self.what}

    def log(self, logger, what: str = "grad", depth: Optional[int] = None, step: Optional[int] = None, snap: Optional[Dict[str, Snapshot]] = None):
        """per-parameter (depth=None) or per-module (by_module(depth)) rows through `logger.update(head=..., step=step, **{name: float})`
        -- the signature of the reference's TensorboardLogger.update: heads "<what>_norm", "<what>_amax" and "<what>_nonfinite".
        A row named like one of the logger's own keywords ("head", "step") is logged with a trailing underscore.
        snap: what read() returned (None: read() now, one copy)"""
        if what not in self.what:
            raise ValueError(f"log: what={what!r} is not measured (what={self.what!r})")
        s = (snap if snap is not None else self.read())[what]
        if depth is not None:
            s = s.by_module(depth)
        # (a row called "head" or "step" -- by_module(1) of a model with such a child -- would collide with the logger's own keywords)
        keys = [n + "_" if n in ("head", "step", "self") else n for n in s.names]
        logger.update(head=f"{what}_norm", step=step, **{n: float(v) for n, v in zip(keys, s.norm)})
        logger.update(head=f"{what}_amax", step=step, **{n: float(v) for n, v in zip(keys, s.amax)})
        logger.update(head=f"{what}_nonfinite", step=step, **{n: float(v) for n, v in zip(keys, s.nonfinite)})
        return s
