"""Flat parameter / gradient storage, fused optimizers and the data-parallel gradient reducer.

Mirrors what the reference wires up in train_SROIE.py:206-235 (DDP(find_unused_parameters=True), SGD for the
CNN/head parameters, AdamW for every parameter whose name contains "bert_model") and steps at
pipeline/train_val_utils.py:272-284, designed for MI355X instead of translated:

* every trainable parameter of a group lives in ONE flat fp32 buffer (so do its gradient and optimizer
  state); `param.data` / `param.grad` are views, conv weights keep their channels_last (OHWI) memory;
* `zero_grad` is one memset, each optimizer step is ONE HIP launch over the flat range
  (libvbg `vbg_sgd_step` / `vbg_adamw_step`, 20 / 28 B per parameter); with several torch param groups (no weight decay on biases
  and LayerNorm weights, layer-wise learning rates) it is still ONE launch: `vbg_sgd_step_seg` / `vbg_adamw_step_seg` walk a chunk
  table over the same buffers and take every group's hyper-parameters by value; `fuse(optimizer)` gives the same single launch to an
  unchanged torch.optim.SGD / Adam / AdamW object, with torch's semantics kept whole (`vbg_sgd_step_seg_opt` / `vbg_adam_step_seg_opt`);
* an EMA / SWA of the parameters is one more flat buffer per group: `WeightAverage.update()` is one `vbg_lerp` launch per buffer,
  validation on the averaged weights an in-place exchange (`vbg_swap`) plus one cache invalidation -- no second model;
* data parallel: the flat gradient buffer is cut into large contiguous buckets; a bucket is all-reduced
  (RCCL over xGMI, async, its own stream) as soon as autograd has accumulated its last gradient, so the
  exchange overlaps the rest of backward; no bucket copies (gradients ARE the bucket); the 1/world
  averaging is folded into the optimizer kernels.  The flat buffers hold the parameters in REVERSE forward order (heads first,
  stem / word embeddings last), so contiguous buckets complete roughly in the order autograd produces them; buckets are launched
  strictly in ONE sequence that is identical on every rank (the completion order rank 0 observed in its first step, broadcast
  once), so data-dependent graphs (classifier_mode full / crf: a per-class net may get no gradient on one rank) can never make two
  ranks issue collectives in different orders.  SyncBatchNorm statistics share the reducer's communicator by default (one
  communicator, one rank-invariant program order: the boring configuration for graphs that are the same on every rank); an own
  communicator for them, concurrent with the buckets, is the opt-in (`sync_bn_group="new"`, FlatReducer.__init__).  Parameters that never receive a gradient
  (`bert_model.pooler.*`, `backbone.resnet.fc.*`) are kept out of the buffers, which is what
  `find_unused_parameters=True` + "skip params with grad None" amounts to in the reference.
"""
import contextlib
import os
import time
from typing import Dict, List, Sequence, Tuple

import torch
import torch.distributed as dist

from . import functions as Fn
from . import ops

STATIC_UNUSED = ("pooler.", "resnet.fc.")


def _phys_view(flat: torch.Tensor, off: int, p: torch.Tensor) -> torch.Tensor:
    """view of flat[off:off+numel] with p's logical shape and p's memory layout (channels_last kept)"""
    n = p.numel()
    chunk = flat[off:off + n]
    if p.dim() == 4 and p.is_contiguous(memory_format=torch.channels_last) and not p.is_contiguous():
        O, I, H, W = p.shape
        return chunk.view(O, H, W, I).permute(0, 3, 1, 2)
    return chunk.view(p.shape)


def _fusion_order(named):
    """Same parameters in the order of the flat buffers:
    * each attention block's query/key/value weights (and then their biases) sit back to back, so the three projections run as
      ONE [3*hidden, hidden] GEMM forward and backward (vbg/functions.BertLayerFn);
    * the units (such a block, or a single parameter) are laid out in REVERSE registration (= forward) order, so the
      contiguous gradient buckets of FlatReducer fill up in roughly the order backward produces them: heads, FPN, trunk
      top-down, stem last; encoder layer 11 ... 0, the embedding tables last.
    The optimizers are element-wise, so the order is otherwise irrelevant."""
    by_name = dict(named)
    units, used = [], set()
    for name, p in named:
        if name in used:
            continue
        if name.endswith("attention.self.query.weight"):
            stem = name[:-len("query.weight")]
            block = [stem + k for k in ("query.weight", "key.weight", "value.weight", "query.bias", "key.bias", "value.bias")]
            if all(b in by_name for b in block):
                units.append([(b, by_name[b]) for b in block])
                used.update(block)
                continue
        units.append([(name, p)])
        used.add(name)
    return [np_ for u in reversed(units) for np_ in u]


class FlatGroup:
    def __init__(self, named: List[Tuple[str, torch.nn.Parameter]], device):
        self.ref_names = [n for n, _ in named]            # the caller's (= reference's) parameter order, for state_dict indices
        named = _fusion_order(named)
        self.names = [n for n, _ in named]
        self.params = [p for _, p in named]
        sizes = [p.numel() for p in self.params]
        # 32-byte aligned slots: float4 kernels / vector GEMM loads stay legal on every view, and the same offsets address the
        # bf16 plane image of the buffer 16-byte aligned (LDS-DMA rows)
        self.offsets, o = [], 0
        for s in sizes:
            self.offsets.append(o)
            o += (s + 7) // 8 * 8
        self.total = (o + 31) // 32 * 32
        self.pflat = torch.zeros((self.total,), device=device, dtype=torch.float32)
        self.gflat = torch.zeros((self.total,), device=device, dtype=torch.float32)
        self.gviews = []                     # the persistent gradient views (re-attached when something set .grad to None)
        self._ptrs = []                      # device address every parameter must still have for the group to be its home
        for p, off in zip(self.params, self.offsets):
            v = _phys_view(self.pflat, off, p.data)
            v.copy_(p.data)
            p.data = v
            gv = _phys_view(self.gflat, off, p.data)
            p.grad = gv
            p._vbg_sunk = True               # weight-gradient GEMMs accumulate straight into this view
            p._vbg_flat = (self, off)
            self.gviews.append(gv)
            self._ptrs.append(self.pflat.data_ptr() + 4 * off)
        self._index = {id(p): i for i, p in enumerate(self.params)}
        # bf16 planes of the whole buffer (csrc/gemm_planes.hip operands), refreshed at most once per parameter version: the plain
        # image [3][total] in ONE elementwise launch, the transposed images of the matrices that asked for one in ONE batched launch
        self._planes = None
        self._planes_tag = None
        self._plain_keys, self._plain_tags = set(), {}
        self._pair = None                    # fp16-pair image [2][total] (operands of the form-1 forward products)
        self._pair_tag = None
        # transposed images: bf16 planes (`_tp`) and fp16-pair planes (`_tq`); jobs: (offset, rows, cols) -> (slot offset, ld)
        self._tp = {"jobs": {}, "buf": None, "tbl": None, "tag": None, "tiles": 0}
        self._tq = {"jobs": {}, "buf": None, "tbl": None, "tag": None, "tiles": 0}
        self._ver = {}
        self._owners = {}
        self._armed = []                     # indices whose gradient view arm() attached in the current backward

    def zero_grad(self):
        self.gflat.zero_()
        for p, gv in zip(self.params, self.gviews):          # re-attach if something set grads to None
            if p.grad is not gv:
                p.grad = gv

    def valid(self) -> bool:
        """every parameter still lives where the group put it (Module.to / .half / a fresh `p.data = ...` moves it away)"""
        return all(p.data_ptr() == a for p, a in zip(self.params, self._ptrs))

    def arm(self):
        """start of a backward pass (vbg.functions.StepRootFn): the reference's loop calls `optimizer.zero_grad()` between forward and
        backward (pipeline/train_val_utils.py:272-273) and torch.optim's default is set_to_none -- every `.grad` is None then.  The
        gradient views come back, over ONE memset of the flat buffer when all of them were dropped (the usual case), slice by slice
        otherwise (a caller that keeps some gradients to accumulate into).  A gradient the caller left in place is accumulated into,
        as torch would."""
        # (a parameter frozen after it was homed keeps `.grad = None`: torch.optim skips it, as it would without flat storage)
        missing, foreign = [], []
        for i, (p, gv) in enumerate(zip(self.params, self.gviews)):
            g = p.grad
            if g is None:
                if p.requires_grad:
                    missing.append(i)
            elif g is not gv:
                foreign.append(i)
        self._armed = missing                # (ModelHome.drop_untouched only hands None back for gradients attached HERE, in this backward)
        if len(missing) == len(self.params):
            self.gflat.zero_()
        else:
            # one memset per contiguous RUN of missing parameters (one frozen parameter used to turn the single memset into
            # ~400 per-parameter launches)
            k = 0
            while k < len(missing):
                j = k
                while j + 1 < len(missing) and missing[j + 1] == missing[j] + 1:
                    j += 1
                i0, i1 = missing[k], missing[j]
                end = self.offsets[i1 + 1] if i1 + 1 < len(self.params) else self.total
                self.gflat[self.offsets[i0]:end].zero_()
                k = j + 1
        for i in missing:
            self.params[i].grad = self.gviews[i]
        # a `.grad` that is somebody else's tensor (DistributedDataParallel's finalize_backward leaves one on a locally-unused parameter):
        # its contents move into the flat view -- the weight-gradient kernels accumulate into the VIEW's memory (wgrad_dest), and
        # torch.optim must see what they wrote
        for i in foreign:
            g = self.params[i].grad
            gv = self.gviews[i]
            if g.shape == gv.shape and g.device == gv.device:
                with torch.no_grad():
                    gv.copy_(g)
                self.params[i].grad = gv

    def attach(self, p):
        """gradient view of one parameter whose `.grad` is None outside an armed backward (a Function used on its own): zeroed, attached"""
        gv = self.gviews[self._index[id(p)]]
        gv.zero_()
        p.grad = gv
        return gv

    def invalidate(self):
        """forget every cached plane image of the buffer.  The caches follow the optimizer kernels (weight epoch), torch in-place
        updates (`_version` of the buffer and of the parameter asked for) and load_state_dict; a write through `param.data`
        (`p.data.copy_(...)`, `p.data.mul_(...)`: EMA / weight-tying code) moves none of these counters -- call this, or
        vbg.ops.bump_weight_epoch(), after such a write"""
        self._planes_tag = self._pair_tag = self._tp["tag"] = self._tq["tag"] = None
        self._plain_tags.clear()
        self._ver.clear()

    def _tag(self):
        return (ops._W_EPOCH[0], self.pflat._version)

    def _stale(self, which: str, off: int, owners) -> bool:
        """refresh of the whole-buffer image `which` needed for the matrix at `off`?  The optimizer kernels of this library bump the epoch
        (`_tag`); torch's own in-place updates (torch.optim on the flat views, load_state_dict, tests) only move the version counters of
        the parameters they touch.  `owners`: the parameter(s) the matrix consists of.  The image is split from the WHOLE buffer, so at a
        refresh the versions of every matrix registered for it are noted -- a matrix asked for later in the same step is then known to be
        current, and one whose counter has moved since (the next step) is known to be stale.  (Round 5: until then a matrix that had not
        been asked for since the last refresh counted as current -- the transposed images, which register their matrices one refresh at a
        time, served the previous step's weights to the data-gradient products under torch.optim.)"""
        reg = self._owners.setdefault(which, {})
        reg[off] = owners
        ver = tuple(t._version for t in owners)
        seen = self._ver.setdefault(which, {})
        if {"p": self._planes_tag, "q": self._pair_tag, "t": self._tp["tag"], "u": self._tq["tag"]}[which] == self._tag() and seen.get(off) == ver:
            return False
        seen.clear()
        for o2, ow in reg.items():
            seen[o2] = tuple(t._version for t in ow)
        return True

    def planes_of(self, off: int, rows: int, cols: int, owners=()):
        """plane operand of the matrix [rows, cols] stored at element offset `off` of the parameter buffer (None if its layout does not
        allow it)"""
        if cols % 32 or off % 8:
            return None
        if self._planes is None:
            self._planes = torch.empty((3, self.total), device=self.pflat.device, dtype=torch.int16)
        key = (off, rows, cols)
        self._plain_keys.add(key)
        if len(self._plain_keys) <= 16:
            # few matrices want the bf16 image (with the fp16-pair forms on: the 12 attention-output projections of bert-base, 7 MB of a
            # 435 MB buffer): each is split on its own, once per parameter version -- not the whole buffer (0.2 ms per step)
            tag = (self._tag(), tuple(t._version for t in owners))
            if self._plain_tags.get(key) != tag:
                with torch.no_grad():
                    ops.split_planes(self.pflat.detach()[off:off + rows * cols].view(rows, cols),
                                     out=ops.Planes(self._planes[:, off:off + rows * cols].view(3, rows, cols), rows, cols, cols))
                self._plain_tags[key] = tag
            return ops.Planes(self._planes[:, off:off + rows * cols].view(3, rows, cols), rows, cols, cols)
        if self._stale("p", off, owners):
            with torch.no_grad():
                ops.split_planes(self.pflat.detach().view(-1, 32), out=ops.Planes(self._planes.view(3, -1, 32), self.total // 32, 32, 32))
            self._planes_tag = self._tag()
        return ops.Planes(self._planes[:, off:off + rows * cols].view(3, rows, cols), rows, cols, cols)

    def pair_of(self, off: int, rows: int, cols: int, owners=()):
        """the same matrix as an fp16-pair plane operand (csrc/gemm_planes.hip FORM 1): one launch per optimizer step for the whole buffer"""
        if cols % 32 or off % 8:
            return None
        if self._pair is None:
            self._pair = torch.empty((2, self.total), device=self.pflat.device, dtype=torch.int16)
        if self._stale("q", off, owners):
            with torch.no_grad():
                ops.split_planes_pair(self.pflat.detach().view(-1, 32), out=ops.Planes(self._pair.view(2, -1, 32), self.total // 32, 32, 32))
            self._pair_tag = self._tag()
        return ops.Planes(self._pair[:, off:off + rows * cols].view(2, rows, cols), rows, cols, cols)

    def planes_t_of(self, off: int, rows: int, cols: int, owners=(), pair=False):
        """plane operand of the TRANSPOSE of that matrix ([cols, rows], reduction over rows); pair: as two fp16 planes (form 1)"""
        if off % 8:
            return None
        st = self._tq if pair else self._tp
        key = (off, rows, cols)
        if key not in st["jobs"]:
            ld = (rows + 31) // 32 * 32
            slot = sum(c * l for (_, _, c), (_, l) in st["jobs"].items())
            st["jobs"][key] = (slot, ld)
            st["tbl"] = None
        if st["tbl"] is None:
            tot = sum(c * l for (_, _, c), (_, l) in st["jobs"].items())
            st["buf"] = torch.empty((2 if pair else 3, (tot + 7) // 8 * 8), device=self.pflat.device, dtype=torch.int16)
            rows_, first = [], 0
            for (o, r, c), (slot, ld) in st["jobs"].items():
                rows_.append([o, r, c, slot, ld, first])
                first += ((ld + 63) // 64) * ((c + 63) // 64)
            st["tiles"] = first
            st["tbl"] = torch.tensor(rows_, dtype=torch.int64).to(self.pflat.device)
            st["tag"] = None
        which = "u" if pair else "t"
        if self._stale(which, off, owners):
            (ops.split_planes_pair_t_batched if pair else ops.split_planes_t_batched)(self.pflat, st["buf"], st["tbl"], len(st["jobs"]), st["tiles"])
            st["tag"] = self._tag()
        slot, ld = st["jobs"][key]
        return ops.Planes(st["buf"][:, slot:slot + cols * ld].view(2 if pair else 3, cols, ld), cols, rows, ld)

    def view(self, flat: torch.Tensor, i: int) -> torch.Tensor:
        """parameter i's slice of another flat buffer of this layout (optimizer state), shaped / laid out like the parameter"""
        return _phys_view(flat, self.offsets[i], self.params[i].data)


class NamedParams(list):
    """[(name, parameter)] that remembers the reference's FULL parameter list of the group (`ref_names`): torch optimizer checkpoints
    key their state by index into that list (train_SROIE.py:215-221 keeps the never-used tensors in it), so the indices written and
    read by _FlatOptimizer.state_dict / load_state_dict stay those of the reference's optimizer even though the unused tensors are
    kept out of the flat buffers"""
    ref_names: List[str] = None


def split_parameters(model: torch.nn.Module, unused: Sequence[str] = STATIC_UNUSED):
    """(cnn_named, bert_named) exactly like train_SROIE.py:215-221, minus the tensors that never receive a gradient
    (`unused`: name fragments; the reference keeps them in its optimizers, where `grad is None` makes every step skip them -- and
    where they still occupy an index: see NamedParams)."""
    cnn, bert = NamedParams(), NamedParams()
    cnn.ref_names, bert.ref_names = [], []
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        dst = bert if "bert_model" in name else cnn
        dst.ref_names.append(name)
        if any(u in name for u in unused):
            continue
        dst.append((name, p))
    return cnn, bert


def home_parameters(model: torch.nn.Module, device=None) -> List[FlatGroup]:
    """Flat parameter / gradient storage owned by the MODEL (called by ViBERTgridNet at its first training forward): the trainable
    parameters move into one flat buffer per optimizer group of the reference (train_SROIE.py:215-221: "bert_model" in name -> AdamW,
    the rest -> SGD), their `.grad` become views of a flat gradient buffer that the weight-gradient kernels accumulate into, and the
    plane / filter images the matrix kernels read are refreshed once per weight version for the whole buffer.  None of this depends on
    the optimizer class the caller constructs: torch.optim.SGD / AdamW update the views in place (their version counters tell the
    caches), FusedSGD / FusedAdamW adopt the groups they find.  Groups that are already in place (and still valid) are kept."""
    cnn, bert = split_parameters(model)
    groups = []
    for named in (cnn, bert):
        if not named:
            continue
        found = {}
        for _, p in named:
            g = getattr(p, "_vbg_flat", (None,))[0]
            found[id(g)] = g
        if None not in found.values() and all(g.valid() for g in found.values()):
            # already homed (an optimizer of vbg.optim built before the first forward, possibly over a different split): kept as is
            groups.extend(g for g in found.values() if all(g is not h for h in groups))
            continue
        dev = device if device is not None else named[0][1].device
        g = FlatGroup(list(named), dev)
        g.ref_names = list(named.ref_names)
        groups.append(g)
    return groups


class ModelHome:
    """What ViBERTgridNet keeps about the flat storage its parameters live in: the groups, and -- for graphs that depend on the data --
    which parameters took part in the current backward (post-accumulate hooks fire for every parameter whose autograd node ran, also
    when a Function wrote the gradient itself and returned None), so that the others get `.grad = None` back when the backward ends,
    as torch.optim expects of parameters that received no gradient (it skips them: no weight decay, no momentum step)."""

    def __init__(self, model, track_unused: bool):
        self.groups = home_parameters(model)
        self.touched = set() if track_unused else None
        if track_unused:
            for g in self.groups:
                for p in g.params:
                    if not getattr(p, "_vbg_touch_hook", False):
                        p.register_post_accumulate_grad_hook(self._touch)
                        p._vbg_touch_hook = True
                    p._vbg_home = self

    @staticmethod
    def _touch(p):
        h = getattr(p, "_vbg_home", None)
        if h is not None and h.touched is not None:
            h.touched.add(id(p))

    def valid(self) -> bool:
        return all(g.valid() for g in self.groups)

    def drop_untouched(self):
        """end of a backward (classifier_mode full): a parameter that took no part in it gets `.grad = None` back -- but only where arm()
        attached the view in THIS backward.  A gradient that already existed when the backward started (gradient accumulation, DDP
        `no_sync` micro-steps) stays, as torch would have left it."""
        t = self.touched
        for g in self.groups:
            for i in g._armed:
                p = g.params[i]
                if id(p) not in t:
                    p.grad = None
            g._armed = []


def _torch_defaults(cls, **kw):
    """the param_group keys of the torch optimizer this one stands in for (so a checkpoint written here loads into it)"""
    return dict(cls([torch.nn.Parameter(torch.zeros(1))], **kw).defaults)


SEG_CHUNK = 4096          # elements per row of the chunk table (16 KB per buffer: 4 float4 trips of a 256-thread block)
MAX_GROUPS = ops.OPTIM_MAX_GROUPS
_UNSUPPORTED = (("nesterov", False), ("dampening", 0), ("amsgrad", False), ("maximize", False))


class ParamGroups(list):
    """[{"params": [(name, parameter), ...], **overrides}] that remembers the one list the groups were cut from (`layout`: the
    model's registration order), which decides the order of the flat buffers -- the groups themselves never do"""
    layout = None


def decay_groups(named, no_decay=("bias", "LayerNorm.weight"), **no_decay_overrides):
    """The two param groups of the usual fine-tuning split, for FusedAdamW / FusedSGD: parameters whose name contains one of the
    `no_decay` fragments go into the second group, which overrides `weight_decay=0.0` (or whatever `no_decay_overrides` says
    instead); everything else keeps the constructor's defaults:

        opt = FusedAdamW(decay_groups(bert_named), device, lr=5e-5, weight_decay=0.01)

    A layer-wise list is built the same way, keyed on the `layer.N.` part of the name -- one dict per layer (times the decay split,
    if wanted), at most 32 dicts in all:

        def depth(name):                                   # embeddings 0, encoder layer N -> N + 1
            return int(name.split("layer.")[1].split(".")[0]) + 1 if "layer." in name else 0
        groups = [{"params": [(n, p) for n, p in named if depth(n) == d], "lr": 5e-5 * 0.9 ** (12 - d)} for d in range(13)]

    The groups only choose hyper-parameters: the flat layout, the gradient buckets and the single launch stay as they are.  The
    list returned here remembers `named`, so a flat buffer the optimizer has to create is laid out as for the single list; with a
    hand-built list pass `layout=named` to the optimizer for the same effect (otherwise the layout follows the groups in the order
    given -- correct, but the gradient buckets of FlatReducer then no longer fill in backward order)."""
    named = list(named)
    if not no_decay_overrides:
        no_decay_overrides = {"weight_decay": 0.0}
    plain = [(n, p) for n, p in named if not any(k in n for k in no_decay)]
    bare = [(n, p) for n, p in named if any(k in n for k in no_decay)]
    groups = ParamGroups([{"params": plain}, {"params": bare, **no_decay_overrides}])
    groups.layout = named
    return groups


def run_table(group: FlatGroup, group_of: Dict[int, int]):
    """[(start, length, group)] over the flat layout: consecutive slots of the same param group merge into one run, a run covers its
    slots' padding (slots are padded to 8 elements), and nothing covers [end of the last slot, total).  group_of: id(param) -> index;
    a parameter of the layout that group_of leaves out (fuse(): no gradient in this step) is covered by no run"""
    runs = []
    for p, off in zip(group.params, group.offsets):
        if id(p) not in group_of:
            continue
        k, end = group_of[id(p)], off + (p.numel() + 7) // 8 * 8
        if runs and runs[-1][2] == k and runs[-1][0] + runs[-1][1] == off:
            runs[-1][1] = end - runs[-1][0]
        else:
            runs.append([off, end - off, k])
    return [tuple(r) for r in runs]


def chunk_rows(runs, chunk: int):
    """the runs cut into rows (start, length, group) of at most `chunk` elements ([n, 3] int64): the kernels give one block a row at a
    time, so the work per block is bounded by `chunk`, not by the longest run"""
    import numpy as np
    if chunk < 4 or chunk % 4:
        raise ValueError("chunk length: a positive multiple of 4 elements")
    runs = np.asarray(runs, dtype=np.int64).reshape(-1, 3)
    per = (runs[:, 1] + chunk - 1) // chunk
    which = np.repeat(np.arange(len(runs)), per)
    k = np.arange(len(which)) - np.repeat(np.cumsum(per) - per, per)          # index of the row inside its run
    start = runs[which, 0] + k * chunk
    length = np.minimum(chunk, runs[which, 0] + runs[which, 1] - start)
    return np.stack([start, length, runs[which, 2]], axis=1)


class _FlatOptimizer(torch.optim.Optimizer):
    """A torch.optim.Optimizer whose parameters, gradients and state live in flat buffers and whose step is one HIP launch.
    Being an Optimizer, it plugs into the reference's loop unchanged: `StepLR(optimizer=...)` (train_SROIE.py:247) and
    `scaler.step(optimizer)` / `scaler.unscale_` (pipeline/train_val_utils.py:274-278) operate on `param_groups` and on the
    `.grad` views; `state_dict()` / `load_state_dict()` use torch's own optimizer checkpoint format (per-parameter state keyed by
    the parameter's index in the caller's list), so optimizer checkpoints interchange with torch.optim.SGD / AdamW
    (train_SROIE.py:377-416 saves them, resume loads them).
    One deliberate difference: the step is element-wise over the whole flat range, so a parameter that received NO gradient in a
    step still gets weight decay / momentum applied (torch skips `grad is None` parameters).  On this model that only concerns the
    per-class nets of classifier_mode full in steps where no segment was predicted positive.

    Two things are called "group" here and they are different: `self.group` is the FlatGroup, the ONE flat buffer all parameters of
    this optimizer live in (what FlatReducer, clip_grad_norm_ and the model's plane caches work on); `self.param_groups` are torch's
    param groups, sets of parameters that share hyper-parameters.  The constructor takes either one list of (name, parameter) pairs
    (one param group) or a list of dicts `{"params": [(name, p), ...], "lr": ..., "weight_decay": ...}` with torch's own keys, one
    param group each; missing keys take the constructor's defaults.  All param groups live in the one FlatGroup, whose layout does not
    depend on them; `step()` reads every param group's current values on each call (schedulers, per-step weight-decay schedules) and
    hands them to one segmented launch.  With one param group the step is the plain whole-range launch.  Checkpoints of several
    groups number the parameters group by group in the order given, as torch.optim does for the same groups.  Flat storage is fixed
    at construction: `add_param_group` afterwards raises.  seg_chunk: elements per row of the chunk table (default SEG_CHUNK); layout: the
    (name, parameter) list that orders a flat buffer created here (decay_groups() supplies it; default: the groups in the order given)."""

    _state_names: Tuple[str, ...] = ()

    def __init__(self, named, device, defaults: Dict, seg_chunk=None, layout=None):
        if layout is None:
            layout = getattr(named, "layout", None)
        named = list(named) if not hasattr(named, "ref_names") else named
        if len(named) > 0 and isinstance(named[0], dict):
            dicts = [dict(d) for d in named]
            if len(dicts) > MAX_GROUPS:
                raise ValueError(f"{len(dicts)} param groups: one segmented launch carries at most {MAX_GROUPS}")
            seen = set()
            for k, d in enumerate(dicts):
                if "params" not in d or len(d["params"]) == 0:
                    raise ValueError(f"param group {k} is empty")
                for n, p in d["params"]:
                    if id(p) in seen:
                        raise ValueError(f"parameter {n} appears in more than one param group")
                    seen.add(id(p))
                self._check_options({**defaults, **{k2: v for k2, v in d.items() if k2 != "params"}})
        else:
            dicts = [{"params": named}]
        self._check_options(defaults)
        # the single list keeps the reference's indices (NamedParams.ref_names); several groups are numbered group by group
        ref = getattr(dicts[0]["params"], "ref_names", None) if len(dicts) == 1 else None
        named = [np_ for d in dicts for np_ in d["params"]]
        flat_named = named
        if layout is not None:              # the order of the flat buffers: the one list the groups were cut from, not the groups
            flat_named = list(layout)
            if len(flat_named) != len(named) or {id(p) for _, p in flat_named} != {id(p) for _, p in named}:
                raise ValueError("layout must list exactly the parameters of the param groups, each once")
        # a group the model (or an earlier optimizer) already homed exactly these parameters in is adopted, not rebuilt
        homes = {id(getattr(p, "_vbg_flat", (None,))[0]): getattr(p, "_vbg_flat", (None,))[0] for _, p in named}
        g = next(iter(homes.values())) if len(homes) == 1 else None
        if (g is not None and len(g.params) == len(named) and set(g._index) == {id(p) for _, p in named} and g.valid()
                and g.pflat.device.type == torch.device(device).type and torch.device(device).index in (None, g.pflat.device.index)):
            self.group = g
            g.zero_grad()
        else:
            self.group = FlatGroup(flat_named, device)
        if ref is not None:                 # indices of the reference optimizer's full parameter list (unused tensors included)
            assert set(n for n, _ in named) <= set(ref)
            self.group.ref_names = list(ref)
        self._group_names = [[n for n, _ in d["params"]] for d in dicts]
        self._constructed = False
        super().__init__([dict(d, params=[p for _, p in d["params"]]) for d in dicts], defaults)
        self._constructed = True
        self.grad_scale = 1.0
        self.steps = 0
        # several param groups: the runs of each over the flat layout, cut into rows of bounded length, uploaded once
        self.segmented = len(dicts) > 1
        self.runs, self.chunk_rows, self.table = None, None, None
        if self.segmented:
            group_of = {id(p): k for k, d in enumerate(dicts) for _, p in d["params"]}
            self.runs = run_table(self.group, group_of)
            self.chunk_rows = chunk_rows(self.runs, int(seg_chunk or SEG_CHUNK))
            self.table = ops.chunk_table(self.chunk_rows, len(dicts), self.group.total, self.group.pflat.device)
        self._vbg_clip = None               # the device coefficient clip_in_step left for the next step()
        self._clip_tbl = None
        import weakref
        self.group._vbg_optimizer = weakref.ref(self)          # (ViBERTgridNet._home: a group a live optimizer steps is never silently replaced)

    def _clip_table(self):
        """the chunk table clip_in_step's norm pass and the clipping step walk: the param groups' own table, or -- one param group, whose
        plain step is the whole-range launch -- one kernel group over the whole layout, built once"""
        if self.segmented:
            return self.table
        if self._clip_tbl is None:
            g = self.group
            self._clip_tbl = ops.chunk_table(chunk_rows([(0, g.total, 0)], SEG_CHUNK), 1, g.total, g.pflat.device)
        return self._clip_tbl

    @staticmethod
    def _check_options(opts: Dict):
        """what the kernels do not implement is refused where the param group is created, not dropped"""
        for key, off in _UNSUPPORTED:
            if key in opts and opts[key] != off:
                raise ValueError(f"{key}={opts[key]!r} is not supported by the fused optimizers (only {key}={off!r})")

    def add_param_group(self, param_group):
        if getattr(self, "_constructed", True):
            raise NotImplementedError("flat storage is fixed at construction: pass every param group to the constructor, as a list of "
                                      "dicts {'params': [(name, parameter), ...], 'lr': ..., 'weight_decay': ...}")
        super().add_param_group(param_group)

    def zero_grad(self, set_to_none: bool = False):
        self._vbg_clip = None               # (a pending clip coefficient belongs to the gradients it was computed from)
        self.group.zero_grad()

    # ---- checkpoint format of torch.optim ---------------------------------------------------------------------------
    def _flat_state(self) -> Dict[str, torch.Tensor]:
        raise NotImplementedError

    def _ref_lists(self):
        """per param group, the names its checkpoint indices stand for, in index order: the reference's full list for the single
        group (never-used tensors keep their index), the group's own parameters in the order given otherwise"""
        return [list(self.group.ref_names)] if not self.segmented else self._group_names

    def state_dict(self):
        g = self.group
        pos = {n: i for i, n in enumerate(g.names)}
        lists = self._ref_lists()
        state, groups, ref_i = {}, [], 0
        for pg, names in zip(self.param_groups, lists):
            groups.append(dict({k: v for k, v in pg.items() if k != "params"}, params=list(range(ref_i, ref_i + len(names)))))
            for n in names:
                if self.steps > 0 and n in pos:          # (not in pos: a tensor that never receives a gradient -- torch keeps no state for it either)
                    i = pos[n]
                    st = {k: g.view(flat, i).clone() for k, flat in self._flat_state().items()}
                    if "exp_avg" in st:
                        st = {"step": torch.tensor(float(self.steps)), **st}
                    state[ref_i] = st
                ref_i += 1
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd):
        g = self.group
        pos = {n: i for i, n in enumerate(g.names)}
        lists = self._ref_lists()
        got = [len(src["params"]) for src in sd.get("param_groups", [])]
        if sd.get("param_groups") and got != [len(names) for names in lists]:
            raise ValueError(f"optimizer checkpoint covers {got} parameters per param group, this optimizer's reference lists have "
                             f"{[len(names) for names in lists]}: build the optimizer from split_parameters(model) (and the same param "
                             "groups) so that the indices are the reference's")
        for pg, src in zip(self.param_groups, sd["param_groups"]):
            pg.update({k: v for k, v in src.items() if k != "params"})
        flats = self._flat_state()
        for f in flats.values():
            f.zero_()
        self.steps = 0
        ref_names = [n for names in lists for n in names]
        for ref_i, st in sd["state"].items():
            n = ref_names[int(ref_i)]
            if n not in pos:                 # state of a tensor kept out of the flat buffers (it never receives a gradient)
                continue
            i = pos[n]
            for k, flat in flats.items():
                if k in st and st[k] is not None:
                    g.view(flat, i).copy_(st[k])
            if "step" in st:
                self.steps = max(self.steps, int(float(st["step"])))
            elif flats:
                self.steps = max(self.steps, 1)


class FusedSGD(_FlatOptimizer):
    """torch.optim.SGD(momentum, weight_decay) semantics (dampening 0, no nesterov) over a flat buffer.
    `grad_scale` is a HOST float here (1 / world size, set by FlatReducer).  torch.amp.GradScaler's protocol for optimizers that
    consume the scale themselves assigns a device tensor to an attribute of that name and deletes it after the step, so this class
    does not declare `_step_supports_amp_scaling`: under a GradScaler it takes the scaler's generic route (unscale_, inf check on
    the host).  The in-launch unscale and inf skip exist for stock torch.optim objects: `fuse(optimizer, amp_scaling=True)`."""

    def __init__(self, named, device, lr, momentum=0.0, weight_decay=0.0, seg_chunk=None, layout=None):
        super().__init__(named, device, _torch_defaults(torch.optim.SGD, lr=lr, momentum=momentum, weight_decay=weight_decay), seg_chunk, layout)
        self.mom = torch.zeros_like(self.group.pflat)

    def _flat_state(self):
        return {"momentum_buffer": self.mom}

    @torch.no_grad()
    def step(self, closure=None):
        clip = _take_clip(self)
        if clip is not None:
            first = ops.SGD_FIRST if self.steps == 0 else 0
            ops.sgd_step_seg_clip(self.group.pflat, self.group.gflat, self.mom, self._clip_table(),
                                  [(g["lr"], g["momentum"], 0.0, g["weight_decay"], first) for g in self.param_groups], None, None, clip,
                                  self.grad_scale, keep_mom=True)
        elif self.segmented:
            ops.sgd_step_seg(self.group.pflat, self.group.gflat, self.mom, self.table,
                             [(g["lr"], g["momentum"], g["weight_decay"]) for g in self.param_groups], self.steps == 0, self.grad_scale)
        else:
            g = self.param_groups[0]
            ops.sgd_step(self.group.pflat, self.group.gflat, self.mom, float(g["lr"]), float(g["momentum"]), float(g["weight_decay"]),
                         self.steps == 0, self.grad_scale)
        self.steps += 1
        ops.bump_weight_epoch()


class FusedAdamW(_FlatOptimizer):
    """torch.optim.AdamW semantics (decoupled weight decay, bias correction, amsgrad off).  Like FusedSGD it keeps a host float
    `grad_scale` and therefore does not declare `_step_supports_amp_scaling` (see there)."""

    def __init__(self, named, device, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, seg_chunk=None, layout=None):
        super().__init__(named, device, _torch_defaults(torch.optim.AdamW, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay), seg_chunk,
                         layout)
        self.m = torch.zeros_like(self.group.pflat)
        self.v = torch.zeros_like(self.group.pflat)

    def _flat_state(self):
        return {"exp_avg": self.m, "exp_avg_sq": self.v}

    @torch.no_grad()
    def step(self, closure=None):
        self.steps += 1
        clip = _take_clip(self)
        if clip is not None:
            ops.adam_step_seg_clip(self.group.pflat, self.group.gflat, self.m, self.v, None, self._clip_table(),
                                   [(g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], self.steps, 0) for g in self.param_groups],
                                   None, None, clip, self.grad_scale)
        elif self.segmented:
            ops.adamw_step_seg(self.group.pflat, self.group.gflat, self.m, self.v, self.table,
                               [(g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"]) for g in self.param_groups],
                               self.steps, self.grad_scale)
        else:
            g = self.param_groups[0]
            ops.adamw_step(self.group.pflat, self.group.gflat, self.m, self.v, float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]),
                           float(g["eps"]), float(g["weight_decay"]), self.steps, self.grad_scale)
        ops.bump_weight_epoch()


# ---- stock torch.optim objects on the fused kernels --------------------------------------------------------------------------
class _Fallback(Exception):
    """this step() call goes to torch's own step (the reason is the message)"""


class _NoGradients(_Fallback):
    pass


def _take_clip(optimizer):
    """the clip coefficient clip_in_step left on the optimizer (one fp32 element of device memory) or None; a step consumes it"""
    clip = getattr(optimizer, "_vbg_clip", None)
    optimizer._vbg_clip = None
    return clip


class _FusedState:
    """what fuse() keeps on the optimizer instance (`_vbg_fused`): the flat state buffers of the FlatGroup last stepped, which state
    tensors are views of them, and the chunk tables built so far.  With amp_scaling: what the last launch under GradScaler's protocol
    did to `optimizer.state` on the host, until reconcile() has learnt whether the device skipped that step"""
    MAX_TABLES = 8

    def __init__(self, seg_chunk, amp=False):
        self.seg_chunk = int(seg_chunk or SEG_CHUNK)
        self.amp = bool(amp)
        self.skipped = 0          # steps that found_inf turned into no-ops (counted at reconcile; a skipped fallback at once)
        self._pending = None      # (host copy of found_inf, event behind the copy or None, undo) of the last AMP launch
        self._flag = None         # the pinned host scalar the copies go to
        self.group = None
        self.flat = {}            # torch's state key -> flat buffer of the group's layout
        self.owned = {}           # (id(param), key) -> the view of self.flat[key] that optimizer.state[param][key] must still be
        self.tables = {}          # per-slot kernel-group assignment (tuple over the layout, -1: absent) -> ChunkTable
        self.rows = None          # the chunk rows of the last fused step ([n, 3] int64), for inspection
        self.launches = 0
        self.fallbacks = 0
        self.last_fallback = None

    def adopt(self, group):
        if self.group is not group:          # another home (the model re-homed its parameters): state held in the old buffers is
            self.group, self.flat, self.owned, self.tables = group, {}, {}, {}          # separate tensors from here on, copied in below

    def buffer(self, key):
        if key not in self.flat:
            self.flat[key] = torch.zeros_like(self.group.pflat)
        return self.flat[key]

    def home(self, st, p, i, key, fresh):
        """optimizer.state[p][key] as a view of the flat buffer: a tensor torch's own step or load_state_dict put there is copied in"""
        own = self.owned.get((id(p), key))
        cur = None if fresh else st.get(key)
        if own is not None and cur is own:
            return
        if own is None:
            own = self.owned[(id(p), key)] = self.group.view(self.buffer(key), i)
        if cur is not None:
            own.copy_(cur)
        elif key != "momentum_buffer":          # (a first momentum step overwrites its slot)
            own.zero_()
        st[key] = own

    def defer(self, found_inf, undo):
        """after an AMP launch: the host does not know whether the kernel took its early exit and does not wait to find out.  The flag
        travels to a pinned host scalar behind the launch; `undo` takes the step's host bookkeeping back if it turns out set"""
        if found_inf.is_cuda:
            if self._flag is None:
                self._flag = torch.zeros(1, dtype=torch.float32).pin_memory()
            self._flag.copy_(found_inf.detach().reshape(1), non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._pending = (self._flag, ev, undo)
        else:
            self._pending = (found_inf.detach().reshape(1).clone(), None, undo)

    def reconcile(self):
        """make `optimizer.state` what torch's own loop leaves behind if the last step under GradScaler's protocol was skipped on the
        device: step counts back by one, state entries and first momentum buffers that step created removed.  Runs at the start of
        every step(), in state_dict() and load_state_dict(); call it before reading `optimizer.state` directly right after a
        `scaler.step(optimizer)`.  Waits for ONE event, the copy of found_inf behind that launch -- long complete by the next step of a
        training loop"""
        if self._pending is None:
            return
        flag, ev, undo = self._pending
        self._pending = None
        if ev is not None and not ev.query():
            ev.synchronize()
        if float(flag) != 0.0:
            undo()
            self.skipped += 1

    def table(self, assign, ngroups, note=True):
        t = self.tables.get(assign)
        if t is None:
            g = self.group
            rows = chunk_rows(run_table(g, {id(p): k for p, k in zip(g.params, assign) if k >= 0}), self.seg_chunk)
            if len(self.tables) >= self.MAX_TABLES:
                self.tables.pop(next(iter(self.tables)))
            t = self.tables[assign] = ops.chunk_table(rows, ngroups, g.total, g.pflat.device)
            t.chunk_rows = rows
        if note:
            self.rows = t.chunk_rows
        return t


def _parent_step(cls):
    """torch's own step of `cls` without the hook wrapper torch.optim.Optimizer puts around every step (the subclass's step carries one
    already: pre / post hooks run once per call)"""
    f = cls.step
    return getattr(f, "__wrapped__", f) if getattr(f, "hooked", False) else f


class _FusedStock:
    """step() of the classes fuse() switches a torch.optim instance to.  Everything else -- constructor, param_groups, state, zero_grad,
    load_state_dict, hooks -- is the parent's."""
    _vbg_parent = None

    @torch.no_grad()
    def step(self, closure=None):
        fs = self._vbg_fused
        fs.reconcile()
        clip = _take_clip(self)          # (consumed by this call whatever becomes of it: launch, skipped step, fallback)
        # GradScaler's protocol (fuse(amp_scaling=True)): for the length of this call the scaler has put two device scalars on the
        # object, `found_inf` and `grad_scale` (None: the caller has run scaler.unscale_ already)
        found_inf = getattr(self, "found_inf", None) if fs.amp else None
        amp = None if found_inf is None else (getattr(self, "grad_scale", None), found_inf)
        known = None if amp is None else set(self.state)
        if closure is None:
            try:
                plan = self._vbg_plan(fs)
                if amp is not None:
                    self._vbg_amp_check(fs, *amp)
            except _Fallback as e:
                fs.fallbacks += 1
                fs.last_fallback = str(e)
            else:
                if amp is None:
                    self._vbg_launch(fs, *plan, clip=clip)
                else:
                    undo = self._vbg_launch(fs, *plan, amp=amp, clip=clip)
                    created = [p for p in self.state if p not in known]
                    fs.defer(found_inf, lambda: self._vbg_undo(undo, created))
                fs.launches += 1
                ops.bump_weight_epoch()          # (after a launch that turns out skipped: one redundant re-split of the plane images)
                return None
        else:
            fs.fallbacks += 1
            fs.last_fallback = "closure"
        if amp is not None:
            # torch's own step knows nothing of the two attributes: do here what GradScaler would have done before calling it
            self._vbg_undo([], [p for p in self.state if p not in known and not self.state[p]])          # (entries the plan touched)
            if float(found_inf) != 0.0:          # (a sync, on this rare path only)
                fs.skipped += 1
                return None
            self._vbg_unscale(amp[0])
            self._vbg_clip_grads(clip)
            # (torch's single-tensor and foreach steps read the two attributes themselves and refuse them: out of sight for the call,
            # back for GradScaler to delete)
            hidden = {k: self.__dict__.pop(k) for k in ("grad_scale", "found_inf") if k in self.__dict__}
            try:
                return _parent_step(self._vbg_parent)(self, closure)
            finally:
                self.__dict__.update(hidden)
        self._vbg_clip_grads(clip)
        return _parent_step(self._vbg_parent)(self, closure)

    def zero_grad(self, set_to_none: bool = True):
        self._vbg_clip = None               # (a pending clip coefficient belongs to the gradients it was computed from)
        return super().zero_grad(set_to_none)

    @staticmethod
    def _vbg_amp_check(fs, grad_scale, found_inf):
        dev = fs.group.pflat.device
        for t in (found_inf,) if grad_scale is None else (grad_scale, found_inf):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.numel() != 1 or t.device != dev:
                raise _Fallback("grad_scale / found_inf is not one fp32 element on the flat buffers' device")

    def _vbg_undo(self, undo, created):
        """the host bookkeeping of a step the device skipped, taken back (`undo`: callables of _vbg_launch; `created`: parameters whose
        state entry did not exist before that step)"""
        for f in undo:
            f()
        for p in created:
            self.state.pop(p, None)

    def _vbg_unscale(self, grad_scale):
        """GradScaler.unscale_ for a step that falls back to torch's own: the present gradients times the inverse scale, in place"""
        if grad_scale is None:
            return
        inv = grad_scale.double().reciprocal().float()
        for (dev, _), grads in self._vbg_grads().items():
            torch._amp_foreach_non_finite_check_and_unscale_(grads, torch.zeros(1, device=dev), inv.to(dev))

    def _vbg_clip_grads(self, clip):
        """a pending clip coefficient for a step that falls back to torch's own: the present gradients times the device scalar, in
        place, as torch.nn.utils.clip_grad_norm_ applies it"""
        if clip is None:
            return
        for (dev, _), grads in self._vbg_grads().items():
            torch._foreach_mul_(grads, clip.reshape(()).to(dev))

    def _vbg_grads(self):
        """(device, dtype) -> the present gradients (the values of a sparse one)"""
        by = {}
        for pg in self.param_groups:
            for p in pg["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse:
                    g = g._values()
                by.setdefault((g.device, g.dtype), []).append(g)
        return by

    def _vbg_present(self, fs):
        """[(param group index, parameter, slot index)] of the parameters with a gradient, after the checks that decide whether this
        call can be one launch over one FlatGroup"""
        present, group = [], None
        for k, pg in enumerate(self.param_groups):
            if pg.get("fused") or pg.get("capturable") or pg.get("differentiable"):
                raise _Fallback("fused / capturable / differentiable param group")
            for p in pg["params"]:
                g = p.grad
                if g is None:
                    continue
                home = getattr(p, "_vbg_flat", None)
                if home is None:
                    raise _Fallback("a parameter with a gradient is not homed in flat storage")
                if group is None:
                    group = home[0]
                elif home[0] is not group:
                    raise _Fallback("the parameters with a gradient live in more than one flat group")
                i = group._index[id(p)]
                if g is not group.gviews[i]:
                    raise _Fallback("a .grad is not the flat gradient view (sparse, replaced or cast)")
                present.append((k, p, i))
        if group is None:
            raise _NoGradients("no parameter has a gradient")
        if not group.valid():
            raise _Fallback("the parameters moved away from their flat buffer (Module.to / a fresh .data)")
        fs.adopt(group)
        return present

    def _vbg_norm_table(self):
        """clip_in_step: (FlatGroup, chunk table over the rows of the parameters with a gradient); the table is the step's own whenever
        that has one kernel group"""
        fs = self._vbg_fused
        have = {i for _, _, i in self._vbg_present(fs)}
        return fs.group, fs.table(tuple(0 if i in have else -1 for i in range(len(fs.group.params))), 1, note=False)

    def state_dict(self):
        """torch's checkpoint, with the state tensors cloned: the views would drag the whole flat buffers into the file"""
        self._vbg_fused.reconcile()
        sd = super().state_dict()
        sd["state"] = {i: {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in st.items()} for i, st in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        self._vbg_fused.reconcile()
        return super().load_state_dict(state_dict)


def _combos(fs, keys):
    """kernel groups: the distinct keys in order of first appearance -> (per-slot assignment over the layout, distinct keys)"""
    index, assign = {}, [-1] * len(fs.group.params)
    for i, key in keys:
        j = index.get(key)
        if j is None:
            j = index[key] = len(index)
        assign[i] = j
    if len(index) > MAX_GROUPS:
        raise _Fallback(f"{len(index)} combinations of param group and step count: one launch carries at most {MAX_GROUPS}")
    return tuple(assign), list(index)


class _StockSGD(_FusedStock, torch.optim.SGD):
    _vbg_parent = torch.optim.SGD

    def _vbg_plan(self, fs):
        present = self._vbg_present(fs)
        keys, homes = [], []
        for k, p, i in present:
            if self.param_groups[k]["momentum"] != 0:
                st = self.state[p]
                first = st.get("momentum_buffer") is None
                homes.append((st, p, i, first))
            else:
                first = False
            keys.append((i, (k, first)))
        assign, combos = _combos(fs, keys)
        return assign, combos, homes

    def _vbg_launch(self, fs, assign, combos, homes, amp=None, clip=None):
        undo = []
        for st, p, i, first in homes:
            if amp is not None and first:          # skipped: the slot was never written (and home() does not zero it), the key goes again
                undo.append((lambda st=st: st.__setitem__("momentum_buffer", None)) if "momentum_buffer" in st else
                            (lambda st=st: st.pop("momentum_buffer", None)))
            fs.home(st, p, i, "momentum_buffer", first)
        hp = []
        for k, first in combos:
            pg = self.param_groups[k]
            flags = ops.SGD_NESTEROV * bool(pg["nesterov"]) + ops.SGD_MAXIMIZE * bool(pg["maximize"]) + ops.SGD_FIRST * first
            hp.append((float(pg["lr"]), float(pg["momentum"]), float(pg["dampening"]), float(pg["weight_decay"]), flags))
        g = fs.group
        if clip is not None:
            ops.sgd_step_seg_clip(g.pflat, g.gflat, fs.flat.get("momentum_buffer"), fs.table(assign, len(hp)), hp, *(amp or (None, None)), clip)
        elif amp is None:
            ops.sgd_step_seg_opt(g.pflat, g.gflat, fs.flat.get("momentum_buffer"), fs.table(assign, len(hp)), hp, 1.0)
        else:
            ops.sgd_step_seg_amp(g.pflat, g.gflat, fs.flat.get("momentum_buffer"), fs.table(assign, len(hp)), hp, *amp)
        return undo


class _AdamStep(_FusedStock):
    def _vbg_plan(self, fs):
        present = self._vbg_present(fs)
        keys, homes = [], []
        for k, p, i in present:
            st = self.state[p]
            fresh = len(st) == 0
            ams = bool(self.param_groups[k]["amsgrad"])
            if not fresh and ("exp_avg" not in st or "exp_avg_sq" not in st or "step" not in st or (ams and "max_exp_avg_sq" not in st)):
                raise _Fallback("optimizer state without torch's keys")          # (torch's own step raises what it raises)
            keys.append((i, (k, 1 if fresh else int(st["step"]) + 1)))
            homes.append((st, p, i, fresh, ams))
        assign, combos = _combos(fs, keys)
        return assign, combos, homes

    def _vbg_launch(self, fs, assign, combos, homes, amp=None, clip=None):
        steps, undo = [], []
        for st, p, i, fresh, ams in homes:
            if fresh and amp is not None:          # skipped: an entry that was empty is empty again
                undo.append(st.clear)
            if fresh:
                st["step"] = torch.tensor(0.0, dtype=torch.float64 if torch.get_default_dtype() == torch.float64 else torch.float32)          # (on the host, as torch keeps it)
            fs.home(st, p, i, "exp_avg", fresh)
            fs.home(st, p, i, "exp_avg_sq", fresh)
            if ams:
                fs.home(st, p, i, "max_exp_avg_sq", fresh)
            steps.append(st["step"])
        hp, any_ams = [], False
        for k, step in combos:
            pg = self.param_groups[k]
            coupled = not pg.get("decoupled_weight_decay", False)
            flags = ops.ADAM_AMSGRAD * bool(pg["amsgrad"]) + ops.ADAM_MAXIMIZE * bool(pg["maximize"]) + ops.ADAM_COUPLED * coupled
            any_ams = any_ams or bool(pg["amsgrad"])
            hp.append((float(pg["lr"]), float(pg["betas"][0]), float(pg["betas"][1]), float(pg["eps"]), float(pg["weight_decay"]), step, flags))
        g = fs.group
        bufs = (g.pflat, g.gflat, fs.buffer("exp_avg"), fs.buffer("exp_avg_sq"), fs.buffer("max_exp_avg_sq") if any_ams else None, fs.table(assign, len(hp)), hp)
        if clip is not None:
            ops.adam_step_seg_clip(*bufs, *(amp or (None, None)), clip)
        elif amp is None:
            ops.adam_step_seg_opt(*bufs, 1.0)
        else:
            ops.adam_step_seg_amp(*bufs, *amp)
        if amp is not None:
            undo.insert(0, lambda: torch._foreach_sub_(steps, 1))          # (bias corrections always come from the true step count)
        torch._foreach_add_(steps, 1)
        return undo


class _StockAdam(_AdamStep, torch.optim.Adam):
    _vbg_parent = torch.optim.Adam


class _StockAdamW(_AdamStep, torch.optim.AdamW):
    _vbg_parent = torch.optim.AdamW


_STOCK = {torch.optim.SGD: _StockSGD, torch.optim.Adam: _StockAdam, torch.optim.AdamW: _StockAdamW}


def fuse(optimizer, seg_chunk=None, amp_scaling=False):
    """Make a stock torch.optim.SGD / Adam / AdamW whose parameters are homed in flat storage (home_parameters: ViBERTgridNet does it
    at its first training forward) step in ONE HIP launch, with torch's semantics kept exactly -- every option (nesterov, dampening,
    maximize, amsgrad, coupled or decoupled weight decay), parameters whose `.grad` is None skipped, per-parameter step counts,
    GradScaler, schedulers, torch's checkpoint format.  Returns the SAME object, its class switched to a subclass that overrides
    `step`; call it between building the optimizer and building its lr schedulers:

        optimizer_cnn = vbg.optim.fuse(torch.optim.SGD(cnn_params, lr=..., momentum=...))
        optimizer_bert = vbg.optim.fuse(torch.optim.AdamW(bert_params, lr=...))

    A step() call that cannot be one launch runs torch's own step for that call: a closure; a parameter with a gradient that is not
    homed (yet), lives in another flat group or has moved away from it (Module.to); a `.grad` that is not the flat gradient view (a
    sparse or replaced gradient); a param group with fused / capturable / differentiable set; optimizer state without torch's keys;
    more than 32 combinations of (param group, step count).  Both paths read and write the same `optimizer.state`: the moments are
    views of flat buffers under torch's own keys, and tensors that torch's step or load_state_dict put there are copied in at the next
    fused step.  `optimizer._vbg_fused` counts `launches` and `fallbacks` and keeps the reason of the last one.  seg_chunk: elements per
    row of the chunk tables (default SEG_CHUNK).

    amp_scaling=True declares `_step_supports_amp_scaling` on this instance, torch's protocol for optimizers that consume GradScaler's
    scale themselves: `scaler.step(optimizer)` then runs only its read-only inf check, puts the device scalars `grad_scale` and
    `found_inf` on the object for the length of the call, and the launch (`vbg_sgd_step_seg_amp` / `vbg_adam_step_seg_amp`) unscales
    the gradients and skips the step on an inf by itself -- no `unscale_` pass, no `found_inf.item()` drain.  A skipped step is then a
    launch that does nothing, and the host learns of it later: `optimizer._vbg_fused.reconcile()` (run by the next step(), by
    state_dict() and load_state_dict(); call it yourself before reading `optimizer.state` right after `scaler.step`) takes the step
    counts and the state entries of a skipped step back and counts it in `skipped`.  A call that falls back to torch's own step under
    the protocol does GradScaler's part first: it reads found_inf (a sync), returns on an inf, unscales the gradients otherwise.
    Without the two attributes (a plain `optimizer.step()`, a disabled scaler) the step is the one without the option."""
    cls = type(optimizer)
    if cls not in _STOCK:
        raise ValueError(f"fuse() takes instances of exactly torch.optim.SGD, Adam or AdamW, not {cls.__module__}.{cls.__qualname__}")
    for k, pg in enumerate(optimizer.param_groups):
        for key in ("capturable", "differentiable"):
            if pg.get(key):
                raise ValueError(f"param group {k} has {key}=True: not supported by the fused step")
    if "step" in vars(optimizer) or hasattr(optimizer.step, "_wrapped_by_lr_sched"):
        raise ValueError("optimizer.step is already wrapped (an lr scheduler was built on this optimizer): call fuse() before building "
                         "schedulers, so that they wrap the fused step")
    optimizer.__class__ = _STOCK[cls]
    optimizer._vbg_fused = _FusedState(seg_chunk, amp_scaling)
    optimizer._vbg_clip = None
    if amp_scaling:
        optimizer._step_supports_amp_scaling = True
    optimizer._patch_step_function()          # the step pre / post hooks of torch.optim.Optimizer, around the new step
    return optimizer


def clip_grad_norm_(optimizers, max_norm: float, norm_scale: float = 1.0) -> float:
    """torch.nn.utils.clip_grad_norm (pipeline/train_val_utils.py:281-282) over the flat gradient buffers."""
    dev = optimizers[0].group.gflat.device
    acc = torch.zeros((1,), device=dev, dtype=torch.float32)
    for o in optimizers:
        ops.sumsq(o.group.gflat, acc)
    total = float(acc.item()) ** 0.5 * norm_scale
    coef = max_norm / (total + 1e-6)
    if coef < 1.0:
        for o in optimizers:
            ops.scale_(o.group.gflat, coef)
    return total


_CLIP_PARTIALS = {}          # device -> the partials buffer clip_in_step's norm launches share (grown, never shrunk)


_NORM_KINDS = {2.0: 2, 1.0: 1, float("inf"): 0}          # norm_type -> the `kind` of vbg_grad_norm_seg / vbg_clip_coef_gate


def _clip_gate(when, dev):
    """clip_in_step's `when`: None, or (loss, threshold) checked by the statement the ops wrappers run -- the loss is handed on as it is and
    never read on the host"""
    if when is None:
        return None
    loss, threshold = ops._check_gate(when, dev, "clip_in_step", pair=(tuple, list))
    return (loss.detach(), threshold)


def clip_in_step(optimizers, max_norm: float, norm_scale: float = 1.0, scaler=None, norm_type=2.0, when=None) -> torch.Tensor:
    """torch.nn.utils.clip_grad_norm_ (norm type 2, 1 or inf) folded into the optimizer step, with no host sync and no pass of its own over the
    gradients beyond the norm: one `vbg_grad_sumsq_seg` launch per optimizer over its chunk table, one `vbg_clip_coef`, and the
    coefficient stays in device memory, pending on every listed optimizer until its next `step()` (or `scaler.step(optimizer)`), whose
    launch multiplies the gradients by it -- stored back to `.grad`, as torch leaves them -- right before the rule reads them
    (`vbg_sgd_step_seg_clip` / `vbg_adam_step_seg_clip`).  Returns the total norm as a 0-dim device tensor.

        total = vbg.optim.clip_in_step([optimizer_cnn, optimizer_bert], max_norm=2)          # pipeline/train_val_utils.py:281-282
        optimizer_cnn.step(); optimizer_bert.step()

    optimizers: any mix of FusedSGD / FusedAdamW and fuse()d stock optimizers -- all those whose gradients count towards the one norm.
    A stock optimizer contributes the parameters whose `.grad` is not None (torch's clip skips the others too), a FusedSGD / FusedAdamW
    its whole layout.  norm_scale multiplies the norm (FlatReducer's 1 / world), as in clip_grad_norm_.  scaler: pass the GradScaler
    when the gradients still hold scaled values (no `scaler.unscale_` call): the norm is divided by its scale on the device, and
    `scaler.step(optimizer)` on a `fuse(optimizer, amp_scaling=True)` object unscales, clips and steps in the one launch; on any other
    optimizer the scaler unscales as it always does and the launch only clips.  With a scaler made by fuse_scaler() the norm launches are
    `vbg_grad_sumsq_seg_inf`: they leave the scaler's inf flag for each optimizer as well, and its `scaler.step(optimizer)` under the
    amp_scaling protocol launches no check of its own.
    A step that falls back to torch's own (fuse(): a closure, ...) multiplies the present gradients by the coefficient first
    (`torch._foreach_mul_`); a step skipped by found_inf consumes the coefficient; `zero_grad()` before the step drops it; a second call
    while one is pending raises.  (A GradScaler that finds an inf never calls step() on an optimizer fused without amp_scaling: the
    coefficient then waits for the loop's zero_grad().)

    norm_type: 2, 1 or float("inf") (int or float), as torch.nn.utils.clip_grad_norm_(..., norm_type=...) defines them; anything else
    raises ValueError.  `error_if_nonfinite` is not offered: raising on the host is a host read of the norm by definition.

    when=(loss, threshold): the reference's `if train_loss > loss_clip_tresh:` around its clip (pipeline/train_val_utils.py:281), decided
    on the device.  loss: a one-element fp64 or fp32 tensor on the flat buffers' device (what ViBERTgridNet.forward returns, detached);
    it is only read by the two launches, never synchronised with.  threshold: a Python number.  The decision is torch's own
    `loss > threshold` in the loss tensor's dtype: strictly greater, a NaN loss closes the gate, +inf opens it.  Gate open: exactly the
    call without `when`.  Gate closed: the pending coefficient is exactly 1.0 (the next step() is the unclipped step bit for bit and
    leaves `.grad` unwritten), the returned total is 0.0 -- the reference computes no norm then either -- and the norm launches return
    before they read a gradient; with a fuse_scaler() scaler they still walk the rows, for the scaler's inf flag.

        vbg.optim.clip_in_step([optimizer_cnn, optimizer_bert], clip_norm, when=(train_loss.detach(), loss_clip_tresh))

    Several ranks: the gate reads the tensor it is given and nothing else.  Where every rank must take the same decision, hand in a loss
    that was all-reduced with MAX on the device queue (`dist.all_reduce(loss, op=dist.ReduceOp.MAX)` on the NCCL/RCCL group): every
    rank then compares the same number.  clip_in_step itself runs no collective.

    A call with norm_type 2 and no `when` issues `vbg_grad_sumsq_seg[_inf]` and `vbg_clip_coef` as before; any other call issues
    `vbg_grad_norm_seg` once per optimizer and one `vbg_clip_coef_gate`."""
    optimizers = list(optimizers)
    if not optimizers:
        raise ValueError("clip_in_step: no optimizers")
    kind = _NORM_KINDS.get(float(norm_type)) if isinstance(norm_type, (int, float)) and not isinstance(norm_type, bool) else None
    if kind is None:
        raise ValueError(f"clip_in_step: norm_type is 2, 1 or float('inf'), not {norm_type!r}")
    work = []
    for o in optimizers:
        if not isinstance(o, (_FlatOptimizer, _FusedStock)):
            raise TypeError("clip_in_step takes FusedSGD / FusedAdamW and optimizers made by fuse(), not " + type(o).__qualname__)
        if getattr(o, "_vbg_clip", None) is not None:
            raise RuntimeError("clip_in_step: a clip coefficient is still pending on an optimizer (step() consumes it, zero_grad() drops it)")
        if isinstance(o, _FlatOptimizer):
            work.append((o, o.group, o._clip_table()))
            continue
        try:
            work.append((o, *o._vbg_norm_table()))
        except _NoGradients:
            pass          # (nothing to count; its step will fall back, with nothing to multiply)
        except _Fallback as e:
            raise RuntimeError(f"clip_in_step: the gradients of a fuse()d optimizer are not one flat buffer ({e})") from None
    if not work:
        raise RuntimeError("clip_in_step: no listed optimizer has a gradient")
    dev = work[0][1].gflat.device
    if any(g.gflat.device != dev for _, g, _ in work):
        raise ValueError("clip_in_step: the optimizers' flat buffers live on more than one device")
    grad_scale = None
    if scaler is not None and scaler.is_enabled():
        from torch.amp.grad_scaler import OptState
        if any(scaler._per_optimizer_states[id(o)]["stage"] is OptState.UNSCALED for o in optimizers):
            raise RuntimeError("clip_in_step(scaler=...) after scaler.unscale_(optimizer): the gradients are unscaled already, leave scaler out")
        grad_scale = scaler._scale
        if grad_scale is None:
            raise RuntimeError("clip_in_step(scaler=...): the scaler has not scaled a loss yet")
    gate = _clip_gate(when, dev)
    n = sum(t.n for _, _, t in work)
    partials = _CLIP_PARTIALS.get(dev)
    if partials is None or partials.numel() < n:
        partials = _CLIP_PARTIALS[dev] = torch.empty((max(n, 1024),), device=dev, dtype=torch.float32)
    # a fuse_scaler()ed scaler: its inf check rides in the norm launches, one flag per optimizer (torch skips per optimizer: a joint flag
    # would skip an optimizer whose own gradients are finite), fresh for this call
    flags = torch.zeros((len(work),), device=dev, dtype=torch.float32).unbind(0) if grad_scale is not None and isinstance(scaler, _FusedScaler) else None
    at = 0
    plain = kind == 2 and gate is None          # the L2 entries without a gate: vbg_grad_sumsq_seg[_inf] / vbg_clip_coef
    for j, (_, g, t) in enumerate(work):
        if not plain:
            ops.grad_norm_seg(g.gflat, t, partials[at:at + t.n], kind, None if flags is None else flags[j], gate)
        elif flags is None:
            ops.grad_sumsq_seg(g.gflat, t, partials[at:at + t.n])
        else:
            ops.grad_sumsq_seg_inf(g.gflat, t, partials[at:at + t.n], flags[j])
        at += t.n
    if plain:
        out = ops.clip_coef(partials, n, max_norm, norm_scale, grad_scale)
    else:
        out = ops.clip_coef_gate(partials, n, max_norm, norm_scale, grad_scale, kind, gate)
    coef = out[1:2]
    for o in optimizers:
        o._vbg_clip = coef
    if flags is not None:
        # kept beside GradScaler's own per-optimizer record, which update() discards, and with the coefficient of this call: the flag
        # speaks for the gradients that coefficient was computed from, and for no others (_FusedScaler._check_inf_per_device)
        for j, (o, _, _) in enumerate(work):
            scaler._per_optimizer_states[id(o)][_CLIP_FLAG] = (flags[j], coef)
    return out[0]


# ---- torch.amp.GradScaler on the fused kernels ---------------------------------------------------------------------------------
_CLIP_FLAG = "_vbg_clip_found_inf"          # key of clip_in_step's (flag, coefficient) in GradScaler._per_optimizer_states[id(optimizer)]


class _ScalerState:
    """what fuse_scaler() keeps on the scaler instance (`_vbg_fused`)"""

    def __init__(self):
        self.launches = 0          # inf checks / unscale passes that were one vbg_grad_unscale_check_seg launch
        self.reused = 0            # inf checks that launched nothing: clip_in_step's norm pass had left the flag
        self.fallbacks = 0         # passes that went to torch's own _unscale_grads_
        self.last_fallback = None


def _scaler_target(optimizer):
    """(FlatGroup, chunk table) of the gradients GradScaler would visit on `optimizer`, when they are one flat buffer"""
    if isinstance(optimizer, _FusedStock):
        return optimizer._vbg_norm_table()          # (the table clip_in_step uses: the rows of the parameters with a gradient)
    if isinstance(optimizer, _FlatOptimizer):
        g = optimizer.group
        if not g.valid():
            raise _Fallback("the parameters moved away from their flat buffer (Module.to / a fresh .data)")
        # (a parameter without a gradient keeps its zeroed slot of the buffer, which the step reads with the rest)
        if any(p.grad is not None and p.grad is not gv for p, gv in zip(g.params, g.gviews)):
            raise _Fallback("a .grad is not the flat gradient view (sparse, replaced or cast)")
        return g, optimizer._clip_table()
    raise _Fallback("not a fuse()d torch.optim optimizer, FusedSGD or FusedAdamW")


class _FusedScaler:
    """the two methods of the classes fuse_scaler() switches a GradScaler instance to.  Everything else -- scale(), step(), unscale_(),
    update(), the scale and its growth tracker, state_dict() -- is torch's."""

    def _unscale_grads_(self, optimizer, inv_scale, found_inf, allow_fp16):
        """torch's pass (a Python loop over every parameter, a multi-tensor launch per device and dtype) as ONE launch over the chunk
        table of the optimizer's flat gradient buffer.  Both of torch's callers land here: unscale_ with the real inverse scale,
        _check_inf_per_device with 1.0, which makes the launch read-only"""
        fs = self._vbg_fused
        try:
            group, table = _scaler_target(optimizer)
            dev = group.gflat.device
            for t in (inv_scale, found_inf):
                if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.numel() != 1 or t.device != dev:
                    raise _Fallback("inv_scale / found_inf is not one fp32 element on the flat buffers' device")
        except _Fallback as e:
            fs.fallbacks += 1
            fs.last_fallback = str(e)
            return super()._unscale_grads_(optimizer, inv_scale, found_inf, allow_fp16)
        ops.grad_unscale_check_seg(group.gflat, table, inv_scale, found_inf)
        fs.launches += 1
        return {found_inf.device: found_inf}

    def _check_inf_per_device(self, optimizer):
        """the inf check of `scaler.step(optimizer)` under the `_step_supports_amp_scaling` protocol: nothing to launch when
        clip_in_step(scaler=self) read these very gradients for the norm -- its coefficient is still pending on the optimizer -- and
        left the flag"""
        state = self._per_optimizer_states[id(optimizer)]
        left = state.pop(_CLIP_FLAG, None)
        if left is not None and left[1] is getattr(optimizer, "_vbg_clip", None):
            self._vbg_fused.reused += 1
            state["found_inf_per_device"] = {left[0].device: left[0]}
            return state["found_inf_per_device"]
        return super()._check_inf_per_device(optimizer)


class _FusedGradScaler(_FusedScaler, torch.amp.GradScaler):
    pass


class _FusedCudaGradScaler(_FusedScaler, torch.cuda.amp.GradScaler):
    pass


_SCALERS = {torch.amp.GradScaler: _FusedGradScaler, torch.cuda.amp.GradScaler: _FusedCudaGradScaler}


def fuse_scaler(scaler):
    """Make a torch.amp.GradScaler (or the torch.cuda.amp.GradScaler the reference constructs, train_SROIE.py) run its pass over the
    gradients -- the inf check of every `scaler.step(optimizer)`, the unscale of `scaler.unscale_(optimizer)` -- as ONE HIP launch per
    optimizer (`vbg_grad_unscale_check_seg`) instead of a Python loop over every parameter and several multi-tensor launches.  Returns
    the SAME object, its class switched to a subclass that overrides two private methods; the scale, the growth tracker, update(),
    state_dict() and every public method stay torch's:

        scaler = vbg.optim.fuse_scaler(torch.cuda.amp.GradScaler(enabled=amp))

    The launch serves fuse()d torch.optim optimizers whose present gradients are the flat views of one group (the check-only call of the
    `amp_scaling=True` protocol reads the gradients, 4 B per element, and writes nothing) and FusedSGD / FusedAdamW (the generic route:
    gradients times the inverse scale, stored back).  After `clip_in_step(optimizers, max_norm, scaler=scaler)` the check of
    `scaler.step(optimizer)` launches nothing at all: the norm pass has tested every element it read (`vbg_grad_sumsq_seg_inf`) and left
    one flag per optimizer.  Everything else goes to torch's own pass for that call: an optimizer of any other class, parameters that
    are not homed (yet) or moved away, a `.grad` that is not the flat view, no gradient at all, a scaler on another device than the
    buffers.  `scaler._vbg_fused` counts `launches`, `reused` and `fallbacks` and keeps the reason of the last one."""
    cls = type(scaler)
    if cls not in _SCALERS:
        raise ValueError(f"fuse_scaler() takes instances of exactly torch.amp.GradScaler or torch.cuda.amp.GradScaler, not "
                         f"{cls.__module__}.{cls.__qualname__}")
    scaler.__class__ = _SCALERS[cls]
    scaler._vbg_fused = _ScalerState()
    return scaler


# ---- weight averaging over the flat storage ------------------------------------------------------------------------------------
class WeightAverage:
    """An exponential moving average (kind="ema") or an equal-weight average (kind="swa") of a model's trainable parameters, kept
    as ONE more flat buffer per FlatGroup -- what torch.optim.swa_utils.AveragedModel keeps as a deep copy of the whole model:

        avg = vbg.optim.WeightAverage(model, kind="ema", decay=0.999)
        ...
        optimizer_cnn.step(); optimizer_bert.step()      # torch.optim, fuse()d, FusedSGD / FusedAdamW, scaler.step(...)
        avg.update()                                      # one vbg_lerp per flat group; the first one copies
        ...
        with avg.applied():                               # averaged weights in the model, the live ones parked in the shadow
            validate(model, ...)
        torch.save({"model": avg.averaged_state_dict(), ...}, path)

    Binding happens at the first update() (or load_state_dict()): the groups are those the model's trainable parameters live in
    (`p._vbg_flat`; the model homes them at its first training forward).  A trainable parameter that has a gradient but no flat home
    (VBG_HOME=0) raises ValueError -- there is no per-parameter route; parameters kept out of the buffers (`pooler.*`, `resnet.fc.*`,
    frozen ones) never change, are their own average and are left alone.  A group whose parameters moved away since (Module.to, a
    fresh `.data`) raises RuntimeError at the next update() / swap().

    Counting is AveragedModel's: `n_averaged` is a host integer, the update at n_averaged == 0 copies the whole buffer, later ones are
    avg <- lerp(avg, p, w) over [0, total) in torch's bits, with w = 1 - decay (ema; `decay`: a float in [0, 1] or a callable
    n_averaged -> decay) or w = 1 / (n_averaged + 1) (swa).  Of the update() calls, numbered from 1, call c averages when c > start and
    (c - start) % every == 0; the others return at once.  A step GradScaler skipped needs nothing special: the average moves toward
    unchanged weights, as AveragedModel's does.

    buffers="live" (torch's use_buffers=False): only parameters are averaged; BatchNorm statistics stay the live model's.
    buffers="average": the model's floating-point buffers are averaged too (torch._foreach_lerp_ over private clones -- plumbing) and
    exchanged along with the parameters; integer buffers stay live.

    swap() exchanges live and averaged weights in place (vbg_swap, no second model) and invalidates every cached weight image;
    applied() is the context manager around two of them.  While applied, update() and a nested applied() raise RuntimeError;
    stepping an optimizer while applied is an error this class does not detect (the step would train the average).
    Data parallel: after the all-reduce every rank steps identical gradients, so every rank's average is identical; no collective is
    added."""

    def __init__(self, model: torch.nn.Module, kind: str = "ema", decay=0.999, every: int = 1, start: int = 0, buffers: str = "live"):
        if kind not in ("ema", "swa"):
            raise ValueError(f"kind={kind!r}: 'ema' or 'swa'")
        if buffers not in ("live", "average"):
            raise ValueError(f"buffers={buffers!r}: 'live' or 'average'")
        if kind == "ema" and not callable(decay) and not 0.0 <= float(decay) <= 1.0:
            raise ValueError(f"decay={decay!r}: a float in [0, 1] or a callable n_averaged -> decay")
        if int(every) < 1 or int(start) < 0:
            raise ValueError("every >= 1 and start >= 0")
        self.model, self.kind, self.buffers = model, kind, buffers
        self.decay = decay if callable(decay) else float(decay)
        self.every, self.start = int(every), int(start)
        self.n_averaged, self.calls = 0, 0
        self.is_applied = False
        self.groups: List[FlatGroup] = None
        self.shadows: List[torch.Tensor] = None
        self._buf_names, self._buf_avg = [], []

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
                    raise ValueError(f"WeightAverage: parameter {name} is trained but does not live in flat storage (VBG_HOME=0, or no training "
                                     "forward on the device yet); there is no per-parameter route here -- use "
                                     "torch.optim.swa_utils.AveragedModel for such a model")
                continue
            if all(g is not h for h in groups):
                groups.append(g)
        if not groups:
            raise ValueError("WeightAverage: no parameter of the model lives in flat storage yet (the model homes its parameters at its "
                             "first training forward on the device); without flat storage use torch.optim.swa_utils.AveragedModel")
        self.groups = groups
        self._check_valid()
        self.shadows = [torch.empty_like(g.pflat) for g in groups]
        if self.buffers == "average":
            named = [(n, b) for n, b in self.model.named_buffers() if b.is_floating_point()]
            self._buf_names = [n for n, _ in named]
            self._buf_avg = [b.detach().clone() for _, b in named]

    def _check_valid(self):
        for g in self.groups:
            if not g.valid():
                raise RuntimeError("WeightAverage: the parameters moved away from the flat buffer this average is bound to (Module.to / a "
                                   "fresh .data); build a new WeightAverage after moving the model")

    def _live_buffers(self):
        have = dict(self.model.named_buffers())
        return [have[n] for n in self._buf_names]

    def _names(self):
        """id(parameter) -> the model's name for it"""
        return {id(p): n for n, p in self.model.named_parameters()}

    # ---- the average ----------------------------------------------------------------------------------------------------------
    def weight(self) -> float:
        """the lerp weight of the next averaging update (n_averaged >= 1), in Python double as torch forms it"""
        if self.kind == "swa":
            return 1.0 / (self.n_averaged + 1)
        d = self.decay(self.n_averaged) if callable(self.decay) else self.decay
        return 1.0 - float(d)

    @torch.no_grad()
    def update(self):
        if self.is_applied:
            raise RuntimeError("WeightAverage.update() while the averaged weights are applied: the model holds the average, not the live weights")
        self.calls += 1
        if self.calls <= self.start or (self.calls - self.start) % self.every:
            return
        self._bind()
        self._check_valid()
        if self.n_averaged == 0:
            # (a plain copy, as AveragedModel's first update: a lerp with weight 1 is not exact)
            for g, s in zip(self.groups, self.shadows):
                s.copy_(g.pflat)
            if self._buf_avg:
                torch._foreach_copy_(self._buf_avg, self._live_buffers())
        else:
            w = self.weight()
            for g, s in zip(self.groups, self.shadows):
                ops.lerp_(s, g.pflat, w)          # padding included: both sides hold the same zeros there
            if self._buf_avg:
                torch._foreach_lerp_(self._buf_avg, self._live_buffers(), w)
        self.n_averaged += 1

    def _invalidate(self):
        for g in self.groups:
            g.invalidate()
        ops.bump_weight_epoch()

    def _need_average(self, what):
        if self.groups is None or self.n_averaged == 0:
            raise RuntimeError(f"WeightAverage.{what}: nothing has been averaged yet (no update() past `start`)")
        self._check_valid()

    @torch.no_grad()
    def swap(self):
        """exchange the live and the averaged weights in place, and tell every cache of a weight image; toggles `is_applied`"""
        self._need_average("swap()")
        for g, s in zip(self.groups, self.shadows):
            ops.swap_(g.pflat, s)
        if self._buf_avg:
            live = self._live_buffers()
            tmp = [b.detach().clone() for b in live]
            torch._foreach_copy_(live, self._buf_avg)
            torch._foreach_copy_(self._buf_avg, tmp)
        self._invalidate()
        self.is_applied = not self.is_applied

    @contextlib.contextmanager
    def applied(self):
        """with avg.applied(): the model computes with the averaged weights; the live ones come back on exit, also on an exception"""
        if self.is_applied:
            raise RuntimeError("WeightAverage.applied(): the averaged weights are applied already")
        self.swap()
        try:
            yield self
        finally:
            self.swap()

    @torch.no_grad()
    def copy_to(self):
        """the averaged weights become the live weights (a copy; the average stays what it is)"""
        if self.is_applied:
            raise RuntimeError("WeightAverage.copy_to() while the averaged weights are applied")
        self._need_average("copy_to()")
        for g, s in zip(self.groups, self.shadows):
            g.pflat.copy_(s)
        if self._buf_avg:
            torch._foreach_copy_(self._live_buffers(), self._buf_avg)
        self._invalidate()

    # ---- checkpoints ----------------------------------------------------------------------------------------------------------
    def _avg_flats(self):
        """the flat buffers that hold the average right now (while applied: the model's own)"""
        return [g.pflat for g in self.groups] if self.is_applied else self.shadows

    def _avg_buffers(self):
        return self._live_buffers() if self.is_applied else self._buf_avg

    @torch.no_grad()
    def averaged_state_dict(self):
        """model.state_dict() with the averaged weights: same keys and layouts (channels_last kept, doubly registered tensors under both
        keys); every tensor that is a view of a flat group is replaced by a clone of the same view of the average, averaged buffers
        (buffers="average") by clones of theirs, everything else is the model's.  Nothing is swapped, the model is not disturbed."""
        self._need_average("averaged_state_dict()")
        where = {}
        for g, flat in zip(self.groups, self._avg_flats()):
            for i, a in enumerate(g._ptrs):
                where[a] = (g, flat, i)
        bufs = dict(zip(self._buf_names, self._avg_buffers()))
        sd = self.model.state_dict()
        out = sd.copy()                                    # (keys in the model's order; `_metadata` carried over below)
        if hasattr(sd, "_metadata"):
            out._metadata = sd._metadata
        done = {}
        for k, t in sd.items():
            hit = where.get(t.data_ptr()) if isinstance(t, torch.Tensor) and t.is_floating_point() else None
            if hit is not None and hit[0].params[hit[2]].numel() == t.numel():
                key = (id(hit[0]), hit[2])
                if key not in done:
                    done[key] = hit[0].view(hit[1], hit[2]).clone()
                out[k] = done[key]
            elif k in bufs:
                out[k] = bufs[k].clone()
        return out

    @torch.no_grad()
    def state_dict(self):
        """counters, settings and the average as per-parameter tensors keyed by parameter name (no dependence on the flat layout)"""
        sd = {"n_averaged": self.n_averaged, "calls": self.calls, "kind": self.kind, "every": self.every, "start": self.start,
              "buffers": self.buffers, "shadow": {}, "shadow_buffers": {}}
        if not callable(self.decay):
            sd["decay"] = self.decay
        if self.groups is not None and self.n_averaged > 0:
            names = self._names()
            for g, flat in zip(self.groups, self._avg_flats()):
                for i, p in enumerate(g.params):
                    sd["shadow"][names[id(p)]] = g.view(flat, i).clone()
            sd["shadow_buffers"] = {n: b.clone() for n, b in zip(self._buf_names, self._avg_buffers())}
        return sd

    @torch.no_grad()
    def load_state_dict(self, sd):
        if self.is_applied:
            raise RuntimeError("WeightAverage.load_state_dict() while the averaged weights are applied")
        if sd["kind"] != self.kind or sd.get("buffers", "live") != self.buffers:
            raise ValueError(f"checkpoint of a kind={sd['kind']!r}, buffers={sd.get('buffers', 'live')!r} average; this one is "
                             f"kind={self.kind!r}, buffers={self.buffers!r}")
        self._bind()
        self._check_valid()
        if int(sd["n_averaged"]) > 0:
            names = self._names()
            want = {names[id(p)] for g in self.groups for p in g.params}
            if set(sd["shadow"]) != want:
                odd = sorted(set(sd["shadow"]) ^ want)
                raise ValueError(f"checkpoint and model disagree on the averaged parameters: {odd[:4]}{'...' if len(odd) > 4 else ''}")
            if set(sd["shadow_buffers"]) != set(self._buf_names):
                raise ValueError("checkpoint and model disagree on the averaged buffers")
            for g, s in zip(self.groups, self.shadows):
                s.zero_()                                  # (the padding between slots, as in the parameter buffer)
                for i, p in enumerate(g.params):
                    g.view(s, i).copy_(sd["shadow"][names[id(p)]])
            for n, b in zip(self._buf_names, self._buf_avg):
                b.copy_(sd["shadow_buffers"][n])
        self.n_averaged, self.calls = int(sd["n_averaged"]), int(sd["calls"])
        self.every, self.start = int(sd["every"]), int(sd["start"])
        if "decay" in sd and not callable(self.decay):
            self.decay = float(sd["decay"])


class FlatReducer:
    """Bucketed, overlapped gradient all-reduce over the flat buffers (replaces DistributedDataParallel's reducer,
    train_SROIE.py:206-210).

    Ordering contract (what keeps N ranks from ever pairing different buffers): bucket collectives are issued in ONE fixed
    sequence `self.order`, bucket `order[k]` only after `order[0..k-1]` have been issued; whatever has not completed by the end
    of backward is flushed by `finish()` in the same sequence.  Step 1 launches nothing during backward: it records the order
    in which this rank's buckets completed; `finish()` then takes rank 0's record as the sequence for every rank (one
    broadcast) -- from step 2 on the buckets fire during backward.  A rank whose graph skips a sub-module in some step simply
    issues the affected bucket (and everything behind it) from `finish()`; the sequence is unchanged."""

    def __init__(self, optimizers, bucket_mb: float = 32.0, group=None, sync_bn_group="auto", serialize_syncbn=None, overlap=None,
                 dry_run=False, force_enable=None, static_graph=None):
        """force_enable (VBG_FORCE_REDUCER=1): run the whole machinery -- hooks, rank-agreed sequence, collectives issued from the staging
        stream, work.wait(), SyncBatchNorm statistics on the communicator -- on a process group of ONE rank as well (every collective is an
        identity there): the one-GPU check of the real backend (ProcessGroupNCCL = RCCL) before a multi-GPU node sees this code.
        static_graph: the caller's word that every rank runs the same autograd graph every step (classifier_mode simp / crf with every
        sub-module used).  With SyncBatchNorm statistics on the buckets' communicator AND overlap, a bucket that one rank issues from
        finish() while the others issue it inside backward sits at a different place among the statistics collectives -- mismatched
        collectives on one communicator.  So on a shared communicator the buckets only leave from inside backward when
        static_graph=True; without that word every bucket is issued from finish(), a rank-invariant point for ANY graph (the overlap is
        what is given up; `sync_bn_group="new"` keeps it for rank-varying graphs on a second communicator).  A rank that asserted
        static_graph=True and then has to flush a bucket from finish() after step 1 raises instead of risking a silent mismatch.
        dry_run (one process): same buckets, same hooks and the same launch sequence, but a bucket's "collective" is a timestamp on
        the stream it would be issued from -- `timeline()` then tells when, inside backward, every bucket could have left
        (tools/bucket_timeline.py)"""
        self.dry = bool(dry_run)
        if force_enable is None:
            force_enable = os.environ.get("VBG_FORCE_REDUCER", "0") != "0"
        self.forced = bool(force_enable) and dist.is_available() and dist.is_initialized() and dist.get_world_size(group) == 1
        self.enabled = dist.is_available() and dist.is_initialized() and (dist.get_world_size(group) > 1 or self.forced)
        if static_graph is None and os.environ.get("VBG_STATIC_GRAPH") is not None:
            static_graph = os.environ["VBG_STATIC_GRAPH"] != "0"
        self.static_graph = static_graph
        self.pg = group
        self.optimizers = optimizers
        self.world = dist.get_world_size(group) if self.enabled else 1
        self.buckets = []          # [tensor view, member count, pending count]
        self.handles = []          # (bucket index, work) of the collectives in flight
        self.bucket_of = {}        # id(param) -> bucket index
        self._reported = set()     # sunk parameters already counted this step
        self.order = None          # the agreed launch sequence (bucket indices); None until the first finish()
        self._observed = []        # completion order seen in the current step
        self._complete = set()
        self._next = 0             # position in `order` of the next bucket to issue
        self._stage = None         # stream the collectives are issued from
        self._streams = {}         # raw handle -> torch stream: compute streams gradients were reported from in this step
        self._events = []          # dry run: (bucket, event) in issue order
        self.steps_done = 0
        self.sync_bn_mode = "none"
        self._phase = "idle"       # what the host is doing, for the watchdog's report
        self._beat = time.monotonic()
        self._watch = None
        self.overlap = (os.environ.get("VBG_DDP_OVERLAP", "1") != "0") if overlap is None else bool(overlap)
        if self.dry:
            self.enabled = False
        elif not self.enabled:
            return
        # SyncBatchNorm statistics and gradient buckets.  The buckets follow ONE rank-agreed sequence, the SyncBatchNorm collectives
        # the program order of forward / backward.  Where the bucket launches fall BETWEEN the SyncBatchNorm collectives is rank-invariant
        # exactly when every rank runs the same autograd graph (classifier_mode simp / crf, every sub-module used every step):
        #   sync_bn_group="default" ("auto" without VBG_SYNCBN_GROUP: THE DEFAULT): statistics and buckets share the reducer's
        #       communicator -- one communicator, one rank-invariant program order of collectives, nothing concurrent.  A statistics
        #       all-reduce queues behind the buckets in flight (a 32 MB bucket: a fraction of a millisecond over xGMI); the encoder's
        #       backward, where most of the gradient bytes leave, contains no BatchNorm.  overlap=False (VBG_DDP_OVERLAP=0) launches every
        #       bucket from finish() instead of from inside backward: the order is then rank-invariant for ANY graph, at the price of
        #       the overlap -- the setting for data-dependent graphs (classifier_mode full) on one communicator;
        #   sync_bn_group="new" (VBG_SYNCBN_GROUP=new; only with group=None -- dist.new_group is a collective over the DEFAULT group,
        #       every rank must construct its reducer): an own communicator for the statistics, collectives of the two communicators
        #       concurrently in flight.  Tolerates rank-varying graphs WITH overlap, but torch documents concurrent collectives on two
        #       NCCL communicators as unsafe when their kernels cannot co-reside: the opt-in A/B, not the default.
        #       serialize_syncbn=True (VBG_SERIALIZE_SYNCBN=1) makes the compute stream wait for the buckets in flight (work.wait() of
        #       every outstanding handle: the collectives run on the backend's own stream) before each statistics collective --
        #       meaningful only with rank-invariant graphs, where the one-communicator default does the same thing for free;
        #   sync_bn_group=<ProcessGroup>: the caller's communicator (required with a sub-group for "new"-style separation).
        if self.dry:
            sync_bn_group = None
        if sync_bn_group == "auto":
            # round 6: the shared communicator is the default again.  The direct communicator has only ever run on a
            # one-rank group, and a second ncclComm_t with collectives in flight beside ProcessGroupNCCL's is the configuration a first
            # N > 1 run should not meet unasked: VBG_SYNCBN_GROUP=direct / sync_bn_group="direct" / bench.py --syncbn-comm direct opt in.
            sync_bn_group = os.environ.get("VBG_SYNCBN_GROUP", "default")
        if Fn.SyncCtx.direct is not None:          # a reducer is being rebuilt: the previous one's communicator goes first
            try:
                Fn.SyncCtx.direct.destroy()
            except Exception:
                pass
        Fn.SyncCtx.direct = None
        if sync_bn_group == "direct":
            # OPT-IN: the statistics on a communicator of this library's own, enqueued on the compute stream (vbg/rccl.py): no event
            # hand-overs to and from ProcessGroupNCCL's stream (measured on one rank: 34.8 vs 35.8 ms per step), and -- the point at
            # N > 1 -- never queued behind a 32 MB gradient bucket on that stream.  Two communicators then have kernels in flight during
            # backward.  That is deadlock-free when every rank ENQUEUES them in the same relative order (streams beyond the device's
            # hardware queues share one, and a collective's kernel parked at the head of a queue holds up whatever sits behind it): the
            # same program on every rank issues the same sequence, which is what static_graph=True asserts -- without it the buckets
            # leave from finish(), behind every statistics collective of the step, as on the shared communicator.
            from . import rccl
            if group is not None or not rccl.available():
                raise ValueError("sync_bn_group='direct' needs backend 'nccl' (RCCL) and the default process group")
            dev = optimizers[0].group.pflat.device
            Fn.SyncCtx.group = group
            comm, err = None, None
            try:
                comm = rccl.DirectComm(dev)
            except Exception as e:
                err = e
            # every rank must end up on the SAME communicator: the ranks agree on success over the default group (a rank-local
            # fallback would leave some ranks on the direct communicator and some on torch.distributed's -- mismatched collectives)
            ok = torch.tensor([0 if comm is None else 1], device=dev, dtype=torch.int32)
            dist.all_reduce(ok, op=dist.ReduceOp.MIN)
            if int(ok.item()) == 1:
                Fn.SyncCtx.direct = comm
                self.sync_bn_mode = "direct RCCL communicator on the compute stream"
            else:
                import sys
                if comm is not None:
                    comm.destroy()
                print(f"[vbg reducer] no direct RCCL communicator on every rank ({'this rank: ' + type(err).__name__ + ': ' + str(err) if err else 'another rank failed'}); "
                      "SyncBatchNorm statistics through torch.distributed on every rank", file=sys.stderr, flush=True)
                sync_bn_group = "default"
        if sync_bn_group == "direct":
            pass
        elif sync_bn_group == "new":
            if group is not None:
                raise ValueError("FlatReducer(group=<sub-group>): pass sync_bn_group=<ProcessGroup> or 'default' -- dist.new_group is a "
                                 "collective over the default group and would hang when only the sub-group's ranks call it")
            Fn.SyncCtx.group = dist.new_group(ranks=list(range(dist.get_world_size())))
            self.sync_bn_mode = "own communicator"
        elif sync_bn_group == "default":
            Fn.SyncCtx.group = group
            self.sync_bn_mode = "shared communicator"
        elif sync_bn_group is not None:
            Fn.SyncCtx.group = sync_bn_group
            self.sync_bn_mode = "caller's communicator"
        if serialize_syncbn is None:
            serialize_syncbn = os.environ.get("VBG_SERIALIZE_SYNCBN", "0") != "0"
        Fn.SyncCtx.before = self._wait_for_buckets if (serialize_syncbn and not self.dry) else None
        Fn.SyncCtx.seq = 0
        Fn.SyncCtx.force = self.forced
        if self.sync_bn_mode in ("shared communicator", "direct RCCL communicator on the compute stream") and self.overlap and not self.static_graph:
            self.overlap = False       # graphs not known to be rank-invariant: every bucket from finish(), a rank-invariant point
        Fn.GRAD_READY[0] = self._param_ready      # sunk gradients (written by the wgrad kernels) report here
        import weakref
        for o in optimizers:                      # (ViBERTgridNet._overlap_safe: these groups' gradients are collected by a reducer that
            o.group._vbg_reducer = weakref.ref(self)      #  knows about the side streams)
        cap = int(bucket_mb * (1 << 20) / 4)
        for o in optimizers:
            if not self.dry:
                o.grad_scale = 1.0 / self.world
            g = o.group
            start, members = 0, []
            for i, (p, off) in enumerate(zip(g.params, g.offsets)):
                members.append(p)
                end = g.offsets[i + 1] if i + 1 < len(g.params) else g.total
                if end - start >= cap or i + 1 == len(g.params):
                    self._add_bucket(g.gflat[start:end], members)
                    start, members = end, []

    def _add_bucket(self, view, members):
        idx = len(self.buckets)
        self.buckets.append([view, len(members), len(members)])
        for p in members:
            self.bucket_of[id(p)] = idx
            p.register_post_accumulate_grad_hook(lambda _p, idx=idx: self._hook_ready(_p, idx))       # autograd-accumulated gradients

    def _hook_ready(self, p, idx):
        """post-accumulate hook of parameter p.  torch runs these hooks for a parameter whose autograd node handed it no gradient
        as well (every sunk parameter: its Function wrote the gradient into the flat buffer itself, reported it through
        `_param_ready` and returned None), so a parameter is counted ONCE per step whichever way it reports first -- counting both
        let a bucket reach zero when only half of its members were complete, and the bucket's all-reduce then raced the kernels
        that were still writing the rest (the last bucket lost: ranks drifted apart in the stem's parameters)."""
        if id(p) in self._reported:
            return
        self._reported.add(id(p))
        self._ready(idx)

    def _param_ready(self, p):
        """a sunk gradient is complete (each sunk parameter feeds exactly one autograd node per step in this model;
        a repeated report for the same parameter is ignored rather than double-counted)"""
        idx = self.bucket_of.get(id(p))
        if idx is not None and id(p) not in self._reported:
            self._reported.add(id(p))
            self._ready(idx)

    def _note_stream(self, dev):
        """remember the stream a gradient was reported from (hundreds of reports per step: the raw handle is two C calls, the torch
        stream object is only built for a handle not seen yet in this step)"""
        raw = ops.raw_stream(dev)
        if raw not in self._streams:
            self._streams[raw] = torch.cuda.current_stream(dev)

    def _issue(self, idx):
        buf = self.buckets[idx][0]
        if self.dry:               # the moment this bucket's collective could start: everything reported so far has been enqueued
            ev = torch.cuda.Event(enable_timing=True)
            ev.record(torch.cuda.current_stream(buf.device))
            self._events.append((idx, ev))
            return
        if not buf.is_cuda:
            self.handles.append((idx, dist.all_reduce(buf, group=self.pg, async_op=True)))
            return
        # gradients are written on more than one compute stream (the encoder's backward runs on vbg.ops.side_stream): the
        # collective is issued from a staging stream that waits for every stream a gradient was reported from and for the side
        # streams -- the reporting stream itself is not held up
        dev = buf.device
        if self._stage is None:
            self._stage = torch.cuda.Stream(device=dev)
        self._note_stream(dev)
        for s in list(self._streams.values()) + [t for t in ops.side_streams() if t.device == dev]:
            self._stage.wait_stream(s)
        with torch.cuda.stream(self._stage):
            self.handles.append((idx, dist.all_reduce(buf, group=self.pg, async_op=True)))

    def timeline(self, start_event):
        """dry run: [(bucket, MB, ms since start_event)] of the last step, in issue order; clears the record (call after a sync)"""
        out = [(i, self.buckets[i][0].numel() * 4 / 1e6, start_event.elapsed_time(ev)) for i, ev in self._events]
        self._events = []
        return out

    def _wait_for_buckets(self):
        """compute stream waits for the bucket collectives issued so far (serialize_syncbn).  The collectives were issued with
        async_op=True: they run on the BACKEND's stream (ProcessGroupNCCL's own), which the staging stream only joins at work.wait() --
        so the current stream has to wait for the works themselves (waiting for the staging stream alone left the buckets
        free to overlap the statistics collective).  work.wait() on NCCL blocks the current STREAM, not the host; on gloo the host.
        The handles stay listed for finish()."""
        for _, h in self.handles:
            h.wait()

    def _ready(self, idx):
        b = self.buckets[idx]
        if b[0].is_cuda:
            self._note_stream(b[0].device)
        b[2] -= 1
        assert b[2] >= 0, "a gradient was reported twice: the bucket would be reduced before it is complete"
        if b[2] != 0:
            return
        self._observed.append(idx)
        self._complete.add(idx)
        if self.order is None or not self.overlap:
            return
        while self._next < len(self.order) and self.order[self._next] in self._complete:
            self._issue(self.order[self._next])
            self._next += 1

    def finish(self):
        """issue what backward left over (in sequence), wait for every bucket (call after backward, before the optimizer
        steps), re-arm the counters"""
        if self.dry:
            if self.order is None:
                self.order = self._observed + [i for i in range(len(self.buckets)) if i not in self._complete]
            while self._next < len(self.order):
                self._issue(self.order[self._next])
                self._next += 1
            for b in self.buckets:
                b[2] = b[1]
            self._reported.clear()
            self._streams.clear()
            self._observed, self._complete, self._next = [], set(), 0
            return
        if not self.enabled:
            return
        self._phase, self._beat = "finish", time.monotonic()
        if self.order is None:
            seen = self._observed + [i for i in range(len(self.buckets)) if i not in self._complete]
            t = torch.tensor(seen, dtype=torch.int64, device=self.buckets[0][0].device)
            dist.broadcast(t, src=dist.get_global_rank(self.pg, 0) if self.pg is not None else 0, group=self.pg)
            self.order = [int(i) for i in t.tolist()]
            assert sorted(self.order) == list(range(len(self.buckets)))
        late = 0
        while self._next < len(self.order):        # a parameter got no gradient this step (zero rows): reduce what is there
            self._issue(self.order[self._next])
            self._next += 1
            late += 1
        for _, h in self.handles:
            h.wait()
        if (late and self.overlap and self.static_graph and self.sync_bn_mode != "own communicator" and self.sync_bn_mode != "none" and self.steps_done >= 1
                and Fn.SyncCtx.seq > 0 and not self.forced):
            raise RuntimeError(f"vbg.optim.FlatReducer(static_graph=True): {late} gradient bucket(s) had to be issued from finish() in step "
                               f"{self.steps_done + 1} -- this rank's autograd graph skipped a sub-module, so its collectives did not interleave "
                               "with the SyncBatchNorm statistics the way the other ranks' did.  Build the reducer with static_graph=False "
                               "(buckets after backward) or sync_bn_group='new' (own communicator for the statistics).")
        self.handles = []
        for b in self.buckets:
            b[2] = b[1]
        self._reported.clear()
        self._streams.clear()
        self._observed, self._complete, self._next = [], set(), 0
        self.steps_done += 1
        self._phase, self._beat = "between steps", time.monotonic()

    # ------------------------------------------------------------------------------------------------------------------------
    def describe_pending(self) -> str:
        """one line for a hang report: which bucket / which SyncBatchNorm collective this rank is at"""
        rank = dist.get_rank() if dist.is_initialized() else 0
        pend = []
        for idx, h in self.handles:
            try:
                done = h.is_completed()
            except Exception:
                done = None
            if not done:
                pend.append(idx)
        nxt = self.order[self._next] if (self.order is not None and self._next < len(self.order)) else None
        waiting = [i for i in range(len(self.buckets)) if self.buckets[i][2] > 0]
        return (f"[vbg reducer] rank {rank}: step {self.steps_done} ({self._phase}), {self.sync_bn_mode if self.enabled else 'disabled'}, "
                f"overlap {'on' if self.overlap else 'off'}; buckets issued {self._next}/{len(self.buckets)}, in flight {pend}, next in sequence {nxt}, "
                f"still collecting gradients {waiting[:8]}{'...' if len(waiting) > 8 else ''}; SyncBatchNorm collectives issued so far "
                f"{getattr(Fn.SyncCtx, 'seq', 0)} (last: {getattr(Fn.SyncCtx, 'last', None)})")

    def start_watchdog(self, seconds: float, exit_code=None):
        """daemon thread: when no step completes for `seconds`, print `describe_pending()` to stderr (once per stall) so that a hung
        collective leaves a diagnostic instead of an empty record; exit_code != None then ends the process"""
        import sys
        import threading

        def run():
            reported = -1
            while True:
                time.sleep(min(5.0, seconds / 4))
                if time.monotonic() - self._beat > seconds and reported != self.steps_done:
                    reported = self.steps_done
                    print(self.describe_pending() + f" -- no progress for {seconds:.0f} s", file=sys.stderr, flush=True)
                    if exit_code is not None:
                        os._exit(exit_code)

        self._watch = threading.Thread(target=run, daemon=True, name="vbg-reducer-watchdog")
        self._watch.start()
