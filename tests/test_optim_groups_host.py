"""Param groups of the fused optimizers, the host side (no GPU, no step taken; the library itself must load): the run table and the
chunk table over a flat layout whose groups interleave, torch's `param_groups`, what construction refuses, the dispatch between
the whole-range and the segmented entries, checkpoint indices against torch.optim, and the argument checks / struct sizes of
vbg_sgd_step_seg / vbg_adamw_step_seg."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# six parameters in the order the flat buffers hold them (vbg.optim._fusion_order: the REVERSE of registration), with their param
# group: "weight" / "scale" tensors decay (A), "bias" / "LayerNorm.weight" tensors do not (B) -- A B A A B A
LAYOUT = [("head.scale", (1,), "A"), ("head.bias", (13,), "B"), ("head.weight", (37, 5), "A"), ("mid.weight", (3, 64), "A"),
          ("mid.LayerNorm.weight", (8,), "B"), ("stem.weight", (130, 33), "A")]
# slots are padded to 8 elements: 8, 16, 192, 192, 8, 4296 -> offsets 0, 8, 24, 216, 408, 416; the last slot ends at 4712, and the
# buffer is rounded up to 32: 4736
OFFSETS, END, TOTAL = [0, 8, 24, 216, 408, 416], 4712, 4736
RUNS = [(0, 8, 0), (8, 16, 1), (24, 384, 0), (408, 8, 1), (416, 4296, 0)]          # the two adjacent A slots merged
CHUNK = 64


def six_params(device, dtype=torch.float32, seed=0):
    """(registration-order [(name, parameter)], {name: group letter}): the list a model would hand over; its flat layout is LAYOUT"""
    g = torch.Generator().manual_seed(seed)
    named = [(n, torch.nn.Parameter(torch.randn(*s, generator=g).to(dtype).to(device))) for n, s, _ in LAYOUT]
    return named[::-1], {n: a for n, _, a in LAYOUT}


def split(named, letters, **b_overrides):
    """[group A dict, group B dict] of a registration-order list"""
    return [{"params": [(n, p) for n, p in named if letters[n] == "A"]},
            {"params": [(n, p) for n, p in named if letters[n] == "B"], **b_overrides}]


def expected_chunks(chunk=CHUNK):
    rows = []
    for start, length, k in RUNS:
        for s in range(start, start + length, chunk):
            rows.append((s, min(chunk, start + length - s), k))
    return np.array(rows, dtype=np.int64)


def test_run_table_and_chunk_table():
    from vbg.optim import FusedAdamW, FusedSGD
    for cls, kw in ((FusedAdamW, {}), (FusedSGD, {"momentum": 0.9})):
        named, letters = six_params("cpu")
        opt = cls(split(named, letters, weight_decay=0.0), "cpu", lr=1e-3, seg_chunk=CHUNK, layout=named, **kw)
        g = opt.group
        assert g.names == [n for n, _, _ in LAYOUT] and g.offsets == OFFSETS and g.total == TOTAL
        assert opt.segmented and opt.runs == RUNS
        rows = opt.chunk_rows
        want = expected_chunks()
        assert rows.shape == (1 + 1 + 6 + 1 + 68, 3) and np.array_equal(rows, want)
        assert tuple(rows[-1]) == (4704, 8, 0)                                       # the 4296-element run: 67 full rows and one of 8
        assert not (rows[:, 0] % 4).any() and not (rows[:, 1] % 4).any()
        assert rows[:, 1].max() == CHUNK and rows[:, 1].min() > 0
        # the rows tile every run exactly, in order, and nothing covers [END, TOTAL)
        covered = np.full(TOTAL, -1)
        for s, n, k in rows:
            assert (covered[s:s + n] == -1).all()
            covered[s:s + n] = k
        for s, n, k in RUNS:
            assert (covered[s:s + n] == k).all()
        assert (covered[:END] >= 0).all() and (covered[END:] == -1).all()
        # the device image: 16-byte rows (long long start, int length, int group)
        t = opt.table
        assert (t.n, t.ngroups, t.numel) == (len(want), 2, TOTAL) and t.rows.dtype == torch.int32 and tuple(t.rows.shape) == (len(want), 4)
        img = t.rows.numpy().view(np.dtype([("start", "<i8"), ("length", "<i4"), ("group", "<i4")])).reshape(-1)
        assert np.array_equal(img["start"], want[:, 0]) and np.array_equal(img["length"], want[:, 1]) and np.array_equal(img["group"], want[:, 2])


def test_default_chunk_length_and_layout_without_a_hint():
    from vbg import optim as vo
    named, letters = six_params("cpu")
    opt = vo.FusedAdamW(vo.decay_groups(named), "cpu", lr=1e-3)                      # decay_groups carries the layout itself
    assert opt.group.names == [n for n, _, _ in LAYOUT] and opt.runs == RUNS
    assert vo.SEG_CHUNK % 4 == 0 and opt.chunk_rows[:, 1].max() <= vo.SEG_CHUNK
    assert np.array_equal(opt.chunk_rows, expected_chunks(vo.SEG_CHUNK))
    assert opt.param_groups[0]["weight_decay"] == 0.01 and opt.param_groups[1]["weight_decay"] == 0.0
    assert [n for n, _ in vo.decay_groups(named)[1]["params"]] == ["mid.LayerNorm.weight", "head.bias"]
    assert vo.decay_groups(named, lr=0.5)[1] == {"params": vo.decay_groups(named)[1]["params"], "lr": 0.5}
    # a hand-built list without a layout: the buffers follow the groups in the order given (reversed, as any list is)
    named2, letters2 = six_params("cpu")
    opt2 = vo.FusedAdamW(split(named2, letters2), "cpu", lr=1e-3)
    assert opt2.group.names == ["head.bias", "mid.LayerNorm.weight", "head.scale", "head.weight", "mid.weight", "stem.weight"]
    assert opt2.runs == [(0, 24, 1), (24, 8 + 192 + 192 + 4296, 0)]
    named3, letters3 = six_params("cpu")
    with pytest.raises(ValueError):
        vo.FusedAdamW(split(named3, letters3), "cpu", lr=1e-3, layout=named3[:-1])


def test_an_already_homed_group_is_adopted():
    from vbg.optim import FlatGroup, FusedSGD
    named, letters = six_params("cpu")
    home = FlatGroup(named, "cpu")                                                   # what the model's first training forward does
    opt = FusedSGD(split(named, letters, lr=0.5), "cpu", lr=0.1, momentum=0.9, seg_chunk=CHUNK)
    assert opt.group is home and opt.runs == RUNS and np.array_equal(opt.chunk_rows, expected_chunks())


def test_param_groups_are_torch_param_groups():
    from vbg.optim import FusedAdamW, FusedSGD
    named, letters = six_params("cpu")
    opt = FusedAdamW(split(named, letters, weight_decay=0.0, lr=3e-4, betas=(0.8, 0.99)), "cpu", lr=1e-3, eps=1e-6, layout=named)
    a, b = opt.param_groups
    assert len(opt.param_groups) == 2
    assert [p.shape for p in a["params"]] == [torch.Size(s) for _, s, k in LAYOUT[::-1] if k == "A"]
    assert [p.shape for p in b["params"]] == [torch.Size(s) for _, s, k in LAYOUT[::-1] if k == "B"]
    twin = torch.optim.AdamW([{"params": a["params"]}, {"params": b["params"], "weight_decay": 0.0, "lr": 3e-4, "betas": (0.8, 0.99)}], lr=1e-3, eps=1e-6)
    for mine, ref in zip(opt.param_groups, twin.param_groups):
        assert set(mine) == set(ref)
        assert {k: v for k, v in mine.items() if k != "params"} == {k: v for k, v in ref.items() if k != "params"}
    assert (a["lr"], a["weight_decay"], a["betas"], a["eps"]) == (1e-3, 0.01, (0.9, 0.999), 1e-6)          # defaults filled in
    assert (b["lr"], b["weight_decay"], b["betas"], b["eps"]) == (3e-4, 0.0, (0.8, 0.99), 1e-6)
    # schedulers work per group
    sched = torch.optim.lr_scheduler.LambdaLR(opt, [lambda e: 0.5 ** e, lambda e: 1.0 / (1 + e)])
    sched.step()
    assert abs(a["lr"] - 0.5e-3) < 1e-15 and abs(b["lr"] - 1.5e-4) < 1e-15
    named, letters = six_params("cpu")
    s = FusedSGD(split(named, letters, momentum=0.5), "cpu", lr=0.1, momentum=0.9, weight_decay=0.005)
    assert [(g["lr"], g["momentum"], g["weight_decay"], g["dampening"], g["nesterov"]) for g in s.param_groups] == \
        [(0.1, 0.9, 0.005, 0, False), (0.1, 0.5, 0.005, 0, False)]


def test_construction_errors():
    from vbg.optim import FusedAdamW, FusedSGD
    named, letters = six_params("cpu")
    a, b = split(named, letters)
    with pytest.raises(ValueError):                                                  # a parameter in two groups
        FusedAdamW([a, {"params": b["params"] + a["params"][:1]}], "cpu", lr=1e-3)
    with pytest.raises(ValueError):                                                  # an empty group
        FusedAdamW([a, b, {"params": []}], "cpu", lr=1e-3)
    many = [(f"p{i}", torch.nn.Parameter(torch.zeros(3))) for i in range(33)]
    with pytest.raises(ValueError):                                                  # 33 groups
        FusedSGD([{"params": [np_]} for np_ in many], "cpu", lr=0.1)
    assert all(not hasattr(p, "_vbg_flat") for p in [p for _, p in named] + [p for _, p in many])          # refused before anything was homed
    FusedSGD([{"params": [np_]} for np_ in many[:32]], "cpu", lr=0.1)                # 32 are fine
    for cls, bad in ((FusedSGD, {"nesterov": True}), (FusedSGD, {"dampening": 0.1}), (FusedSGD, {"maximize": True}),
                     (FusedAdamW, {"amsgrad": True}), (FusedAdamW, {"maximize": True})):
        named, letters = six_params("cpu")
        kw = {"momentum": 0.9} if cls is FusedSGD else {}
        with pytest.raises(ValueError):
            cls(split(named, letters, **bad), "cpu", lr=1e-3, **kw)
        with pytest.raises(ValueError):                                              # the one-dict list is a created group too
            cls([{"params": named, **bad}], "cpu", lr=1e-3, **kw)
    named, letters = six_params("cpu")
    for opt in (FusedAdamW(split(named, letters), "cpu", lr=1e-3), FusedSGD([(f"q{i}", torch.nn.Parameter(torch.zeros(3))) for i in range(2)], "cpu", lr=0.1)):
        with pytest.raises(NotImplementedError, match="constructor"):
            opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(2))]})
        assert len(opt.param_groups) == (2 if opt.segmented else 1)


@pytest.mark.parametrize("which", ["sgd", "adamw"])
def test_one_group_takes_the_whole_range_entry(which, monkeypatch):
    """the single list and a list of one dict: identical state, and step() calls the old entry (the dispatch decision is checked with
    the entries replaced by recorders: no launch)"""
    from vbg import ops
    from vbg.optim import FusedAdamW, FusedSGD
    cls, kw = (FusedSGD, {"momentum": 0.9, "weight_decay": 0.005}) if which == "sgd" else (FusedAdamW, {"weight_decay": 0.02})
    calls = []
    for name in ("sgd_step", "adamw_step", "sgd_step_seg", "adamw_step_seg"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: calls.append((_n, a)))
    n1, _ = six_params("cpu")
    n2, _ = six_params("cpu")
    n3, l3 = six_params("cpu")
    one = cls(n1, "cpu", lr=1e-3, **kw)
    dict1 = cls([{"params": n2}], "cpu", lr=1e-3, **kw)
    two = cls(split(n3, l3), "cpu", lr=1e-3, layout=n3, **kw)
    assert not one.segmented and not dict1.segmented and two.segmented
    assert one.table is None and dict1.table is None and one.runs is None
    assert one.group.names == dict1.group.names == two.group.names and one.group.offsets == dict1.group.offsets and one.group.total == dict1.group.total
    assert torch.equal(one.group.pflat, dict1.group.pflat) and torch.equal(one.group.pflat, two.group.pflat)
    assert len(dict1.param_groups) == 1
    assert {k: v for k, v in one.param_groups[0].items() if k != "params"} == {k: v for k, v in dict1.param_groups[0].items() if k != "params"}
    assert [p.shape for p in one.param_groups[0]["params"]] == [p.shape for p in dict1.param_groups[0]["params"]]
    assert one.state_dict()["param_groups"] == dict1.state_dict()["param_groups"]
    for o in (one, dict1, two):
        o.step()
    assert [c[0] for c in calls] == [f"{which}_step", f"{which}_step", f"{which}_step_seg"]
    k = 3 if which == "sgd" else 4                                                   # the first argument after the buffers
    assert calls[0][1][k:] == calls[1][1][k:]                                        # the same scalar arguments
    assert len(calls[2][1][-3]) == 2 and calls[2][1][k] is two.table
    # a one-dict list with an override is still one group on the old entry, with the override in force
    n4, _ = six_params("cpu")
    o4 = cls([{"params": n4, "lr": 0.25}], "cpu", lr=1e-3, **kw)
    o4.step()
    assert calls[-1][0] == f"{which}_step" and calls[-1][1][k] == 0.25


def _twin_groups(opt, **kw):
    return [dict({k: v for k, v in g.items() if k in kw or k == "params"}) for g in opt.param_groups]


def test_checkpoint_indices_equal_torch_adamw():
    from vbg.optim import FusedAdamW
    named, letters = six_params("cpu")
    opt = FusedAdamW(split(named, letters, weight_decay=0.0, lr=3e-4), "cpu", lr=1e-3, layout=named)
    twin = torch.optim.AdamW([{"params": opt.param_groups[0]["params"]}, {"params": opt.param_groups[1]["params"], "weight_decay": 0.0, "lr": 3e-4}], lr=1e-3)
    sd, sd_t = opt.state_dict(), twin.state_dict()
    assert sd["param_groups"] == sd_t["param_groups"]
    assert [g["params"] for g in sd["param_groups"]] == [[0, 1, 2, 3], [4, 5]] and sd["state"] == {}
    # with state: the same keys, and every index names the same parameter on both sides
    opt.steps = 3
    opt.m.copy_(torch.arange(TOTAL, dtype=torch.float32))
    for p in [p for g in twin.param_groups for p in g["params"]]:
        p.grad = torch.zeros_like(p)
    twin.step()
    sd, sd_t = opt.state_dict(), twin.state_dict()
    assert sorted(sd["state"]) == sorted(sd_t["state"]) == list(range(6))
    order = [n for n, _ in named if letters[n] == "A"] + [n for n, _ in named if letters[n] == "B"]
    for i, n in enumerate(order):
        off = OFFSETS[[x for x, _, _ in LAYOUT].index(n)]
        st = sd["state"][i]
        assert set(st) == set(sd_t["state"][i]) == {"step", "exp_avg", "exp_avg_sq"}
        assert st["exp_avg"].shape == sd_t["state"][i]["exp_avg"].shape and float(st["step"]) == 3.0
        assert torch.equal(st["exp_avg"].flatten(), torch.arange(off, off + st["exp_avg"].numel(), dtype=torch.float32))
    twin.load_state_dict(sd)                                                         # torch accepts it
    with pytest.raises(ValueError):                                                  # other groups: refused, not mis-assigned
        opt.load_state_dict(torch.optim.AdamW([p for g in twin.param_groups for p in g["params"]], lr=1e-3).state_dict())


@pytest.mark.parametrize("which", ["sgd", "adamw"])
def test_state_dict_round_trip(which):
    from vbg.optim import FusedAdamW, FusedSGD
    cls, kw = (FusedSGD, {"momentum": 0.9}) if which == "sgd" else (FusedAdamW, {})
    named, letters = six_params("cpu")
    a = cls(split(named, letters, weight_decay=0.0, lr=3e-4), "cpu", lr=1e-3, layout=named, **kw)
    a.steps = 2
    gen = torch.Generator().manual_seed(5)
    for f in a._flat_state().values():
        f[:END].copy_(torch.randn(END, generator=gen))
    a.param_groups[1]["lr"] = 7e-5                                                   # what a scheduler left behind
    named2, letters2 = six_params("cpu", seed=1)
    b = cls(split(named2, letters2), "cpu", lr=1.0, layout=named2, **kw)
    b.load_state_dict(a.state_dict())
    assert b.steps == (2 if which == "adamw" else 1)                                 # (SGD checkpoints carry no step count: "not the first step")
    for k, f in a._flat_state().items():
        # parameter slots equal; the padding between slots is not part of any parameter and comes back zero
        for i in range(6):
            assert torch.equal(a.group.view(f, i), b.group.view(b._flat_state()[k], i)), (k, i)
    assert [{k: v for k, v in g.items() if k != "params"} for g in b.param_groups] == [{k: v for k, v in g.items() if k != "params"} for g in a.param_groups]
    assert b.param_groups[1]["lr"] == 7e-5 and b.param_groups[1]["weight_decay"] == 0.0


def test_chunk_table_is_validated_where_it_is_built():
    from vbg import ops
    ok = ops.chunk_table([(0, 8, 0), (8, 64, 1)], 2, 72, "cpu")
    assert ok.n == 2
    assert ops.chunk_table(np.zeros((0, 3), dtype=np.int64), 1, 0, "cpu").n == 0
    for bad, ngroups, numel in (([(2, 8, 0)], 1, 64), ([(0, 6, 0)], 1, 64), ([(0, 0, 0)], 1, 64), ([(0, 8, 1)], 1, 64), ([(0, 8, -1)], 1, 64),
                                ([(60, 8, 0)], 1, 64), ([(-4, 8, 0)], 1, 64), ([(0, 16, 0), (8, 8, 0)], 1, 64), ([(0, 8, 0)], 0, 64),
                                ([(0, 8, 0)], 33, 64)):
        with pytest.raises(ValueError):
            ops.chunk_table(bad, ngroups, numel, "cpu")
    with pytest.raises(ValueError):                                                  # hyper-parameter sets must match the table's groups
        ops.sgd_step_seg(torch.zeros(72), torch.zeros(72), torch.zeros(72), ok, [(0.1, 0.9, 0.0)], True)
    with pytest.raises(ValueError):                                                  # buffers shorter than the table's range
        ops.adamw_step_seg(torch.zeros(64), torch.zeros(72), torch.zeros(72), torch.zeros(72), ok, [(1e-3, 0.9, 0.999, 1e-8, 0.0)] * 2, 1)


def test_argument_errors_of_the_segmented_entries():
    from vbg import lib as L
    sgd, adamw = L.lib.vbg_sgd_step_seg, L.lib.vbg_adamw_step_seg
    hs, ha = (L.SgdGroup * 33)(), (L.AdamwGroup * 33)()
    assert sgd(None, None, None, None, 0, hs, 1, 1, 1.0, None) == 0                  # nchunks == 0 is a no-op
    assert sgd(None, None, None, None, 0, hs, 32, 0, 1.0, None) == 0
    assert adamw(None, None, None, None, None, 0, ha, 1, 1, 1.0, None) == 0
    assert adamw(None, None, None, None, None, 0, ha, 32, 1, 1.0, None) == 0
    for ng in (0, 33, -1):
        assert sgd(None, None, None, None, 0, hs, ng, 1, 1.0, None) == -1
        assert adamw(None, None, None, None, None, 0, ha, ng, 1, 1.0, None) == -1
    assert sgd(None, None, None, None, -1, hs, 1, 1, 1.0, None) == -1
    assert adamw(None, None, None, None, None, -1, ha, 1, 1, 1.0, None) == -1
    assert adamw(None, None, None, None, None, 0, ha, 1, 0, 1.0, None) == -1         # step >= 1, as vbg_adamw_step
    assert sgd(None, None, None, None, 1, hs, 1, 1, 1.0, None) == -1                 # null buffers with work to do
    assert adamw(None, None, None, None, None, 1, ha, 1, 1, 1.0, None) == -1
    assert L.OPTIM_MAX_GROUPS == 32


def test_struct_sizes_against_the_c_compiler(tmp_path):
    """sizeof / offsetof of vbg_optim_chunk, vbg_sgd_group, vbg_adamw_group from a C compiler over include/vbg.h == the ctypes mirrors"""
    from vbg.lib import AdamwGroup, OptimChunk, SgdGroup
    assert (C.sizeof(OptimChunk), C.sizeof(SgdGroup), C.sizeof(AdamwGroup)) == (16, 12, 20)
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    assert cc is not None, "no C compiler"
    pairs = (("vbg_optim_chunk", OptimChunk), ("vbg_sgd_group", SgdGroup), ("vbg_adamw_group", AdamwGroup))
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "vbg.h"', 'int main(void) {', 'printf("max 0 %d\\n", VBG_OPTIM_MAX_GROUPS);']
    for st, cls in pairs:
        src.append(f'printf("{st} sizeof %zu\\n", sizeof({st}));')
        for name, _ in cls._fields_:
            src.append(f'printf("{st} {name} %zu\\n", offsetof({st}, {name}));')
    src += ['return 0; }']
    cfile = tmp_path / "sz.c"
    cfile.write_text("\n".join(src))
    exe = str(tmp_path / "sz")
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(cfile), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {(a, b): int(c) for a, b, c in (ln.split() for ln in out if ln)}
    assert got[("max", "0")] == 32
    for st, cls in pairs:
        assert got[(st, "sizeof")] == C.sizeof(cls)
        for name, _ in cls._fields_:
            assert got[(st, name)] == getattr(cls, name).offset, (st, name)
