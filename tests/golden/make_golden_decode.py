"""Generate tests/golden/decode.npz by calling the REAL reference post-processing, deployment/inference_EPHOIE.EPHOIE_postprocessing
(C = 12, no regex filters, plain concatenation), on CPU tensors.  Every segment's text is unique ("[17]" for segment 17), so each
returned string spells its run's start and length.  The fixture is plain data (inputs, texts, returned strings; allow_pickle=False);
tests read the .npz only.

    python tests/golden/make_golden_decode.py [reference root]

The reference's modules import `ltp` and `torchvision`, which are not installed: `ltp` is stubbed here, torchvision by
make_golden.install_torchvision_stub.  Neither is reached by the function under test.

Conditions on the inputs, asserted below, under which a last-ulp difference between torch's CPU softmax and the library's cannot
change a class or a winner: every row's two largest probabilities differ by at least 0.05; within a class, two filed run means are
either ties made from bit-identical rows or at least 1e-3 apart."""
import importlib.machinery
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402

C = 12
TOP2_GAP = 0.05
MEAN_GAP = 1e-3


def install_ltp_stub():
    m = types.ModuleType("ltp")
    m.__spec__ = importlib.machinery.ModuleSpec("ltp", None)
    m.LTP = type("LTP", (), {})
    sys.modules["ltp"] = m


def rows_for(classes, levels, seed):
    """one row per entry: small noise everywhere, `level` on the row's class"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(len(classes), C, generator=g) - 0.5
    for i, (c, a) in enumerate(zip(classes, levels)):
        x[i, c] = a
    return x.float()


def conditions(x, tied_runs=()):
    """assert the two conditions of the module docstring; tied_runs: pairs of run starts whose rows are bit-identical by construction"""
    p = x.softmax(1)
    top = p.topk(min(2, C), dim=1).values
    assert float((top[:, 0] - top[:, 1]).min()) >= TOP2_GAP, float((top[:, 0] - top[:, 1]).min())
    cls = p.argmax(1).tolist()
    score = p.max(1).values.double().tolist()
    n = len(cls)
    starts = [i for i in range(n) if i == 0 or cls[i] != cls[i - 1]]
    filed = {}
    for k, s in enumerate(starts):
        e = starts[k + 1] if k + 1 < len(starts) else n
        where = cls[s] if k + 1 < len(starts) else (C - 1 if n == 1 else cls[n - 2])
        filed.setdefault(where, []).append((s, sum(score[s:e]) / (e - s)))
    for recs in filed.values():
        for i in range(len(recs)):
            for j in range(i + 1, len(recs)):
                (sa, ma), (sb, mb) = recs[i], recs[j]
                if (sa, sb) in tied_runs:
                    assert ma == mb, (sa, sb, ma, mb)
                else:
                    assert abs(ma - mb) >= MEAN_GAP, (sa, sb, ma, mb)
    return cls


def random_case(n):
    """a few hundred rows in runs of 1..6 segments; the first seed whose run means are MEAN_GAP apart"""
    for seed in range(1000):
        g = torch.Generator().manual_seed(9000 + seed)
        classes, levels = [], []
        while len(classes) < n:
            c = int(torch.randint(0, C, (1,), generator=g))
            if classes and c == classes[-1]:
                continue
            ln = min(int(torch.randint(1, 7, (1,), generator=g)), n - len(classes))
            classes += [c] * ln
            levels += (2.0 + 4.0 * torch.rand(ln, generator=g)).tolist()
        x = rows_for(classes, levels, 9500 + seed)
        try:
            conditions(x)
        except AssertionError:
            continue
        return x
    raise RuntimeError("no seed met the conditions")


def cases():
    out = {}
    out["n1"] = rows_for([3], [3.0], 1)                                             # filed under class C - 1
    out["n2_same"] = rows_for([6, 6], [3.0, 4.0], 2)
    out["n2_diff_second_wins"] = rows_for([3, 5], [2.5, 4.0], 3)                    # both records under class 3; "[1]" wins it
    out["n2_diff_first_wins"] = rows_for([3, 5], [4.0, 2.5], 4)
    out["last_single_after_long"] = rows_for([2, 2, 2, 7], [3.0, 3.5, 2.5, 5.0], 5)   # "[3]" filed under class 2, and wins it
    out["last_single_loses"] = rows_for([0, 2, 2, 2, 7], [3.0, 5.0, 5.5, 4.5, 2.5], 6)
    tie = rows_for([4, 4, 0, 4, 4, 0, 0], [3.0, 4.0, 3.0, 3.0, 4.0, 2.5, 4.5], 7)
    tie[3:5] = tie[0:2]                                                             # bit-identical rows: equal means, the first run wins
    out["tie_first_wins"] = tie
    out["random300"] = random_case(300)
    return out, {"tie_first_wins": {(0, 3)}}


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else MG.REF
    MG.install_torchvision_stub()
    install_ltp_stub()
    sys.path.insert(0, ref)
    from deployment.inference_EPHOIE import EPHOIE_CLASS_LIST, EPHOIE_postprocessing

    assert len(EPHOIE_CLASS_LIST) == C
    xs, tied = cases()
    arrs = {"names": np.array(list(xs))}
    for name, x in xs.items():
        cls = conditions(x, tied.get(name, ()))
        texts = [f"[{i}]" for i in range(x.shape[0])]
        got = EPHOIE_postprocessing(pred_label=x, num_classes=C, ocr_text=(texts,))
        want = [got[k] for k in EPHOIE_CLASS_LIST[1:]]                              # classes 1 .. C - 1 (the function skips class 0)
        assert any(want), name
        arrs[f"x_{name}"] = x.numpy()
        arrs[f"text_{name}"] = np.array(texts)
        arrs[f"want_{name}"] = np.array(want)
        print(name, "classes", sorted(set(cls)), "->", {i + 1: s[:24] for i, s in enumerate(want) if s})
    np.savez_compressed(os.path.join(HERE, "decode.npz"), **arrs)
    assert not any(v.dtype == object for v in arrs.values())


if __name__ == "__main__":
    main()
