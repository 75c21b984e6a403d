"""Generate tests/golden/metrics.npz by calling the REAL reference pipeline/criteria.py token_F1_criteria on CPU tensors.  The module
imports `seqeval.metrics`, which is not installed: a stub stands in `sys.modules` (token_F1_criteria does not reach it).  The fixture
is plain data (scores, gt classes, the returned counts and ratios; allow_pickle=False); tests read the .npz only.

    python tests/golden/make_golden_metrics.py [reference root]

Inputs: C in {2, 5, 7}; scores on both sides of -1, 0, 1 and 2 (the function truncates them toward zero and compares with 0 and 1),
negative values, exact 0.0, 1.0, 2.0 and -1.0, softmax rows (the function's normal diet: nearly every cell 0) and one-hot rows (the
only rows on which its TP / FP cells fill)."""
import importlib.machinery
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402


def install_seqeval_stub():
    pkg = types.ModuleType("seqeval")
    pkg.__spec__ = importlib.machinery.ModuleSpec("seqeval", None, is_package=True)
    pkg.__path__ = []
    m = types.ModuleType("seqeval.metrics")
    m.__spec__ = importlib.machinery.ModuleSpec("seqeval.metrics", None)
    for name in ("precision_score", "recall_score", "f1_score", "classification_report"):
        setattr(m, name, None)
    pkg.metrics = m
    sys.modules["seqeval"] = pkg
    sys.modules["seqeval.metrics"] = m


def cases():
    out = {}
    edge = [-2.5, -1.0, -0.999, -0.5, -0.0, 0.0, 0.25, 0.999, 1.0, 1.5, 1.999, 2.0, 2.5, 1e9]
    g = torch.Generator().manual_seed(11)
    # every edge value in every column, under its own class and under another
    x = torch.tensor([[edge[(i + 3 * k) % len(edge)] for k in range(2)] for i in range(2 * len(edge))], dtype=torch.float32)
    out["edges_c2"] = (x, torch.arange(x.shape[0]) % 2)
    x = torch.tensor([[edge[(i + 5 * k) % len(edge)] for k in range(5)] for i in range(5 * len(edge))], dtype=torch.float32)
    out["edges_c5"] = (x, torch.arange(x.shape[0]) % 5)
    out["uniform_c7"] = (torch.rand(300, 7, generator=g) * 5.0 - 2.0, torch.randint(0, 7, (300,), generator=g))      # straddles -1, 0, 1, 2
    out["softmax_c5"] = ((torch.randn(257, 5, generator=g) * 3.0).softmax(1), torch.randint(0, 5, (257,), generator=g))
    hot = torch.nn.functional.one_hot(torch.randint(0, 7, (120,), generator=g), 7).float()                          # exact 1.0 and 0.0
    out["one_hot_c7"] = (hot, torch.randint(0, 7, (120,), generator=g))
    out["negative_c2"] = (-torch.rand(40, 2, generator=g) * 3.0, torch.randint(0, 2, (40,), generator=g))
    return out


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else MG.REF
    install_seqeval_stub()
    sys.path.insert(0, ref)
    from pipeline.criteria import token_F1_criteria

    arrs = {"names": np.array(list(cases()))}
    for name, (x, gt) in cases().items():
        cut = x.shape[0] // 3                                                      # two entries of pred_gt_list: the function concatenates
        got = token_F1_criteria([(x[:cut], gt[:cut]), (x[cut:], gt[cut:])])
        c = got["num_classes"]
        assert c == x.shape[1]
        arrs[f"x_{name}"] = x.numpy()
        arrs[f"gt_{name}"] = gt.numpy().astype(np.int64)
        arrs[f"counts_{name}"] = np.array([[got[k][key] for key in ("TP", "TN", "FP", "FN")] for k in range(c)], dtype=np.int64)
        arrs[f"prf_{name}"] = np.array([[got[k][key] for key in ("precision", "recall", "F1")] for k in range(c)], dtype=np.float64)
        print(name, tuple(x.shape), arrs[f"counts_{name}"].tolist())
    assert not any(v.dtype == object for v in arrs.values())
    np.savez_compressed(os.path.join(HERE, "metrics.npz"), **arrs)


if __name__ == "__main__":
    main()
