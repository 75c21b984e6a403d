"""Generate tests/golden/crf_posterior.npz by calling the REAL reference CRF, model/crf.py, in double on CPU tensors.

    python tests/golden/make_golden_crf_posterior.py [reference root]

For three cases, (ntag, rows) = (9, 15), (27, 300) and (27, 700), the fixture records the inputs (emissions, transitions), the log Z
of `_forward_alg`, the gradient of that log Z with respect to the emissions -- the reference's own statement of the posterior
marginals p(y_t = i | x) -- and the path and score of `_viterbi_decode`.  The reference's file is loaded on its own (it imports
nothing but torch).  The fixture is plain data (allow_pickle=False); tests read the .npz only.

Inputs as in tests/test_gpu_kernels.py::test_crf_vs_oracle: randn emissions, 2 * randn transitions, START = ntag - 2, STOP = ntag - 1
with the START row and the STOP column at -10000."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [("t9_n15", 9, 15), ("t27_n300", 27, 300), ("t27_n700", 27, 700)]


def load_reference_crf(ref):
    spec = importlib.util.spec_from_file_location("reference_crf", os.path.join(ref, "model", "crf.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    if len(sys.argv) > 1:
        ref = sys.argv[1]
    else:
        sys.path.insert(0, HERE)
        import make_golden as MG
        ref = MG.REF
    R = load_reference_crf(ref)
    arrs = {"names": np.array([c[0] for c in CASES])}
    for name, ntag, rows in CASES:
        g = torch.Generator().manual_seed(7000 + ntag + rows)
        em = torch.randn(rows, ntag, generator=g)
        trans = torch.randn(ntag, ntag, generator=g) * 2
        start, stop = ntag - 2, ntag - 1
        tag_to_ix = {f"t{k}": k for k in range(ntag - 2)}
        tag_to_ix[R.START_TAG], tag_to_ix[R.STOP_TAG] = start, stop
        crf = R.CRF(tag_to_ix).double()
        with torch.no_grad():
            crf.transitions.copy_(trans.double())
            crf.transitions[start, :] = -10000
            crf.transitions[:, stop] = -10000
        feats = em.double().requires_grad_(True)
        logz = crf._forward_alg(feats)
        (marg,) = torch.autograd.grad(logz, feats)
        logz = logz.detach()
        with torch.no_grad():
            score, path = crf._viterbi_decode(feats)
        assert float((marg.sum(1) - 1).abs().max()) < 1e-9
        arrs[f"em_{name}"] = em.numpy()
        arrs[f"trans_{name}"] = crf.transitions.detach().float().numpy()
        arrs[f"ends_{name}"] = np.array([start, stop], dtype=np.int32)
        arrs[f"logz_{name}"] = np.array(float(logz), dtype=np.float64)
        arrs[f"marg_{name}"] = marg.numpy()
        arrs[f"path_{name}"] = np.array(path, dtype=np.int32)
        arrs[f"score_{name}"] = np.array(float(score), dtype=np.float64)
        print(name, "logz", float(logz), "score", float(score), "min row max", float(marg.max(1).values.min()))
    assert not any(v.dtype == object for v in arrs.values())
    np.savez_compressed(os.path.join(HERE, "crf_posterior.npz"), **arrs)


if __name__ == "__main__":
    main()
