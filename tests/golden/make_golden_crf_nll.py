"""Generate tests/golden/crf_nll.npz by calling the REAL reference CRF, model/crf.py, in double on CPU tensors.

    python tests/golden/make_golden_crf_nll.py [reference root]

For three cases, (ntag, rows) = (9, 15), (27, 300) and (27, 700), the fixture records the inputs (emissions, transitions, gold tags),
the value of `CRF.forward(feats, tags)` -- (log Z - gold score) / rows -- and autograd's gradient of it with respect to the emissions
and to the transitions.  The reference's file is loaded on its own (it imports nothing but torch).  The fixture is plain data
(allow_pickle=False); tests read the .npz only.

Inputs as in tests/golden/make_golden_crf_posterior.py (the same seeds: the same emissions and transitions), the tags drawn behind them
from the tags that are neither START nor STOP."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_crf_posterior import CASES, load_reference_crf  # noqa: E402


def main():
    if len(sys.argv) > 1:
        ref = sys.argv[1]
    else:
        import make_golden as MG
        ref = MG.REF
    R = load_reference_crf(ref)
    # model/crf.py creates its initial vector and its score accumulator with the default dtype; with float32 there the gold score is
    # added up in float32 even under .double() (a [1] float32 tensor plus 0-dim doubles stays float32).  In double means all of it.
    torch.set_default_dtype(torch.float64)
    arrs = {"names": np.array([c[0] for c in CASES])}
    for name, ntag, rows in CASES:
        g = torch.Generator().manual_seed(7000 + ntag + rows)
        em = torch.randn(rows, ntag, generator=g, dtype=torch.float32)
        trans = torch.randn(ntag, ntag, generator=g, dtype=torch.float32) * 2
        tags = torch.randint(0, ntag - 2, (rows,), generator=g)
        start, stop = ntag - 2, ntag - 1
        tag_to_ix = {f"t{k}": k for k in range(ntag - 2)}
        tag_to_ix[R.START_TAG], tag_to_ix[R.STOP_TAG] = start, stop
        crf = R.CRF(tag_to_ix).double()
        with torch.no_grad():
            crf.transitions.copy_(trans.double())
            crf.transitions[start, :] = -10000
            crf.transitions[:, stop] = -10000
        feats = em.double().requires_grad_(True)
        nll = crf(feats, tags)
        dem, dtrans = torch.autograd.grad(nll.sum(), [feats, crf.transitions])
        # at marginal scale every row of the emission gradient is a distribution less an indicator: it sums to 0
        assert float((dem * rows).sum(1).abs().max()) < 1e-9
        arrs[f"em_{name}"] = em.numpy()
        arrs[f"trans_{name}"] = crf.transitions.detach().float().numpy()
        arrs[f"ends_{name}"] = np.array([start, stop], dtype=np.int32)
        arrs[f"tags_{name}"] = tags.numpy().astype(np.int32)
        nll = nll.detach()
        assert nll.dtype == torch.float64
        arrs[f"nll_{name}"] = np.array(float(nll.sum()), dtype=np.float64)
        arrs[f"dem_{name}"] = dem.numpy()
        arrs[f"dtrans_{name}"] = dtrans.numpy()
        print(name, "nll", float(nll.sum()), "max |dem| * rows", float(dem.abs().max()) * rows, "max |dtrans| * rows", float(dtrans.abs().max()) * rows)
    assert not any(v.dtype == object for v in arrs.values())
    np.savez_compressed(os.path.join(HERE, "crf_nll.npz"), **arrs)


if __name__ == "__main__":
    main()
