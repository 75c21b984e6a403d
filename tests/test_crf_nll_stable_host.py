"""What the GPU tests of vbg_crf_nll_stable lean on, checked without a GPU: the fp64 restatement (tests/crf_nll_restate.py) against
brute-force enumeration and against the reference CRF's own numbers (tests/golden/crf_nll.npz: `CRF.forward(feats, tags)` of the real
model/crf.py in double, with autograd's gradients), the two entries' argument checks, and the switch that routes CRF.nll."""
import os
import subprocess
import sys

import numpy as np
import pytest

import crf_nll_restate as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "crf_nll.npz")
CASES = [("t9_n15", (15, 9)), ("t27_n300", (300, 27)), ("t27_n700", (700, 27))]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN, allow_pickle=False)


def test_fixture_cases(golden):
    assert [str(n) for n in golden["names"]] == [c[0] for c in CASES]
    for name, shape in CASES:
        assert golden[f"em_{name}"].shape == shape and golden[f"dem_{name}"].shape == shape
        assert golden[f"dem_{name}"].dtype == np.float64 and golden[f"dtrans_{name}"].dtype == np.float64
        assert golden[f"tags_{name}"].dtype == np.int32 and golden[f"tags_{name}"].shape == (shape[0],)
        assert golden[f"dtrans_{name}"].shape == (shape[1], shape[1])


@pytest.mark.parametrize("T,rows", [(4, 1), (4, 2), (4, 3), (4, 4), (5, 1), (5, 4), (3, 3)])
def test_restatement_against_brute_force(T, rows):
    start, stop = T - 2, T - 1
    rng = np.random.default_rng(60 + 10 * T + rows)
    em = rng.standard_normal((rows, T))
    trans = 2 * rng.standard_normal((T, T))
    trans[start, :] = -10000
    trans[:, stop] = -10000
    tags = rng.integers(0, T - 2, rows)
    nll, logz, dem, dtr = R.nll_and_grads(em, tags, trans, start, stop)
    bnll, bz, bdem, bdtr = R.brute_force(em, tags, trans, start, stop)
    assert abs(logz - bz) <= 1e-12 * max(1.0, abs(bz)) and abs(nll - bnll) <= 1e-12 * max(1.0, abs(bnll))
    assert float(np.abs(dem - bdem).max()) <= 1e-12 and float(np.abs(dtr - bdtr).max()) <= 1e-12
    # what the tables are by construction: rows of distributions less indicators; all transitions of a path less all of the gold one's
    assert float(np.abs(dem.sum(1)).max()) <= 1e-12 and abs(float(dtr.sum())) <= 1e-12
    assert bool((dem[:, [start, stop]] == 0).all())


def test_restatement_of_an_empty_document():
    trans = np.array([[0.5, 1.0, -10000.0], [-10000.0] * 3, [0.25, 2.0, -10000.0]])
    nll, logz, dem, dtr = R.nll_and_grads(np.zeros((0, 3)), [], trans, 1, 2)
    assert nll == 0.0 and logz == 2.0 and dem.shape == (0, 3) and not dtr.any()


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_restatement_against_the_reference(golden, name):
    """1e-9 absolute at marginal scale (rows x gradient): the bound the fixtures' generators assert on their own row sums"""
    em, trans, tags = golden[f"em_{name}"], golden[f"trans_{name}"], golden[f"tags_{name}"]
    start, stop = (int(v) for v in golden[f"ends_{name}"])
    n = em.shape[0]
    nll, _, dem, dtr = R.nll_and_grads(em, tags, trans, start, stop)
    e_em = float(np.abs(dem - n * golden[f"dem_{name}"]).max())
    e_tr = float(np.abs(dtr - n * golden[f"dtrans_{name}"]).max())
    e_nll = abs(n * nll - n * float(golden[f"nll_{name}"]))
    print(name, "restatement - reference at marginal scale: emissions", e_em, "transitions", e_tr, "nll", e_nll)
    assert e_em <= 1e-9 and e_tr <= 1e-9 and e_nll <= 1e-9


# ---- the entries' argument checks: before any launch, without a GPU
def test_entry_argument_errors_do_not_need_a_gpu():
    import ctypes as C
    from vbg import lib as L
    f, b = L.lib.vbg_crf_nll_stable, L.lib.vbg_crf_nll_stable_bwd
    p = C.c_void_p(64)                                       # never dereferenced: every call below returns before a launch
    ok = dict(em=p, tags=p, off=p, ndoc=1, trans=p, ntag=7, start=5, stop=6, nll=p, logz=p, du=p, tu=p)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["em"], a["tags"], a["off"], a["ndoc"], a["trans"], a["ntag"], a["start"], a["stop"], a["nll"], a["logz"], a["du"], a["tu"], None)

    assert call(ntag=0) == -1 and call(ntag=65, start=63, stop=64) == -1
    assert call(start=-1) == -1 and call(start=7) == -1 and call(stop=-1) == -1 and call(stop=7) == -1
    assert call(ndoc=-1) == -1
    assert call(du=None) == -1 and call(tu=None) == -1                                # exactly one table
    assert call(du=None, ndoc=0) == -1 and call(ntag=0, ndoc=0) == -1                 # wrong whatever the number of documents
    for k in ("em", "tags", "off", "trans", "nll", "logz"):
        assert call(**{k: None}) == -1, k
    assert call(ndoc=0) == 0 and call(ndoc=0, du=None, tu=None) == 0                  # no document: a no-op
    assert f(None, None, None, 0, None, 1, 0, 0, None, None, None, None, None) == 0  # one tag is inside [1, 64]

    okb = dict(du=p, tu=p, off=p, ndoc=1, ntag=7, gout=p, dem=p, dtr=p)

    def callb(**kw):
        a = dict(okb, **kw)
        return b(a["du"], a["tu"], a["off"], a["ndoc"], a["ntag"], a["gout"], a["dem"], a["dtr"], None)

    assert callb(ntag=0) == -1 and callb(ntag=65) == -1 and callb(ndoc=-1) == -1
    for k in ("du", "tu", "off", "gout", "dem", "dtr"):
        assert callb(**{k: None}) == -1, k
    assert callb(ndoc=0) == 0 and b(None, None, None, 0, 64, None, None, None, None) == 0


# ---- the switch
def _child(env_value):
    env = {k: v for k, v in os.environ.items() if k != "VBG_CRF_STABLE"}
    if env_value is not None:
        env["VBG_CRF_STABLE"] = env_value
    code = "from vbg import ops; print(int(ops.crf_stable_enabled()))"
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True,
                         cwd=os.path.join(os.path.dirname(HERE), "vibertgrid-pytorch_amd"))
    return out.stdout.strip().splitlines()[-1]


def test_switch_is_off_by_default_and_follows_the_environment():
    assert _child(None) == "0" and _child("0") == "0" and _child("") == "0"
    assert _child("1") == "1"


def test_crf_nll_picks_the_function_by_the_switch(monkeypatch):
    import torch
    from model.crf import CRF, START_TAG, STOP_TAG
    from vbg import functions as Fn
    from vbg import ops
    if "VBG_CRF_STABLE" not in os.environ:
        assert ops.crf_stable_enabled() is False
    taken = []
    monkeypatch.setattr(Fn.CrfNllFn, "apply", staticmethod(lambda *a: taken.append(("default", a)) or "default"))
    monkeypatch.setattr(Fn.CrfNllStableFn, "apply", staticmethod(lambda *a: taken.append(("stable", a)) or "stable"))
    crf = CRF({"O": 0, "B-x": 1, START_TAG: 2, STOP_TAG: 3})
    feats, tags, off = torch.zeros(3, 4), torch.zeros(3, dtype=torch.int32), torch.tensor([0, 3], dtype=torch.int32)
    before = ops.crf_stable_enabled()
    try:
        ops.set_crf_stable(False)
        assert crf.nll(feats, tags, off) == "default"
        ops.set_crf_stable(True)
        assert ops.crf_stable_enabled() is True
        assert crf.nll(feats, tags, off) == "stable"                                  # read at call time, not at construction
        assert crf(feats, tags.long()) == "stable"                                    # CRF.forward goes through nll
        ops.set_crf_stable(False)
        assert crf(feats, tags.long()) == "default"
    finally:
        ops.set_crf_stable(before)
    assert [t[0] for t in taken] == ["default", "stable", "stable", "default"]
    for _, a in taken:                                                                # the same arguments on both routes
        assert a[0] is feats and a[1] is crf.transitions and a[4:] == (2, 3)
