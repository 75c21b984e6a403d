"""The wave kernels of the CRF head and the field decoding kernels against tests/golden/crf_decode_bits.npz: the bits of every output of
ops.crf_posterior, crf_viterbi, crf_path_logp, crf_nll_stable, crf_nll_stable_bwd, field_decode, field_decode_tags, field_runs and
field_runs_tags, as recorded on an MI355X by the commit before csrc/crf.hip and csrc/decode.hip stated their shared steps once
(tests/golden/make_golden_crf_decode_bits.py holds the cases and the inputs' bits and replays them here).  Values stay with the fp64
restatements of test_gpu_crf_*.py, test_gpu_field_*.py and test_gpu_decode_tags.py.  The first test needs no GPU: it holds the committed
file to the generator's cases on any machine."""
import os
import sys

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_golden_crf_decode_bits as M          # noqa: E402

sys.path.remove(GOLDEN)


@pytest.fixture(scope="module")
def fix(golden):
    return M.load(golden("crf_decode_bits.npz"))


def compare(fix, prefix, run):
    """every recorded word of the case, and the same bits on a second call"""
    want = {k.split(":", 1)[1]: v for k, v in fix[1].items() if k.startswith(prefix + ":")}
    got, again = run(), run()
    assert sorted(got) == sorted(want), prefix
    for name, t in got.items():
        sha, size, kept = M.digest(t)
        assert size == want[name][1], (prefix, name, size)
        assert np.array_equal(kept, want[name][2]), (prefix, name, kept, want[name][2])
        assert sha == want[name][0], (prefix, name)
        assert M.digest(again[name])[0] == sha, (prefix, name)


def test_the_fixture_holds_every_case(fix):
    inp, rec = fix
    cases = {k.split(":", 1)[0] for k in rec}
    assert cases == {f"crf/{f}/{n}" for f, n in M.crf_case_ids()} | {f"{e}/{c}" for e, c in M.decode_case_ids()}
    assert [n for _, n in M.crf_case_ids()] == list(M.CRF_EDGE_NTAG) + list(M.CRF_TILE_NTAG) + [M.CRF_SHIFT_NTAG]
    for f, n in M.crf_case_ids():                           # the stable loss at its three sizes, loss-only call and scaling launch included
        names = {k.split(":", 1)[1] for k in rec if k.startswith(f"crf/{f}/{n}:")}
        assert {"post/path", "post/score", "post/logz", "post/marg", "vit/path", "vit/score", "logp/viterbi/lm", "logp/random/lc"} <= names
        assert ("stable/bwd/dtrans" in names and "stable/loss_only/nll" in names and "stable/dem_unit" in names) == (n in M.CRF_STABLE_NTAG)
    for e, c in M.decode_case_ids():
        names = {k.split(":", 1)[1] for k in rec if k.startswith(f"{e}/{c}:")}
        assert len(names) == 3 * 2 * len(M.DEC_ROWS)
    again = M.make_inputs()                                 # what the generator would store today (the replay reads the file's)
    assert sorted(again) == sorted(inp) and all(inp[k].dtype == again[k].dtype and inp[k].shape == again[k].shape for k in inp)
    # the inputs reach what they are there for: tags outside the table in the random path, begin tags inside a run on rows 64, 255, 256
    path = M.crf_inputs(inp, "tile", 25)[5].tolist()
    assert -1 in path and 25 in path and path[-1] == 1 << 30
    for c in M.DEC_C:
        p, tb = inp[f"path/{c}/r513"].tolist(), M.tag_table(c)[2]
        assert all(tb[p[r]] == 1 and p[r - 1] == p[r] for r in M.DEC_BEGIN_ROWS)


@pytest.mark.gpu
@pytest.mark.parametrize("family,ntag", M.crf_case_ids())
def test_crf_bits(fix, family, ntag):
    from vbg import ops
    compare(fix, f"crf/{family}/{ntag}", lambda: M.crf_case(ops, fix[0], family, ntag, torch.device("cuda")))


@pytest.mark.gpu
@pytest.mark.parametrize("entry,C", M.decode_case_ids())
def test_decode_bits(fix, entry, C):
    from vbg import ops
    compare(fix, f"{entry}/{C}", lambda: M.decode_case(ops, fix[0], entry, C, torch.device("cuda")))
