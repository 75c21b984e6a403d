"""vbg_ohem_topk against today's route on the same list (ops.ce_fwd, ops.sort_desc, two gathers: pipeline/custom_loss.py
CrossEntropyLossOHEM.forward), both on the device: the chosen elements and the keep are EQUAL.  vbg_ce_fwd_dyn / vbg_ce_bwd_dyn against
the fp64 statement of tests/test_gpu_small_kernels.py::_check_ce at its tolerances.  Needs a real MI355X."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from vbg import ops as _ops
    return _ops


def dev():
    return torch.device("cuda")


def gen(seed):
    return torch.Generator().manual_seed(seed)


def close(a, b, rtol, atol):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    d = (a - b).abs()
    ok = a.shape == b.shape and bool((d <= atol + rtol * b.abs()).all())
    if not ok:
        print("max abs", float(d.max()), "at", int(d.argmax()))
    return ok


def todays_route(ops, logits, elem, labels, m, k, w, up, H, W):
    """CrossEntropyLossOHEM.forward's choice on the first m entries of `elem`"""
    el = elem[:m].contiguous()
    keep = min(m, k)
    if not (0 < keep < m):
        return el, keep
    v = ops.ce_fwd(logits, el, labels, m, w, up, H, W)
    _, si = ops.sort_desc(v)
    ranks = ops.gather_i32(si, si[:keep].contiguous())
    return ops.gather_i32(el, ranks), keep


def problem(ncls, rows, seed, up=0, B=0, H=0, W=0):
    """logits with repeated rows (tied losses), saturated rows (loss +0 for their class), labels with one value outside [0, ncls)"""
    g = gen(seed)
    logits = torch.randn(rows, ncls, generator=g) * 2.0
    logits[rows // 3:rows // 3 + rows // 4] = logits[:rows // 4]                     # repeated rows
    nel = rows if not up else B * H * W
    labels = torch.randint(0, ncls, (nel,), generator=g)
    if not up:
        labels[rows // 3:rows // 3 + rows // 4] = labels[:rows // 4]                 # ... with the same label: exactly tied losses
        sat = torch.arange(rows - rows // 5, rows)
        logits[sat] = -200.0
        logits[sat, labels[sat]] = 200.0                                             # saturated: log-softmax is exactly 0
    labels[5 % nel] = ncls + 3                                                       # outside the classes: NaN loss, sorted first
    return logits, labels


@pytest.mark.parametrize("ncls", [2, 5, 64])
@pytest.mark.parametrize("cap", [32, 512, 4096])
def test_ohem_topk_equals_todays_route(ops, ncls, cap):
    d = dev()
    rows = 3000
    logits, labels = problem(ncls, rows, seed=cap + ncls)
    w = torch.tensor([0.5, 0.0, 2.0, 1.5, 1.0, 0.25, 3.0])[torch.arange(ncls) % 7]   # class 1 has weight 0: more +0 losses
    lg, lab, wd = logits.to(d), labels.int().to(d), w.to(d)
    k = cap // 2
    g = gen(9 * cap + ncls)
    ms = [0, 1, k, k + 1, cap]
    # all five counts in two calls: lists of capacity `cap` side by side, each with its own device count
    elems = [torch.randint(0, rows, (cap,), generator=g).int() for _ in ms]
    for e in elems:
        e[1] = 5                                                                     # the element with the label out of range
    for lo in (0, 4):
        part = list(range(lo, min(lo + 4, len(ms))))
        elem = torch.cat([elems[j] for j in part]).to(d)
        m_dev = torch.tensor([ms[j] for j in part], dtype=torch.int32, device=d)
        out, keep = ops.ohem_topk(lg, elem, m_dev, [cap] * len(part), [k] * len(part), lab, wd)
        for slot, j in enumerate(part):
            want, wkeep = todays_route(ops, lg, elems[j].to(d), lab, ms[j], k, wd, 0, 0, 0)
            assert int(keep[slot]) == wkeep, (ms[j], int(keep[slot]), wkeep)
            got = out[slot * cap:slot * cap + wkeep]
            assert torch.equal(got, want[:wkeep]), (ms[j], got[:8].tolist(), want[:8].tolist())


def test_ohem_topk_upsampled_logits_and_unequal_lists(ops):
    """up_shift = 2 over H, W = 16, 24 (logits rows at quarter resolution: every 4 x 4 block of elements shares a row, so ties are the
    rule), two lists of different capacity and k in one call"""
    d = dev()
    B, H, W, ncls = 2, 16, 24, 5
    logits, labels = problem(ncls, B * (H >> 2) * (W >> 2), seed=77, up=2, B=B, H=H, W=W)
    lg, lab = logits.to(d), labels.int().to(d)
    g = gen(78)
    caps, ks, ms = [64, 512], [32, 256], [50, 400]
    elems = [torch.randperm(B * H * W, generator=g)[:c].int() for c in caps]
    out, keep = ops.ohem_topk(lg, torch.cat(elems).to(d), torch.tensor(ms, dtype=torch.int32, device=d), caps, ks, lab, None, 2, H, W)
    o = 0
    for j, (e, cap, k, m) in enumerate(zip(elems, caps, ks, ms)):
        want, wkeep = todays_route(ops, lg, e.to(d), lab, m, k, None, 2, H, W)
        assert int(keep[j]) == wkeep
        assert torch.equal(out[o:o + wkeep], want[:wkeep])
        o += cap


def test_ohem_topk_argument_errors(ops):
    from vbg import lib as L
    d = dev()
    lg = torch.zeros(8, 2, device=d)
    e = torch.zeros(8192, dtype=torch.int32, device=d)
    lab = torch.zeros(8, dtype=torch.int32, device=d)
    m = torch.zeros(4, dtype=torch.int32, device=d)
    with pytest.raises(L.VbgError):
        ops.ohem_topk(lg, e, m, [4097], [8], lab)                                    # cap <= 4096
    with pytest.raises(L.VbgError):
        ops.ohem_topk(lg, e, m, [0], [8], lab)
    with pytest.raises(L.VbgError):
        ops.ohem_topk(lg, e, m, [16], [0], lab)


@pytest.mark.parametrize("ncls", [2, 5, 64])
@pytest.mark.parametrize("which", ["zero", "one", "cap-1"])
def test_ce_dyn_counts(ops, ncls, which):
    """the first `count` of `cap` elements; the slots at and beyond the count hold VALID indices of rows with a large loss, so that an
    over-read is a wrong sum, not a fault.  Losses 1e-5 / 1e-6, gradients 1e-4 / 1e-6 (fp64 statement); the destination outside the
    selected rows and outside the logits' columns is untouched bit for bit."""
    d = dev()
    rows, cap, ld, c0 = 500, 300, 80, 3
    count = {"zero": 0, "one": 1, "cap-1": cap - 1}[which]
    g = gen(31 + ncls)
    logits = torch.randn(rows, ncls, generator=g) * 2.0
    labels = torch.randint(0, ncls, (rows,), generator=g)
    bad = torch.arange(rows - 20, rows)                                              # rows with a loss of about 60
    logits[bad] = 30.0
    logits[bad, labels[bad]] = -30.0
    elem = torch.randint(0, rows - 20, (cap,), generator=g)
    elem[count:] = bad[torch.arange(cap - count) % 20]
    w = torch.tensor([0.5, 0.0, 2.0, 1.5, 1.0, 0.25, 3.0])[torch.arange(ncls) % 7]
    wide = torch.randn(rows, ld, generator=g)
    wide[:, c0:c0 + ncls] = logits
    lg = wide.to(d)[:, c0:c0 + ncls]
    el_d, lab_d, w_d = elem.int().to(d), labels.int().to(d), w.to(d)
    n_dev = torch.tensor([count], dtype=torch.int32, device=d)
    sentinel = torch.full((cap,), -7.25, device=d)
    got = ops.ce_fwd_dyn(lg, el_d, lab_d, n_dev, w_d, out=sentinel.clone())
    x = logits.double().requires_grad_(True)
    pick = elem[:count].long()
    ref = F.cross_entropy(x[pick], labels[pick], weight=w.double(), reduction="none")
    assert close(got[:count], ref, 1e-5, 1e-6)
    assert torch.equal(got[count:], sentinel[count:])                                # nothing written at or beyond the count
    gs = torch.tensor([1.7])
    (ref.sum() * 0.3 * float(gs)).backward()
    R = torch.randn(rows, ld, generator=g) * 0.05
    want = R.double()
    if count:
        want[:, c0:c0 + ncls] += x.grad
    for det in (False, True):
        with ops.deterministic_scope(det):
            dl = R.to(d)
            ops.ce_bwd_dyn(lg, el_d, lab_d, n_dev, w_d, gs.to(d), 0.3, 0, 0, 0, dl[:, c0:c0 + ncls])
        dlc = dl.cpu()
        assert close(dlc, want, 1e-4, 1e-6), det
        untouched = torch.ones(rows, dtype=torch.bool)
        untouched[pick] = False
        assert torch.equal(dlc[untouched], R[untouched]), det                        # rows nobody selected: bit for bit
        assert torch.equal(dlc[:, :c0], R[:, :c0]) and torch.equal(dlc[:, c0 + ncls:], R[:, c0 + ncls:])


def test_selected_ce_dyn_fn_sum_and_gradient(ops):
    """vbg.functions.SelectedCEDynFn: sum over the first count elements times a device scale, gradient through ce_bwd_dyn"""
    from vbg import functions as Fn
    d = dev()
    rows, ncls, cap, count = 200, 5, 64, 37
    g = gen(4)
    logits = torch.randn(rows, ncls, generator=g)
    labels = torch.randint(0, ncls, (rows,), generator=g)
    elem = torch.randint(0, rows, (cap,), generator=g)
    lg = logits.to(d).requires_grad_(True)
    scale = torch.tensor([1.0 / count], device=d)
    out = Fn.SelectedCEDynFn.apply(lg, elem.int().to(d), torch.tensor([count], dtype=torch.int32, device=d), labels.int().to(d), None, scale, 0, 0, 0)
    out.backward()
    x = logits.double().requires_grad_(True)
    ref = F.cross_entropy(x[elem[:count]], labels[elem[:count]], reduction="sum") / count
    ref.backward()
    assert out.dim() == 0 and out.dtype == torch.float32
    assert close(out, ref, 1e-5, 1e-6) and close(lg.grad, x.grad, 1e-4, 1e-6)
