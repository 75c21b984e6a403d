"""Rectangular RoIAlign bins (roi_shape=(h, w)) without a GPU: known answers for the restatement (tests/roi_align_restate.py), the
oracle's square RoIAlign against it on cfg2-like boxes, the model's shape handling and the argument checks of the (h, w) C entries."""
import numpy as np
import pytest
import torch

import roi_align_restate as R


def _ramp(H, W, C=1):
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return np.repeat((10 * yy + xx)[None, :, :, None], C, 3)


@pytest.mark.parametrize("shape", [(3, 21), (5, 2), (7, 7), (1, 1), (8, 32)])
def test_constant_map_gives_constant(shape):
    f = np.full((1, 16, 20, 3), 2.5)
    y = R.roi_align_fwd(f, [[4, 8, 40, 36], [0, 0, 80, 64], [-2, -2, 30, 20]], [0, 0, 0], shape, 0.25)
    assert y.shape == (3,) + shape + (3,)
    assert np.allclose(y, 2.5, rtol=0, atol=1e-6)


@pytest.mark.parametrize("shape", [(3, 21), (5, 2)])
def test_affine_ramp_is_sampled_at_bin_centres(shape):
    """bilinear interpolation and averaging are exact for an affine map: every bin returns the ramp at its centre"""
    oh, ow = shape
    f = _ramp(32, 40)
    box = [8, 12, 92, 96]                                   # *0.25 -> x 2..23, y 3..24 (21 x 21 feature pixels)
    y = R.roi_align_fwd(f, [box], [0], shape, 0.25)[0, :, :, 0]
    bh, bw = 21.0 / oh, 21.0 / ow
    exp = np.array([[10 * (3.0 + (p + .5) * bh) + (2.0 + (q + .5) * bw) for q in range(ow)] for p in range(oh)])
    assert np.allclose(y, exp, rtol=1e-5, atol=1e-4)


def test_gh_differs_from_gw():
    """a 3 x 21 output on a 21 x 21 RoI: gh = ceil(21 / 3) = 7 samples down, gw = 1 across; the count is 7"""
    y1, x1, bin_h, bin_w, gh, gw, cnt = R.geometry([8, 12, 92, 96], 0.25, 3, 21)
    assert (gh, gw, cnt) == (7, 1, 7) and bin_h == np.float32(7.0) and bin_w == np.float32(1.0)
    # against a direct sum over the samples with the full 2-D taps
    f = np.random.default_rng(0).standard_normal((1, 32, 40, 2))
    got = R.roi_align_fwd(f, [[8, 12, 92, 96]], [0], (3, 21), 0.25)
    ref = np.zeros((3, 21, 2))
    for p in range(3):
        for q in range(21):
            for i in range(gh):
                for j in range(gw):
                    ty = R.tap1(R.sample_coord(y1, p, bin_h, i, gh), 32)
                    tx = R.tap1(R.sample_coord(x1, q, bin_w, j, gw), 40)
                    if ty is None or tx is None:
                        continue
                    for yy, wy in ((ty[0], ty[2]), (ty[1], ty[3])):
                        for xx, wx in ((tx[0], tx[2]), (tx[1], tx[3])):
                            ref[p, q] += float(wy) * float(wx) * f[0, yy, xx]
    assert np.allclose(got[0], ref / cnt, rtol=1e-12, atol=1e-12)


def test_degenerate_outside_and_clipped_boxes():
    H, W = 16, 16
    f = np.ones((1, H, W, 1))
    # outside: every sample has y > H and x > W -> 0
    assert float(np.abs(R.roi_align_fwd(f, [[400, 400, 440, 440]], [0], (3, 21), 0.25)).max()) == 0.0
    # clipped at the origin: samples in [-1, 0] clamp to 0, so a constant map still gives the constant
    assert np.allclose(R.roi_align_fwd(f, [[-2, 0, 26, 28]], [0], (2, 5), 0.25), 1.0)
    # clipped past the far edge: samples beyond W add nothing, those in [W - 1, W] sit on the last column
    y = R.roi_align_fwd(f, [[48, 0, 80, 8]], [0], (1, 4), 0.25)[0, 0, :, 0]     # x 12..20 on a 16-wide map
    assert np.allclose(y[:2], 1.0) and y[3] == 0.0
    # degenerate (zero-area) box -> 1 x 1 feature pixel, one sample per bin at bins of 1/h, 1/w
    g = R.geometry([20, 24, 20, 24], 0.25, 3, 21)
    assert g[4:] == (1, 1, 1) and g[2] == np.float32(1.0) / np.float32(3) and g[3] == np.float32(1.0) / np.float32(21)
    ramp = _ramp(H, W)
    y = R.roi_align_fwd(ramp, [[20, 24, 20, 24]], [0], (3, 21), 0.25)[0, :, :, 0]
    exp = np.array([[10 * (6 + (p + .5) / 3) + (5 + (q + .5) / 21) for q in range(21)] for p in range(3)])
    assert np.allclose(y, exp, rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("shape", [(3, 21), (8, 32), (7, 7)])
def test_adjoint_identity(shape):
    """<A f, g> == <f, A^T g> on cfg2-like boxes"""
    rng = np.random.default_rng(5)
    B, H, W, C = 2, 24, 32, 3
    boxes, doc = R.cfg2_like_boxes(rng, B, 12, H, W)
    f = rng.standard_normal((B, H, W, C))
    g = rng.standard_normal((len(boxes),) + shape + (C,))
    lhs = float((R.roi_align_fwd(f, boxes, doc, shape, 0.25) * g).sum())
    rhs = float((f * R.roi_align_adjoint(g, (B, H, W, C), boxes, doc, shape, 0.25)).sum())
    assert abs(lhs - rhs) <= 1e-10 * max(1.0, abs(lhs))


def test_oracle_square_roi_align_matches_restatement():
    """the independent pin of the oracle's RoIAlign: cfg2-like boxes (>= 20 per document) with clipped, degenerate, whole-map and
    more-than-one-sample-per-bin boxes"""
    import vbg_oracle as O
    rng = np.random.default_rng(11)
    B, H, W, C = 2, 128, 128, 4
    boxes, doc = R.cfg2_like_boxes(rng, B, 20, H, W)
    assert all((doc == b).sum() >= 20 for b in range(B))
    gs = [R.geometry(bx, 0.25, 7, 7) for bx in boxes]
    assert any(g[4] > 1 and g[5] > 1 for g in gs) and any(g[4] == 1 and g[5] == 1 for g in gs)
    f = rng.standard_normal((B, H, W, C)).astype(np.float32)
    per_doc = [torch.from_numpy(boxes[doc == b]).float() for b in range(B)]
    ref = O.roi_align(torch.from_numpy(f).permute(0, 3, 1, 2).contiguous(), per_doc, 7, 0.25)     # [n, C, 7, 7], boxes in doc order
    got = R.roi_align_fwd(f, boxes, doc, 7, 0.25)
    err = np.abs(ref.permute(0, 2, 3, 1).double().numpy() - got)
    assert float(err.max()) <= 3e-5, float(err.max())


def test_grid_roi_align_shapes():
    from model.grid_roi_align import GridROIAlign
    assert GridROIAlign((3, 21)).output_size == (3, 21)
    assert GridROIAlign(7).output_size == 7
    with pytest.raises(TypeError):
        GridROIAlign([3, 21])                     # what a YAML list gives: upstream raises TypeError here too
    from vbg import ops
    assert ops.roi_out_hw(7) == (7, 7) and ops.roi_out_hw((3, 21)) == (3, 21) and ops.roi_out_hw((4, 16, 9)) == (4, 16)
    assert ops.roi_bwd_form(128, 128, 7, 7) == "sep" and ops.roi_bwd_form(128, 128, 3, 21) == "sep"
    assert ops.roi_bwd_form(128, 128, 8, 32) == "tap" and ops.roi_bwd_form(128, 128, 14, 14) == "tap"
    assert ops.roi_bwd_form(128, 128, 1, 32) == "sep" and ops.roi_bwd_form(128, 128, 1, 33) == "tap"
    assert ops.roi_bwd_form(300, 128, 7, 7) == "tap"


def test_late_fusion_sizes_linear_by_h_times_w():
    from model.field_type_classification_head import LateFusion
    lf = LateFusion(768, 8, (3, 21))
    assert tuple(lf.ROI_embedding_net.linear.weight.shape) == (1024, 8 * 63)
    lf = LateFusion(768, 8, (4, 16, 2))                 # a longer tuple: its first two entries
    assert tuple(lf.ROI_embedding_net.linear.weight.shape) == (1024, 8 * 64)


def test_hw_entries_argument_errors_without_a_launch():
    from vbg import lib as L
    lib = L.lib
    for oh, ow in ((0, 7), (7, 0), (-1, 3), (3, -2)):
        assert lib.vbg_roi_align_hw_fwd(1, 1, 8, 8, 4, 1, 1, 1, oh, ow, 0.25, 1, None) == -1
        assert lib.vbg_roi_align_hw_bwd(1, 1, 8, 8, 4, 1, 1, 1, oh, ow, 0.25, 1, None) == -1
        assert lib.vbg_roi_align_hw_bwd_det(1, 1, 8, 8, 4, 1, 1, 1, oh, ow, 0.25, 1, None) == -1
    assert lib.vbg_roi_align_hw_bwd_det(1, 1, 8, 8, 4, 1, 1, 1, 3, 33, 0.25, 1, None) == -1     # out_w beyond 32
    assert lib.vbg_roi_align_hw_bwd_det(1, 1, 8, 8, 4, 1, 1, 1, 33, 3, 0.25, 1, None) == -1     # out_h beyond 32
    assert lib.vbg_roi_align_hw_bwd_det(1, 1, 8, 512, 4, 1, 1, 1, 3, 32, 0.25, 1, None) == -1   # wx[32][512] beyond 48 KB of LDS
    assert lib.vbg_roi_align_hw_fwd(None, 1, 8, 8, 4, None, None, 1, 3, 21, 0.25, None, None) == -1
    # no RoIs: nothing to launch, success
    assert lib.vbg_roi_align_hw_fwd(1, 1, 8, 8, 4, None, None, 0, 3, 21, 0.25, 1, None) == 0
