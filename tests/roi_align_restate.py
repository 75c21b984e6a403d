"""RoIAlign restated from the published algorithm (He et al., Mask R-CNN; torchvision.ops.RoIAlign with output_size=(h, w),
spatial_scale, sampling_ratio=-1, aligned=False), independent of the oracle and of torch.

Geometry per RoI, each step one np.float32 operation in the kernels' order (csrc/roi.hip roi_geo / sample_coord / make_tap):
    x1 = box[0] * scale, ...;  roi_w = max(x2 - x1, 1),  roi_h = max(y2 - y1, 1)
    bin_h = roi_h / h,  bin_w = roi_w / w,  gh = ceil(roi_h / h),  gw = ceil(roi_w / w),  count = max(gh * gw, 1)
    sample y of bin row p, index i = (y1 + p * bin_h) + ((i + .5) * bin_h) / gh     (x likewise)
A sample outside [-1, size] adds nothing; otherwise it is clamped to >= 0, and at or past size - 1 both taps sit on the last row.
The bilinear weights are separable (hy | ly) x (hx | lx) and a sample is valid iff its y and its x are, so the RoIAlign matrix of one
RoI is Wy (x) Wx / count with Wy[p][Y] = the summed y weights of bin row p's samples on row Y.  The forward applies it in fp64; the
adjoint applies its transpose (the exact backward of the same sparse matrix).  Layout: feature maps NHWC [B, H, W, C], RoI outputs
[n, h, w, C]."""
import math

import numpy as np

f32 = np.float32


def out_hw(out_size):
    """int -> (s, s); tuple -> its first two entries (as torchvision reads output_size)"""
    if isinstance(out_size, (int, np.integer)):
        return int(out_size), int(out_size)
    return int(out_size[0]), int(out_size[1])


def geometry(box, scale, oh, ow):
    """-> (y_start, x_start, bin_h, bin_w, gh, gw, count) as the kernels compute them (fp32 scalar steps)"""
    s = f32(scale)
    x1, y1, x2, y2 = (f32(f32(v) * s) for v in box)
    rw = max(f32(x2 - x1), f32(1.0))
    rh = max(f32(y2 - y1), f32(1.0))
    bin_h, bin_w = f32(rh / f32(oh)), f32(rw / f32(ow))
    gh, gw = int(math.ceil(float(f32(rh / f32(oh))))), int(math.ceil(float(f32(rw / f32(ow)))))
    return y1, x1, bin_h, bin_w, gh, gw, max(gh * gw, 1)


def sample_coord(start, p, bin_, i, g):
    return f32(f32(start + f32(f32(p) * bin_)) + f32(f32(f32(f32(i) + f32(0.5)) * bin_) / f32(g)))


def tap1(v, size):
    """1-D bilinear tap of one sample coordinate -> None (outside) or (i0, i1, w0, w1), w in fp32"""
    v = f32(v)
    if v < f32(-1.0) or v > f32(size):
        return None
    if v <= f32(0.0):
        v = f32(0.0)
    i0 = int(v)
    if i0 >= size - 1:
        i0 = i1 = size - 1
        v = f32(i0)
    else:
        i1 = i0 + 1
    w1 = f32(v - f32(i0))
    w0 = f32(f32(1.0) - w1)
    return i0, i1, w0, w1


def axis_weights(start, bin_, g, nbins, size):
    """-> dense [nbins, size] fp64: row p = the summed 1-D weights of bin p's g samples"""
    w = np.zeros((nbins, size), np.float64)
    for p in range(nbins):
        for i in range(g):
            t = tap1(sample_coord(start, p, bin_, i, g), size)
            if t is None:
                continue
            i0, i1, w0, w1 = t
            w[p, i0] += float(w0)
            w[p, i1] += float(w1)
    return w


def roi_matrices(box, scale, oh, ow, H, W):
    """-> (Wy [oh, H], Wx [ow, W], count): the RoI's RoIAlign matrix is kron(Wy, Wx) / count"""
    y1, x1, bin_h, bin_w, gh, gw, cnt = geometry(box, scale, oh, ow)
    return axis_weights(y1, bin_h, gh, oh, H), axis_weights(x1, bin_w, gw, ow, W), cnt


def _support(w):
    nz = np.nonzero(w.any(0))[0]
    return (int(nz[0]), int(nz[-1]) + 1) if nz.size else (0, 0)


def roi_align_fwd(feat, boxes, box_doc, out_size, scale):
    """feat [B, H, W, C]; boxes [n, 4] (x1, y1, x2, y2 image coordinates); box_doc [n] -> [n, h, w, C] fp64"""
    feat = np.asarray(feat, np.float64)
    boxes, box_doc = np.asarray(boxes), np.asarray(box_doc)
    _, H, W, C = feat.shape
    oh, ow = out_hw(out_size)
    y = np.zeros((len(boxes), oh, ow, C), np.float64)
    for r in range(len(boxes)):
        wy, wx, cnt = roi_matrices(boxes[r], scale, oh, ow, H, W)
        (ya, yb), (xa, xb) = _support(wy), _support(wx)
        if ya == yb or xa == xb:
            continue
        patch = feat[int(box_doc[r]), ya:yb, xa:xb]
        y[r] = np.einsum("py,yxc,qx->pqc", wy[:, ya:yb], patch, wx[:, xa:xb]) / cnt
    return y


def roi_align_adjoint(dy, feat_shape, boxes, box_doc, out_size, scale):
    """the transpose of roi_align_fwd: dy [n, h, w, C] -> d feat [B, H, W, C] fp64"""
    dy = np.asarray(dy, np.float64)
    boxes, box_doc = np.asarray(boxes), np.asarray(box_doc)
    B, H, W, C = feat_shape
    oh, ow = out_hw(out_size)
    df = np.zeros((B, H, W, C), np.float64)
    for r in range(len(boxes)):
        wy, wx, cnt = roi_matrices(boxes[r], scale, oh, ow, H, W)
        (ya, yb), (xa, xb) = _support(wy), _support(wx)
        if ya == yb or xa == xb:
            continue
        df[int(box_doc[r]), ya:yb, xa:xb] += np.einsum("py,pqc,qx->yxc", wy[:, ya:yb], dy[r], wx[:, xa:xb]) / cnt
    return df


def cfg2_like_boxes(rng, ndoc, per_doc, H, W):
    """image-space boxes of cfg2-like documents on a [H, W] feature map (stride 4): 8-72 x 8-24 px text boxes, plus per document a
    whole-map box, a clipped one, a degenerate one, a sub-pixel one, one fully outside, a tall one (several y samples per bin) and a
    large one (several samples per bin on both axes) -> (boxes int32 [n, 4], box_doc int32 [n])"""
    ih, iw = 4 * H, 4 * W
    boxes, doc = [], []
    for b in range(ndoc):
        x1 = rng.integers(0, iw - 72, per_doc)
        y1 = rng.integers(0, ih - 24, per_doc)
        w = rng.integers(8, 73, per_doc)
        h = rng.integers(8, 25, per_doc)
        bx = np.stack([x1, y1, x1 + w, y1 + h], 1)
        extra = np.array([[0, 0, iw, ih], [iw - 6, ih - 5, iw + 40, ih + 30], [10, 10, 10, 10], [0, 0, 3, 2],
                          [iw + 50, ih + 50, iw + 90, ih + 70], [17, 3, 18, ih - 2], [-12, -9, iw // 2, ih // 2]])
        boxes.append(np.concatenate([bx, extra]))
        doc += [b] * (per_doc + len(extra))
    return np.concatenate(boxes).astype(np.int32), np.asarray(doc, np.int32)
