"""A numpy statement of a1 (pipeline/transform.py:104-171, 225-271 of the reference), written from the formula and shared by the
host and GPU tests of vbg_transform_batch.

An image is fp32 CHW on the 0..1 scale (format 0), uint8 CHW (format 1) or uint8 HWC (format 2); a byte u is the sample
float32(u) / float32(255), by division.  Every sample is normalised, (x - mean[c]) / std[c], and the output pixel (oy, ox) of an
[oh, ow] resize is the bilinear blend at the source coordinate

    fy = max((oy + 0.5) * h / oh - 0.5, 0)          fx = max((ox + 0.5) * w / ow - 0.5, 0)

with y0 = floor(fy), y1 = min(y0 + 1, h - 1), ly = fy - y0 (columns alike): align_corners=False with the scale in / out, which is what
`F.interpolate(..., recompute_scale_factor=True)` uses.  oh == h and ow == w is the plain normalisation.  The result lies in the
top-left corner of a zero [H, W, 3] slot.  Boxes: int(float32(v) * float32(ratio)) with columns 0, 2 on the HEIGHT ratio oh / h and
columns 1, 3 on the width ratio ow / w (the reference's swap, :167-168), ratios formed in double and rounded to fp32.
"""
import numpy as np

F32_CHW, U8_CHW, U8_HWC = 0, 1, 2


def samples(img: np.ndarray, fmt: int) -> np.ndarray:
    """-> fp32 [3, h, w] on the 0..1 scale"""
    if fmt == F32_CHW:
        assert img.dtype == np.float32 and img.shape[0] == 3
        return img
    assert img.dtype == np.uint8
    chw = img if fmt == U8_CHW else np.transpose(img, (2, 0, 1))
    assert chw.shape[0] == 3
    return chw.astype(np.float32) / np.float32(255.0)


def transform_image(img, fmt, oh, ow, mean, std, H, W) -> np.ndarray:
    """-> fp32 [H, W, 3]: the slot of one image"""
    x = samples(np.asarray(img), fmt)
    _, h, w = x.shape
    mean = np.asarray(mean, dtype=np.float32).reshape(3, 1, 1)
    std = np.asarray(std, dtype=np.float32).reshape(3, 1, 1)
    xn = ((x - mean) / std).astype(np.float32)
    out = np.zeros((H, W, 3), dtype=np.float32)
    if (oh, ow) == (h, w):
        out[:oh, :ow] = np.transpose(xn, (1, 2, 0))
        return out
    sy, sx = np.float32(h) / np.float32(oh), np.float32(w) / np.float32(ow)
    fy = np.maximum((np.arange(oh, dtype=np.float32) + np.float32(0.5)) * sy - np.float32(0.5), np.float32(0))
    fx = np.maximum((np.arange(ow, dtype=np.float32) + np.float32(0.5)) * sx - np.float32(0.5), np.float32(0))
    y0, x0 = fy.astype(np.int64), fx.astype(np.int64)
    y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
    ly, lx = (fy - y0.astype(np.float32))[:, None], (fx - x0.astype(np.float32))[None, :]
    hy, hx = np.float32(1) - ly, np.float32(1) - lx
    a, b = xn[:, y0][:, :, x0], xn[:, y0][:, :, x1]
    d, e = xn[:, y1][:, :, x0], xn[:, y1][:, :, x1]
    v = hy * (hx * a + lx * b) + ly * (hx * d + lx * e)
    out[:oh, :ow] = np.transpose(v.astype(np.float32), (1, 2, 0))
    return out


def rescale_boxes(boxes: np.ndarray, h, w, oh, ow) -> np.ndarray:
    """int64 [S, 4] -> int32 [S, 4]"""
    rh, rw = np.float32(oh / h), np.float32(ow / w)
    r = np.array([rh, rw, rh, rw], dtype=np.float32)
    return (np.asarray(boxes).reshape(-1, 4).astype(np.float32) * r).astype(np.int32)


def transform_batch(images, fmts, sizes, mean, std, H, W, boxes):
    """-> (batch fp32 [B,H,W,3], boxes int32 [N,4], box_off int32 [B+1], box_doc int32 [N]); boxes[b] may be None (no rows)"""
    B = len(images)
    batch = np.stack([transform_image(images[b], fmts[b], sizes[b][0], sizes[b][1], mean, std, H, W) for b in range(B)]) \
        if B else np.zeros((0, H, W, 3), np.float32)
    rows, off, doc = [], [0], []
    for b in range(B):
        x = samples(np.asarray(images[b]), fmts[b])
        bx = np.zeros((0, 4), np.int64) if boxes[b] is None else np.asarray(boxes[b]).reshape(-1, 4)
        rows.append(rescale_boxes(bx, x.shape[1], x.shape[2], sizes[b][0], sizes[b][1]))
        off.append(off[-1] + len(bx))
        doc += [b] * len(bx)
    packed = np.concatenate(rows, 0) if rows else np.zeros((0, 4), np.int32)
    return batch, packed.astype(np.int32), np.asarray(off, np.int32), np.asarray(doc, np.int32)
