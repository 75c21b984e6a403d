"""Host side of the batched input transform (vbg_transform_batch): the numpy yardstick of the GPU tests against torch's CPU chain,
format detection from strides, descriptor tables across the launch cap, argument errors without a launch, and the PackedBatch round
trip of an HWC byte image.  No GPU."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import transform_restate as R

MEAN, STD = [0.9248, 0.9224, 0.9215], [0.1532, 0.1545, 0.1536]


def _bytes(h, w, seed):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 256, size=(3, h, w)).astype(np.uint8))


def _torch_chain(x01, scale):
    """normalise, then the reference's resize_image (:139-146)"""
    m, s = torch.tensor(MEAN).view(3, 1, 1), torch.tensor(STD).view(3, 1, 1)
    xn = (x01 - m) / s
    if scale is None:
        return xn
    return F.interpolate(xn[None], scale_factor=scale, mode="bilinear", recompute_scale_factor=True, align_corners=False)[0]


def test_division_by_255_is_torchs_conversion_and_the_reciprocal_is_not():
    u = torch.arange(256, dtype=torch.uint8)
    ref = u.float().div(255).numpy()
    got = R.samples(np.broadcast_to(u.numpy().reshape(1, 16, 16), (3, 16, 16)).copy(), R.U8_CHW)[0].reshape(-1)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    recip = u.numpy().astype(np.float32) * np.float32(1.0 / 255.0)
    assert int((recip.view(np.uint32) != ref.view(np.uint32)).sum()) == 126


@pytest.mark.parametrize("h,w,scale", [(37, 53, 0.78), (5, 7, 3.3), (1, 9, 3.0), (64, 64, None)])
@pytest.mark.parametrize("fmt", [R.F32_CHW, R.U8_CHW, R.U8_HWC])
def test_restatement_against_torch_cpu(h, w, scale, fmt):
    u8 = _bytes(h, w, 7 * h + w)
    x01 = u8.float().div(255)
    ref = _torch_chain(x01, scale)
    oh, ow = ref.shape[-2:]
    if scale is not None:
        assert (oh, ow) == (int(math.floor(h * scale)), int(math.floor(w * scale)))
    img = {R.F32_CHW: x01.numpy(), R.U8_CHW: u8.numpy(), R.U8_HWC: np.ascontiguousarray(u8.permute(1, 2, 0).numpy())}[fmt]
    H, W = oh + 3, ow + 5
    got = R.transform_image(img, fmt, oh, ow, MEAN, STD, H, W)
    tol = 1e-6 if scale is None else 1e-4
    assert np.allclose(got[:oh, :ow], ref.permute(1, 2, 0).numpy(), rtol=tol, atol=tol)
    pad = got.copy()
    pad[:oh, :ow] = 0
    assert not pad.view(np.uint32).any()                        # +0.0 bit for bit outside the image


def test_restated_boxes_match_the_reference_arithmetic():
    boxes = np.array([[0, 0, 10, 20], [3, 7, 33, 51], [1, 1, 36, 52]], dtype=np.int64)
    h, w, oh, ow = 37, 53, 28, 41
    rh, rw = torch.tensor(oh / h, dtype=torch.float32), torch.tensor(ow / w, dtype=torch.float32)
    t = torch.from_numpy(boxes).float()
    ref = torch.stack([t[:, 0] * rh, t[:, 1] * rw, t[:, 2] * rh, t[:, 3] * rw], 1).int().numpy()
    assert np.array_equal(R.rescale_boxes(boxes, h, w, oh, ow), ref)


def test_format_is_read_from_strides():
    from vbg import ops
    from vbg.lib import IMAGE_F32_CHW, IMAGE_U8_CHW, IMAGE_U8_HWC
    for h, w in ((5, 7), (3, 7), (5, 3), (3, 3), (1, 9), (9, 1)):
        hwc = torch.from_numpy(np.random.RandomState(h * 10 + w).randint(0, 256, size=(h, w, 3)).astype(np.uint8))
        view = hwc.permute(2, 0, 1)
        t, fmt = ops.transform_input(view)
        if view.is_contiguous():                # (h == w == 1 only: both readings address the same bytes)
            assert fmt == IMAGE_U8_CHW
        else:
            assert fmt == IMAGE_U8_HWC and t.data_ptr() == hwc.data_ptr()          # read in place
        chw = view.contiguous()
        t, fmt = ops.transform_input(chw)
        assert fmt == IMAGE_U8_CHW and t.data_ptr() == chw.data_ptr()
        t, fmt = ops.transform_input(chw.float())
        assert fmt == IMAGE_F32_CHW and t.dtype == torch.float32
    # other strides: a copy; other float dtypes: fp32
    wide = torch.zeros(3, 6, 10, dtype=torch.uint8)[:, :, ::2]
    t, fmt = ops.transform_input(wide)
    assert fmt == IMAGE_U8_CHW and t.is_contiguous() and t.shape == (3, 6, 5)
    t, fmt = ops.transform_input(torch.zeros(3, 4, 5, dtype=torch.float64))
    assert fmt == IMAGE_F32_CHW and t.dtype == torch.float32 and t.is_contiguous()
    t, fmt = ops.transform_input(torch.zeros(4, 5, 3).permute(2, 0, 1))
    assert fmt == IMAGE_F32_CHW and t.is_contiguous()


@pytest.mark.parametrize("dt", [torch.int8, torch.int16, torch.int32, torch.int64, torch.bool])
def test_integer_images_other_than_bytes_raise(dt):
    from vbg import ops
    with pytest.raises(TypeError):
        ops.transform_input(torch.zeros(3, 4, 5, dtype=dt))


def test_descriptor_table_and_offsets_past_the_cap():
    from vbg import lib as L, ops
    cap = ops.TRANSFORM_MAX_IMAGES
    assert cap == L.lib.vbg_transform_max_images() == L.TRANSFORM_MAX_IMAGES and cap >= 8
    B = cap + 3
    images = [torch.zeros(3, 2 + b % 3, 3 + b % 2, dtype=torch.uint8 if b % 2 else torch.float32) for b in range(B)]
    coors = [None if b == 5 else torch.zeros((b % 4, 4), dtype=torch.int64) for b in range(B)]
    sizes = [(4 + b % 2, 6) for b in range(B)]
    descs, keep, counts = ops.transform_table(images, sizes, coors)
    assert len(descs) == B and counts == [0 if b == 5 else b % 4 for b in range(B)]
    row = 0
    for b in range(B):
        d = descs[b]
        assert d.img == images[b].data_ptr() and d.format == (1 if b % 2 else 0)
        assert (d.h, d.w, d.oh, d.ow) == (2 + b % 3, 3 + b % 2, 4 + b % 2, 6)
        assert d.S == counts[b] and d.box_row == row                    # the offsets run on across the launch boundary
        assert (d.boxes is None) == (counts[b] == 0)
        row += counts[b]
    assert (cap + cap - 1) // cap == 1 and (B + cap - 1) // cap == 2


def test_argument_errors_before_any_launch():
    import ctypes as C
    from vbg import lib as L
    f = L.lib.vbg_transform_batch
    m = (C.c_float * 3)(0.5, 0.5, 0.5)
    one = C.c_void_p(16)                                              # (never dereferenced: every call below fails its checks)

    def call(B=1, H=8, W=8, N=0, **kw):
        d = (L.TransformImage * 1)()
        d[0].img, d[0].format, d[0].h, d[0].w, d[0].oh, d[0].ow, d[0].S, d[0].box_row = 16, 0, 4, 4, 8, 8, 0, 0
        for k, v in kw.items():
            setattr(d[0], k, v)
        return f(d, B, m, m, one, H, W, None, None, None, N, None)

    assert f(None, 0, None, None, None, 0, 0, None, None, None, 0, None) == 0          # B == 0: a no-op
    assert call(B=-1) == -1
    for field in ("h", "w", "oh", "ow"):
        assert call(**{field: 0}) == -1
    assert call(oh=9) == -1 and call(ow=9) == -1                       # larger than the slot
    assert call(format=3) == -1 and call(format=-1) == -1
    assert call(S=-1) == -1
    assert call(S=2, N=2) == -1                                        # rows without a box pointer
    assert call(img=None) == -1


def _collate(images):
    z = torch.zeros(2, dtype=torch.int64)
    B = len(images)
    return (tuple(images), tuple(z for _ in range(B)), tuple(z for _ in range(B)),
            tuple(torch.zeros((2, 4), dtype=torch.int64) for _ in range(B)), torch.zeros((B, 4), dtype=torch.int64), torch.ones((B, 4), dtype=torch.int64))


def test_packed_batch_keeps_an_hwc_view():
    from vbg.batch import PackedBatch
    rs = np.random.RandomState(3)
    hwc = [torch.from_numpy(rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)) for h, w in ((37, 53), (5, 7), (3, 3))]
    views = [t.permute(2, 0, 1) for t in hwc]
    pb = PackedBatch.pack(*_collate(views), pin=False)
    out = pb.to("cpu")[0]
    for v, o, src in zip(views, out, hwc):
        assert o.dtype == torch.uint8 and o.shape == v.shape and o.stride() == v.stride() and torch.equal(o, v)
        n = src.numel()
        start = o.data_ptr() - pb.buf.data_ptr()
        assert torch.equal(pb.buf[start:start + n], src.reshape(-1))      # the bytes as they lay in memory: no transpose
    # the same pixels as ToTensor's fp32: four times the image bytes (up to the 16-byte slots)
    pf = PackedBatch.pack(*_collate([v.float().div(255) for v in views]), pin=False)
    rest = PackedBatch.pack(*_collate([torch.zeros(3, 0, 0, dtype=torch.uint8) for _ in views]), pin=False).nbytes()
    img_u8, img_f32 = pb.nbytes() - rest, pf.nbytes() - rest
    assert img_u8 == sum((v.numel() + 15) // 16 * 16 for v in views)
    assert 4 * (img_u8 - 15 * len(views)) <= img_f32 <= 4 * img_u8       # (a slot is rounded up by at most 15 bytes)


def test_packed_batch_of_contiguous_inputs_is_unchanged():
    from vbg.batch import PackedBatch
    rs = np.random.RandomState(4)
    imgs = [torch.from_numpy(rs.rand(3, 6, 5).astype(np.float32)), torch.from_numpy(rs.randint(0, 256, size=(3, 4, 7)).astype(np.uint8))]
    args = _collate(imgs)
    pb = PackedBatch.pack(*args, pin=False)
    # the layout of the parent: every tensor's bytes in order, each slot rounded up to 16
    want = []
    for g in (args[0], args[1], args[2], args[3], (args[4],), (args[5],)):
        for t in g:
            raw = t.contiguous().view(-1).view(torch.uint8) if t.numel() else torch.zeros(0, dtype=torch.uint8)
            want.append(raw)
            want.append(torch.zeros(-raw.numel() % 16, dtype=torch.uint8))
    want = torch.cat(want)
    assert pb.nbytes() == want.numel()
    off = 0
    for row in pb.table:
        assert len(row) == 4                                               # no strides recorded for contiguous tensors
    for g in (args[0], args[1], args[2], args[3], (args[4],), (args[5],)):
        for t in g:
            n = t.numel() * t.element_size()
            assert torch.equal(pb.buf[off:off + n], want[off:off + n])
            off += (n + 15) // 16 * 16
    out = pb.to("cpu")
    assert all(torch.equal(a, b) and a.is_contiguous() for a, b in zip(out[0], imgs))
