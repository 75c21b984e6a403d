"""vbg_transform_batch (csrc/convaux.hip): the whole of a1 in one launch per group of images, for fp32 CHW, uint8 CHW and uint8 HWC
inputs.  Bitwise against the per-image kernels it shares its arithmetic with, bitwise between the three input formats of the same
pixels, against the numpy restatement (tests/transform_restate.py; validated against torch's CPU chain in
tests/test_transform_batch_host.py), across the launch boundary, through the drop-in transform class on the reference's golden file
and through a small model.  The batch buffer handed to the entry is NaN-filled first: the kernel owes every element, padding
included.  Needs a real MI355X."""
import numpy as np
import pytest
import torch

import transform_restate as R

pytestmark = pytest.mark.gpu

MEAN, STD = [0.9248, 0.9224, 0.9215], [0.1532, 0.1545, 0.1536]
H = W = 64
# (h, w) -> (oh, ow): downscale, upscale, identity, single-row; every slot of the 64 x 64 batch has right and bottom padding
CASES = [((37, 53), (29, 41)), ((5, 7), (16, 23)), ((64, 64), (64, 64)), ((1, 9), (3, 27))]
NBOX = [37, 0, 1, 5]


def dev():
    return torch.device("cuda")


@pytest.fixture(scope="module")
def ops():
    from vbg import ops as _ops
    return _ops


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _call(ops, images, sizes, coors, Hh=H, Ww=W):
    out = torch.full((len(images), Hh, Ww, 3), float("nan"), device=dev())
    batch, boxes, off, doc = ops.transform_batch(images, sizes, MEAN, STD, Hh, Ww, coors, out=out)
    assert batch.data_ptr() == out.data_ptr()
    return batch, boxes, off, doc


@pytest.fixture(scope="module")
def mixed():
    """one batch of the four cases as bytes (CPU): uint8 CHW images, int64 boxes that include 0, the image's far corner and values
    whose product with the ratio truncates"""
    rs = np.random.RandomState(11)
    u8, coors = [], []
    for ((h, w), _), n in zip(CASES, NBOX):
        img = rs.randint(0, 256, size=(3, h, w)).astype(np.uint8)
        if (h, w) == (64, 64):
            img[:, :16, :16] = np.arange(256, dtype=np.uint8).reshape(16, 16)      # all 256 byte values in every channel
        u8.append(torch.from_numpy(img))
        c = rs.randint(0, max(h, w) + 1, size=(n, 4)).astype(np.int64)
        if n:
            c[0] = [0, 0, h, w]
        coors.append(torch.from_numpy(c))
    sizes = [s for _, s in CASES]
    return u8, coors, sizes


def _fp32(u8):
    return [u.float().div(255) for u in u8]                      # torch's CPU conversion: the yardstick of the byte formats


def test_a_fp32_bitwise_against_the_per_image_kernels(ops, mixed):
    from model.BERTgrid_generator import BERTgridGenerator
    u8, coors, sizes = mixed
    d = dev()
    imgs = [x.to(d) for x in _fp32(u8)]
    dcoors = [c.to(d) for c in coors]
    ref = torch.zeros((4, H, W, 3), device=d)
    rc = []
    for b, (im, (oh, ow)) in enumerate(zip(imgs, sizes)):
        ops.normalize_resize(im, oh, ow, MEAN, STD, ref, b)
        h, w = im.shape[-2:]
        rc.append(ops.rescale_boxes(dcoors[b], oh / h, ow / w))
    rboxes, roff, rdoc = BERTgridGenerator.pack_boxes(tuple(rc))
    batch, boxes, off, doc = _call(ops, imgs, sizes, dcoors)
    assert _same_bits(batch, ref)                                # resized region and the +0.0 padding, bit for bit
    assert _same_bits(boxes, rboxes) and _same_bits(off, roff) and _same_bits(doc, rdoc)
    for b, (oh, ow) in enumerate(sizes):                         # (said again, without the reference: the padding is +0.0)
        pad = batch[b].clone()
        pad[:oh, :ow] = 0
        assert not _bits(pad).any()


def test_b_uint8_chw_bitwise_against_fp32_of_the_cpu_division(ops, mixed):
    u8, coors, sizes = mixed
    d = dev()
    dcoors = [c.to(d) for c in coors]
    ref = _call(ops, [x.to(d) for x in _fp32(u8)], sizes, dcoors)
    got = _call(ops, [u.to(d) for u in u8], sizes, dcoors)
    assert all(_same_bits(a, b) for a, b in zip(got, ref))
    # the 16 x 16 block of all byte values, identity path: 256 distinct normalised values per channel, each the CPU's bits
    blk = got[0][2, :16, :16].cpu()
    for c in range(3):
        want = (torch.arange(256, dtype=torch.uint8).float().div(255) - torch.tensor(MEAN[c])) / torch.tensor(STD[c])
        assert torch.equal(blk[..., c].reshape(-1).view(torch.int32), want.view(torch.int32))


def test_c_uint8_hwc_view_bitwise_against_uint8_chw(ops, mixed):
    u8, coors, sizes = mixed
    d = dev()
    dcoors = [c.to(d) for c in coors]
    ref = _call(ops, [u.to(d) for u in u8], sizes, dcoors)
    # a decoded image as it lies in memory, [h, w, 3], seen through permute: rows of 3 * 53 and 3 * 7 bytes start unaligned.  One
    # device buffer with a one-byte lead, so not even the first row is aligned.
    views = []
    for u in u8:
        hwc = u.permute(1, 2, 0).contiguous()
        raw = torch.empty(hwc.numel() + 1, dtype=torch.uint8, device=d)
        raw[1:] = hwc.reshape(-1).to(d)
        v = raw[1:].view(hwc.shape).permute(2, 0, 1)
        views.append(v)
    assert [ops.transform_input(v)[1] for v in views] == [2, 2, 2, 2]
    assert all(ops.transform_input(v)[0].data_ptr() == v.data_ptr() for v in views)          # read in place
    got = _call(ops, views, sizes, dcoors)
    assert all(_same_bits(a, b) for a, b in zip(got, ref))
    # mixed formats in one launch
    fp = _fp32(u8)
    got = _call(ops, [fp[0].to(d), views[1], u8[2].to(d), views[3]], sizes, dcoors)
    assert all(_same_bits(a, b) for a, b in zip(got, ref))


@pytest.mark.parametrize("fmt", [R.F32_CHW, R.U8_CHW, R.U8_HWC])
def test_d_against_the_restatement(ops, mixed, fmt):
    u8, coors, sizes = mixed
    d = dev()
    if fmt == R.F32_CHW:
        host = [x.numpy() for x in _fp32(u8)]
        imgs = [torch.from_numpy(x).to(d) for x in host]
    elif fmt == R.U8_CHW:
        host = [u.numpy() for u in u8]
        imgs = [u.to(d) for u in u8]
    else:
        host = [np.ascontiguousarray(u.permute(1, 2, 0).numpy()) for u in u8]
        imgs = [torch.from_numpy(x).to(d).permute(2, 0, 1) for x in host]
    rb, rboxes, roff, rdoc = R.transform_batch(host, [fmt] * 4, sizes, MEAN, STD, H, W, [c.numpy() for c in coors])
    batch, boxes, off, doc = _call(ops, imgs, sizes, [c.to(d) for c in coors])
    got = batch.cpu().numpy()
    for b, ((h, w), (oh, ow)) in enumerate(CASES):
        tol = 1e-6 if (h, w) == (oh, ow) else 1e-4
        err = float(np.abs(got[b] - rb[b]).max())
        print(f"format {fmt} image {b}: max abs err {err:.3e} (tolerance {tol:g})")
        assert np.allclose(got[b], rb[b], rtol=tol, atol=tol)
    assert np.array_equal(boxes.cpu().numpy(), rboxes)
    assert np.array_equal(off.cpu().numpy(), roff) and np.array_equal(doc.cpu().numpy(), rdoc)


def test_e_across_the_launch_boundary(ops):
    B = ops.TRANSFORM_MAX_IMAGES + 1
    rs = np.random.RandomState(5)
    d = dev()
    u8 = [torch.from_numpy(rs.randint(0, 256, size=(3, 2, 3)).astype(np.uint8)) for _ in range(B)]
    coors = [torch.from_numpy(rs.randint(0, 4, size=(2, 4)).astype(np.int64)) for _ in range(B)]
    sizes = [((2, 3) if b % 3 == 0 else (3, 5)) for b in range(B)]
    Hh, Ww = 4, 6
    host, fmts, imgs = [], [], []
    for b, u in enumerate(u8):
        fmt = b % 3
        fmts.append(fmt)
        if fmt == R.F32_CHW:
            host.append(u.float().div(255).numpy())
            imgs.append(torch.from_numpy(host[-1]).to(d))
        elif fmt == R.U8_CHW:
            host.append(u.numpy())
            imgs.append(u.to(d))
        else:
            host.append(np.ascontiguousarray(u.permute(1, 2, 0).numpy()))
            imgs.append(torch.from_numpy(host[-1]).to(d).permute(2, 0, 1))
    rb, rboxes, roff, rdoc = R.transform_batch(host, fmts, sizes, MEAN, STD, Hh, Ww, [c.numpy() for c in coors])
    batch, boxes, off, doc = _call(ops, imgs, sizes, [c.to(d) for c in coors], Hh, Ww)
    got = batch.cpu().numpy()
    assert not np.isnan(got).any()
    assert np.allclose(got, rb, rtol=1e-4, atol=1e-4)            # every slot, the one behind the boundary included
    for b, (oh, ow) in enumerate(sizes):
        pad = got[b].copy()
        pad[:oh, :ow] = 0
        assert not pad.view(np.uint32).any(), b
    assert np.array_equal(boxes.cpu().numpy(), rboxes)
    assert np.array_equal(off.cpu().numpy(), roff) and off.cpu().tolist() == list(range(0, 2 * B + 1, 2))
    assert np.array_equal(doc.cpu().numpy(), rdoc)


def test_f_through_the_transform_class(ops, golden):
    from pipeline.transform import GeneralizedViBERTgridTransform
    g = golden("transform.npz")
    d = dev()
    tr = GeneralizedViBERTgridTransform(MEAN, STD, [48, 64], 56, 80)
    imgs = tuple(torch.from_numpy(g[f"img{i}"]).to(d) for i in range(3))
    coors = tuple(torch.from_numpy(g[f"coor{i}"]).to(d) for i in range(3))
    u8 = tuple((torch.from_numpy(g[f"img{i}"]) * 255).round().clamp(0, 255).to(torch.uint8) for i in range(3))
    q01 = tuple(u.float().div(255).to(d) for u in u8)            # the bytes' floats, divided on the CPU
    was = ops.transform_batch_enabled()
    try:
        for mode, seed in (("eval", None), ("train", 123)):
            getattr(tr, mode)()
            res = {}
            for on in (True, False):
                ops.set_transform_batch(on)
                if seed is not None:
                    torch.manual_seed(seed)
                res[on] = tr.forward_packed(imgs, coors)
                draws_after = torch.rand(1).item() if seed is not None else None
                res[on] += (draws_after,)
            (b1, c1, s1, p1, r1), (b0, c0, s0, p0, r0) = res[True], res[False]
            assert s1 == s0 and np.array_equal(np.array(s1), g[mode + "_sizes"]) and r1 == r0       # same draws, same generator state after
            assert _same_bits(b1, b0)
            assert all(_same_bits(a, b) for a, b in zip(p1, p0))          # boxes, box_off, box_doc
            ref = torch.from_numpy(g[mode + "_batch"]).permute(0, 2, 3, 1)
            assert torch.allclose(b1.cpu(), ref, rtol=1e-4, atol=1e-4)
            for i in range(3):
                for c in (c1[i], c0[i]):
                    assert c.dtype == torch.int32 and c.shape == g[f"{mode}_coor{i}"].shape
                    assert np.array_equal(c.cpu().numpy(), g[f"{mode}_coor{i}"])                  # bit exact against the reference
            # forward_nhwc and forward keep their conventions
            if seed is not None:
                torch.manual_seed(seed)
            il, oc = tr(imgs, coors)
            assert _same_bits(il.tensors, b1.permute(0, 3, 1, 2).contiguous()) and [tuple(s) for s in il.image_sizes] == [tuple(s) for s in s1]
            # bytes: the batched entry whatever the switch says, equal to the fp32 route on the bytes' floats
            for on in (True, False):
                ops.set_transform_batch(on)
                if seed is not None:
                    torch.manual_seed(seed)
                bq, cq, sq, pq = tr.forward_packed(q01, coors)
                if seed is not None:
                    torch.manual_seed(seed)
                bu, cu, su, pu = tr.forward_packed(tuple(u.to(d) for u in u8), coors)
                assert su == sq and _same_bits(bu, bq) and all(_same_bits(a, b) for a, b in zip(pu, pq))
        # an image without boxes: None in the list, nothing packed
        tr.eval()
        for on in (True, False):
            ops.set_transform_batch(on)
            b, c, s, p = tr.forward_packed(imgs, (coors[0], None, coors[2]))
            assert p is None and c[1] is None and np.array_equal(c[2].cpu().numpy(), g["eval_coor2"])
            assert torch.allclose(b.cpu(), torch.from_numpy(g["eval_batch"]).permute(0, 2, 3, 1), rtol=1e-4, atol=1e-4)
    finally:
        ops.set_transform_batch(was)


def test_g_small_model_forward_from_bytes(ops, golden, tmp_path):
    import random
    from test_gpu_model import build_product, load_synth, to_dev
    from test_oracle_golden import _e2e_inputs, e2e_cfg
    g = golden("e2e.npz")
    cfg = e2e_cfg("resnet_18_fpn")
    d = dev()
    net = build_product(tmp_path, "resnet_18_fpn", cfg)
    load_synth(net, cfg, 1200)
    net = net.to(d).eval()
    imgs, segs, classes, coors, corpus, mask = _e2e_inputs(g)
    u8 = [(im * 255).round().clamp(0, 255).to(torch.uint8) for im in imgs]
    q01 = [u.float().div(255) for u in u8]
    random.seed(7)
    with torch.no_grad():
        ref = net(*to_dev((q01, segs, classes, coors, corpus, mask), d))
    random.seed(7)
    with torch.no_grad():
        got = net(*to_dev((u8, segs, classes, coors, corpus, mask), d))
    assert len(ref) == len(got) and all(torch.equal(a, b) for a, b in zip(ref, got))
