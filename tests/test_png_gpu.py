"""GPU: the device PNG encoder (csrc/png.hip through host/png.py) equals its definition tests/png_model.py byte for byte: one mixed
batch of every case of tests/png_cases.py in both kinds, with the planes at odd offsets and padded row strides inside one buffer and the
RGBA inputs as separate RGB and alpha buffers; every image alone (batch invariance); a second call (repeatability); the chunked public
entry; and an image with several stripes and workgroups live at once."""
import functools

import numpy as np
import pytest
import torch

import png_cases
import png_model as M
from diffuman4d_amd.host import lib as L
from diffuman4d_amd.host import png

pytestmark = pytest.mark.gpu
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def cases():
    cs = png_cases.cases()
    names = sorted(cs)
    return names, [cs[k] for k in names], [M.encode(cs[k]) for k in names]


@functools.lru_cache(maxsize=None)
def staged():
    """(planes buffer, rgb buffer, items): every plane starts at an odd offset and its rows are 1 + 3 k bytes further apart than they
    are long; the bytes between them are 0xA5 so that a read outside a row shows."""
    _, imgs, _ = cases()
    pbuf, rbuf, items = [np.full(3, 0xA5, np.uint8)], [np.full(5, 0xA5, np.uint8)], []
    plen, rlen = 3, 5

    def put(store, at, a, pad):
        h, rowbytes = a.shape[0], a[0].size
        region = np.full((h, rowbytes + pad), 0xA5, np.uint8)
        region[:, :rowbytes] = a.reshape(h, rowbytes)
        tail = np.full(2 - (region.size & 1), 0xA5, np.uint8)  # keeps the next offset odd
        store += [region.reshape(-1), tail]
        return at, rowbytes + pad, at + region.size + tail.size

    for k, a in enumerate(imgs):
        pad = 1 + 3 * (k % 4)
        if a.ndim == 2:
            off, stride, plen = put(pbuf, plen, a, pad)
            items.append((png.L, a.shape[0], a.shape[1], off, stride))
        else:
            roff, rstride, rlen = put(rbuf, rlen, np.ascontiguousarray(a[:, :, :3]), pad)
            aoff, astride, plen = put(pbuf, plen, np.ascontiguousarray(a[:, :, 3]), pad + 2)
            items.append((png.RGBA, a.shape[0], a.shape[1], roff, rstride, aoff, astride))
    assert all(it[3] & 1 for it in items)
    return torch.from_numpy(np.concatenate(pbuf)).to(DEV), torch.from_numpy(np.concatenate(rbuf)).to(DEV), items


@functools.lru_cache(maxsize=None)
def batch_files():
    planes, rgb, items = staged()
    return png.png_encode_planes(planes, rgb, items)


def test_mixed_batch_equals_the_model():
    names, _, model = cases()
    files = batch_files()
    assert len(files) == len(model)
    for name, got, want in zip(names, files, model):
        assert got == want, f"{name}: {len(got)} bytes, the model has {len(want)}"


def test_each_image_alone_and_a_second_call_give_the_same_bytes():
    planes, rgb, items = staged()
    files = batch_files()
    assert png.png_encode_planes(planes, rgb, items) == files
    for k, it in enumerate(items):
        assert png.png_encode_planes(planes, rgb, [it]) == [files[k]], cases()[0][k]


def test_public_entry_chunked_by_a_tiny_budget():
    names, imgs, model = cases()
    planes = [torch.from_numpy(np.ascontiguousarray(a if a.ndim == 2 else a[:, :, :3])).to(DEV) for a in imgs]
    alphas = [None if a.ndim == 2 else torch.from_numpy(np.ascontiguousarray(a[:, :, 3])).to(DEV) for a in imgs]
    assert png.encode_png_batch(planes, alphas, workspace_bytes=1) == model  # one image per call
    assert png.encode_png_batch(planes, alphas, workspace_bytes=1 << 20) == model
    assert png.encode_png_batch(planes, alphas) == model
    ls = [k for k, a in enumerate(imgs) if a.ndim == 2]
    assert png.encode_png_batch([planes[k] for k in ls]) == [model[k] for k in ls]
    with pytest.raises(L.Dm4dError, match="HIP device"):
        png.encode_png_batch([planes[0].cpu()])
    with pytest.raises(L.Dm4dError, match="HIP device"):
        k = next(k for k, a in enumerate(alphas) if a is not None)
        png.encode_png_batch([planes[k]], [alphas[k].cpu()])


def test_views_of_one_buffer_are_read_in_place():
    """Rows of a wider tensor: the row stride is larger than the row, and nothing is gathered."""
    rng = np.random.default_rng(8)
    wide = torch.from_numpy(rng.integers(0, 256, (40, 64), dtype=np.uint8)).to(DEV)
    views = [wide[3:20, 5:22], wide[0:40, 1:2], wide[10:11, 0:64]]
    assert png.encode_png_batch(views) == [M.encode(v.cpu().numpy()) for v in views]


def test_several_stripes_and_workgroups_at_once():
    rng = np.random.default_rng(9)
    rgb, mask = png_cases.result_like(520, 300)
    noisy, mask = rgb.copy(), mask.copy()
    noisy[100:140] = rng.integers(0, 256, (40, 300, 3), dtype=np.uint8)
    img = np.dstack([noisy, mask])
    assert M.n_stripes(520, 300, 4) >= 19
    got = png.encode_png_batch([torch.from_numpy(noisy).to(DEV)], [torch.from_numpy(mask).to(DEV)])
    assert got == [M.encode(img)]
    import io

    from PIL import Image
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(got[0]))), img)
