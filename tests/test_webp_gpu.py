"""GPU: the device lossless-WebP encoder (csrc/webp.hip through host/webp.py) equals its definition tests/webp_model.py byte for byte: one
mixed batch of every case of tests/webp_cases.py, the images at odd offsets and padded row strides inside one buffer; every image alone
(batch invariance); a second call (repeatability); strided views against gathered copies; the chunked public entry."""
import functools
import io

import numpy as np
import pytest
import torch
from PIL import Image

import webp_cases
import webp_model as M
from diffuman4d_amd.host import lib as L
from diffuman4d_amd.host import webp

pytestmark = pytest.mark.gpu
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def cases():
    cs = webp_cases.cases()
    names = sorted(cs)
    return names, [cs[k] for k in names], [M.encode(cs[k]) for k in names]


@functools.lru_cache(maxsize=None)
def staged():
    """(rgb buffer, items): every image starts at an odd offset and its rows are 1 + 3 k bytes further apart than they are long; the
    bytes between them are 0xA5 so that a read outside a row shows."""
    _, imgs, _ = cases()
    parts, items, at = [np.full(5, 0xA5, np.uint8)], [], 5
    for k, a in enumerate(imgs):
        h, w = a.shape[:2]
        pad = 1 + 3 * (k % 4)
        region = np.full((h, 3 * w + pad), 0xA5, np.uint8)
        region[:, :3 * w] = a.reshape(h, 3 * w)
        tail = np.full(2 - (region.size & 1), 0xA5, np.uint8)  # keeps the next offset odd
        parts += [region.reshape(-1), tail]
        items.append((h, w, at, 3 * w + pad))
        at += region.size + tail.size
    assert all(it[2] & 1 for it in items)
    return torch.from_numpy(np.concatenate(parts)).to(DEV), items


@functools.lru_cache(maxsize=None)
def batch_files():
    return webp.webp_encode_planes(*staged())


def test_mixed_batch_equals_the_model():
    names, imgs, model = cases()
    files = batch_files()
    assert len(files) == len(model)
    for name, img, got, want in zip(names, imgs, files, model):
        assert got == want, f"{name}: {len(got)} bytes, the model has {len(want)}"
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(got))), img), name


def test_each_image_alone_and_a_second_call_give_the_same_bytes():
    rgb, items = staged()
    files = batch_files()
    assert webp.webp_encode_planes(rgb, items) == files
    for k, it in enumerate(items):
        assert webp.webp_encode_planes(rgb, [it]) == [files[k]], cases()[0][k]


def test_strided_views_of_one_buffer_against_gathered_copies():
    """Windows of a wider tensor: the row stride is larger than the row; read in place, they give what their copies give."""
    rng = np.random.default_rng(8)
    wide = rng.integers(0, 256, (120, 90, 3), dtype=np.uint8)
    wide[30:100, 20:70] = (3, 3, 3)
    wide_d = torch.from_numpy(wide).to(DEV)
    views = [wide_d[3:20, 5:22], wide_d[0:120, 1:2], wide_d[10:11, 0:90], wide_d[25:110, 10:80]]
    got = webp.encode_webp_batch(views)
    assert got == [M.encode(v.cpu().numpy()) for v in views]
    assert got == webp.encode_webp_batch([v.contiguous() for v in views])
    assert got == webp.encode_webp_batch([v.clone() for v in views])  # different storages: gathered


def test_public_entry_chunked_by_a_tiny_budget():
    names, imgs, model = cases()
    images = [torch.from_numpy(a).to(DEV) for a in imgs]
    assert webp.encode_webp_batch(images, workspace_bytes=1) == model  # one image per call
    assert webp.encode_webp_batch(images, workspace_bytes=1 << 20) == model
    assert webp.encode_webp_batch(images) == model
    assert webp.encode_webp_batch([]) == []
    with pytest.raises(L.Dm4dError, match="HIP device"):
        webp.encode_webp_batch([images[0].cpu()])
    with pytest.raises(L.Dm4dError, match="uint8"):
        webp.encode_webp_batch([images[0].float()])
    with pytest.raises(L.Dm4dError, match=r"\[h, w, 3\]"):
        webp.encode_webp_batch([images[0][:, :, 0]])
