"""Lossless WebP files encoded on the device: packed 8-bit RGB images become complete files (RIFF framing and one VP8L chunk) by
csrc/webp.hip (``dm4d_webp_encode_u8``), and only the files' bytes cross PCIe.  The host stores them verbatim.

The files are valid WebP whose decoded pixels are exactly the input; their bytes are not libwebp's (its match search, predictors and
colour cache are not reproduced).  They are defined by tests/webp_model.py, which the device equals byte for byte ("Device
WebP (lossless)").  There is no CPU path: a host tensor is an error.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import torch

from . import codec as _c
from . import lib as _l
from . import ops

DEFAULT_WORKSPACE = 1 << 30


def n_stripes(h: int, w: int) -> int:
    """Stripes (the unit of the tokeniser and of the emitter) of an h x w image; a function of the size alone."""
    return (h * w + _l.WEBP_STRIPE_PIXELS - 1) // _l.WEBP_STRIPE_PIXELS


def _device_bytes(h: int, w: int) -> int:
    """Device bytes one image of a call needs besides its pixels: tokens + stripe records + its image record, bit offsets and seam bytes
    + its share of the blob."""
    s = n_stripes(h, w)
    return 2 * h * w + s * _l.WEBP_STRIPE_REC + _l.WEBP_IMAGE_REC + 16 * (s + 1) + 64 + 800 + 6 * h * w


def webp_encode_planes(rgb: torch.Tensor, items: Sequence[Tuple]) -> List[bytes]:
    """The WebP files of images that already lie in a device buffer the caller owns.

    rgb: device uint8 [bytes] with the packed RGB images; items: ``(h, w, byte offset, row stride in bytes)``.  One call of the library
    (five launches), one synchronisation (the lengths) and one copy of exactly the bytes produced."""
    lib = _l.load()
    n = len(items)
    if n < 1:
        raise ValueError("items: at least one image")
    desc = torch.zeros((n, _l.WEBP_FIELDS), dtype=torch.int64)
    pix0 = stripe0 = bound = 0
    for k, it in enumerate(items):
        if len(it) != 4:
            raise _l.Dm4dError(f"items[{k}]: {it!r} is not (h, w, offset, row stride)")
        h, w = int(it[0]), int(it[1])
        b = int(lib.dm4d_webp_bound(h, w))
        if b == 0:
            raise _l.Dm4dError(f"items[{k}]: {it!r} is no image of a side in 1..{_l.WEBP_MAX_SIDE}")
        desc[k, :6] = torch.tensor([h, w, int(it[2]), int(it[3]), pix0, stripe0])
        pix0, stripe0, bound = pix0 + h * w, stripe0 + n_stripes(h, w), bound + b
    ws_bytes = int(lib.dm4d_webp_ws_bytes(pix0, stripe0, n))
    if ws_bytes == 0:
        raise _l.Dm4dError(f"webp_encode_planes: {n} images with {pix0} pixels are out of range for one call")
    with torch.cuda.device(rgb.device):
        return _c.read_back(*ops.webp_encode(rgb, desc, bound, ws_bytes))


def encode_webp_batch(images, workspace_bytes: int = DEFAULT_WORKSPACE) -> List[bytes]:
    """Device uint8 tensors [h, w, 3] (any sizes) -> their lossless WebP files, as bytes.

    A pixel's three bytes and a row's pixels must be contiguous; a row stride larger than the row (a view of a wider buffer) is read in
    place when all tensors of a chunk share one storage, otherwise the images are gathered first.  The batch is processed in chunks
    whose device memory stays below `workspace_bytes` (a chunk holds at least one image); one synchronisation and one device-to-host
    copy per chunk."""
    images = list(images)
    if not images:
        return []
    shapes = []
    for k, t in enumerate(images):
        _c.require_device_u8(t, f"images[{k}]")
        if t.dim() != 3 or t.shape[2] != 3:
            raise _l.Dm4dError(f"images[{k}]: expected [h, w, 3], got {tuple(t.shape)}")
        h, w = int(t.shape[0]), int(t.shape[1])
        if not (1 <= h <= _l.WEBP_MAX_SIDE and 1 <= w <= _l.WEBP_MAX_SIDE):
            raise ValueError(f"images[{k}]: size {w} x {h} is outside 1..{_l.WEBP_MAX_SIDE}")
        shapes.append((h, w))
    files: List[bytes] = []
    for first, last in _c.chunks([_device_bytes(h, w) + 3 * h * w for h, w in shapes], workspace_bytes, _c.MAX_DECODE_CHUNK):
        with torch.cuda.device(images[first].device):
            buf, at = _c.gather(images[first:last], 3)
            files += webp_encode_planes(buf, [shapes[first + j] + at[j] for j in range(last - first)])
    return files
