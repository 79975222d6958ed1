"""PNG files encoded on the device: 8-bit L planes (masks) and RGBA images (a packed RGB image plus a separate alpha plane; no RGBA
buffer is ever made) become complete files by csrc/png.hip (``dm4d_png_encode_u8``): filter, deflate, chunk CRC-32s, zlib header and
Adler-32 are all computed there, and only the files' bytes cross PCIe.  The host stores them verbatim.

The files are valid PNGs whose decoded pixels are exactly the input; their bytes are not Pillow's (zlib's match search is not
reproduced).  They are defined by tests/png_model.py, which the device equals byte for byte ("Device PNG").  There is no
CPU path: a host tensor is an error.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch

from . import codec as _c
from . import lib as _l
from . import ops

DEFAULT_WORKSPACE = 1 << 30
L, RGBA = _l.PNG_L, _l.PNG_RGBA


def stripe_rows(h: int, w: int, channels: int) -> int:
    """Rows of one stripe (= one deflate block = one IDAT chunk) of an h x w image; a function of the size and kind alone."""
    return max(1, _l.PNG_STRIPE_BYTES // (1 + w * channels))


def n_stripes(h: int, w: int, channels: int) -> int:
    rows = stripe_rows(h, w, channels)
    return (h + rows - 1) // rows


def _device_bytes(h: int, w: int, channels: int) -> int:
    """Device bytes one image of a call needs besides its pixels: filtered stream + tokens + stripe records + its share of the blob."""
    filt = h * (1 + w * channels)
    return 3 * filt + n_stripes(h, w, channels) * (_l.PNG_STRIPE_REC + 4) + 64 + 64 + 576 * n_stripes(h, w, channels) + 2 * filt


def png_encode_planes(planes: torch.Tensor, rgb: Optional[torch.Tensor], items: Sequence[Tuple]) -> List[bytes]:
    """The PNG files of images that already lie in device buffers the caller owns.

    planes: device uint8 [bytes], the L planes and the alpha planes; rgb: device uint8 [bytes] with the packed RGB images, or None.
    items: ``(L, h, w, plane offset, row stride)`` or ``(RGBA, h, w, rgb offset, rgb row stride, alpha offset, alpha row stride)``,
    offsets and strides in bytes.  One call of the library (five launches), one synchronisation (the lengths) and one copy of exactly
    the bytes produced."""
    lib = _l.load()
    n = len(items)
    if n < 1:
        raise ValueError("items: at least one image")
    desc = torch.zeros((n, _l.PNG_FIELDS), dtype=torch.int64)
    filt0 = stripe0 = bound = 0
    for k, it in enumerate(items):
        kind, h, w = int(it[0]), int(it[1]), int(it[2])
        ch = 4 if kind == RGBA else 1
        b = int(lib.dm4d_png_bound(h, w, ch))
        if kind not in (L, RGBA) or b == 0 or len(it) != (7 if kind == RGBA else 5):
            raise _l.Dm4dError(f"items[{k}]: {it!r} is no L or RGBA image of a side in 1..{_l.MATTING_MAX_SIDE}")
        desc[k, :3] = torch.tensor([kind, h, w])
        desc[k, 3:3 + len(it) - 3] = torch.tensor([int(v) for v in it[3:]])
        desc[k, 7], desc[k, 8] = filt0, stripe0
        filt0, stripe0, bound = filt0 + h * (1 + w * ch), stripe0 + n_stripes(h, w, ch), bound + b
    ws_bytes = int(lib.dm4d_png_ws_bytes(filt0, stripe0, n))
    if ws_bytes == 0:
        raise _l.Dm4dError(f"png_encode_planes: {n} images with {filt0} filtered bytes are out of range for one call")
    with torch.cuda.device(planes.device):
        return _c.read_back(*ops.png_encode(planes, rgb, desc, bound, ws_bytes))


def encode_png_batch(planes, alphas: Optional[Sequence] = None, workspace_bytes: int = DEFAULT_WORKSPACE) -> List[bytes]:
    """Device uint8 tensors (any sizes) -> their PNG files, as bytes.

    planes[k]: [h, w] -> an L file; [h, w, 3] with alphas[k] = [h, w] -> an RGBA file (alphas: None, or per image None or the alpha
    plane).  Rows must be contiguous; a row stride larger than the row (a view of a wider buffer) is read in place when all tensors of
    a kind share one storage, otherwise the images are gathered first.  The batch is processed in chunks whose device memory stays
    below `workspace_bytes` (a chunk holds at least one image); one synchronisation and one device-to-host copy per chunk."""
    planes = list(planes)
    alphas = [None] * len(planes) if alphas is None else list(alphas)
    if len(alphas) != len(planes):
        raise ValueError(f"alphas: {len(alphas)} entries for {len(planes)} images")
    if not planes:
        return []
    shapes = []
    for k, (p, a) in enumerate(zip(planes, alphas)):
        for name, t in ((f"planes[{k}]", p), (f"alphas[{k}]", a)):
            if t is not None:
                _c.require_device_u8(t, name)
        rgba = a is not None
        if p.dim() != (3 if rgba else 2) or (rgba and (p.shape[2] != 3 or tuple(a.shape) != tuple(p.shape[:2]))):
            raise _l.Dm4dError(f"planes[{k}]: expected [h, w], or [h, w, 3] with an [h, w] alpha plane, got {tuple(p.shape)}")
        h, w = int(p.shape[0]), int(p.shape[1])
        if not (1 <= h <= _l.MATTING_MAX_SIDE and 1 <= w <= _l.MATTING_MAX_SIDE):
            raise ValueError(f"planes[{k}]: size {w} x {h} is outside 1..{_l.MATTING_MAX_SIDE}")
        shapes.append((h, w, 4 if rgba else 1))
    dev = planes[0].device
    files: List[bytes] = []
    for first, last in _c.chunks([_device_bytes(h, w, ch) + h * w * ch for h, w, ch in shapes], workspace_bytes):
        with torch.cuda.device(dev):
            ones = [alphas[k] if alphas[k] is not None else planes[k] for k in range(first, last)]   # 1 byte per pixel
            threes = [planes[k] for k in range(first, last) if alphas[k] is not None]                # 3 bytes per pixel
            pbuf, pat = _c.gather(ones, 1)
            rbuf, rat = _c.gather(threes, 3) if threes else (None, [])
            items, r = [], 0
            for j, k in enumerate(range(first, last)):
                h, w, ch = shapes[k]
                if ch == 1:
                    items.append((L, h, w) + pat[j])
                else:
                    items.append((RGBA, h, w) + rat[r] + pat[j])
                    r += 1
            files += png_encode_planes(pbuf, rbuf, items)
    return files
