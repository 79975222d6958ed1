"""Result JPEGs encoded on the device: ``images/{cam}/{frame}.jpg`` of the sampler's result contract without the host's Pillow work.

``encode_jpeg_batch`` takes finished uint8 HWC images that live on the GPU, undoes the dataset's crop there
(``imgwrite.restore_cropped_image``: bicubic resize + paste onto a white canvas, ``dm4d_restore_crop_u8``) and runs the baseline JPEG
encoder of csrc/jpeg.hip on the canvases (``dm4d_jpeg_encode_rgb_u8``).  One blob of entropy-coded bytes per chunk of the batch
crosses PCIe; the host only concatenates header + scan + EOI.  The files are byte for byte what
``restore_cropped_image(Image.fromarray(a), crop).save(path, quality=q)`` writes ("Device JPEG"; tests/jpeg_model.py is the
definition in numpy).  There is no CPU path: a host tensor is an error.

The tables are those of ITU-T T.81 Annex K (K.1, K.2 quantisation; K.3 - K.6 Huffman), which is what libjpeg writes by default.
"""
from __future__ import annotations

import struct
from typing import List, Optional, Sequence, Tuple

import torch

from . import codec as _c
from . import lib as _l
from .ops import _p, _req, _stream
from .resample import TableSet

# -- Annex K ------------------------------------------------------------------------------------------------------------------------
QUANT_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
              18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100,
              103, 99)
QUANT_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                ) + (99,) * 32
# (number of codes of length 1..16, symbols in code order)
DC_LUMA = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12)))
DC_CHROMA = ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12)))
AC_LUMA = ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D), bytes.fromhex(
    "01 02 03 00 04 11 05 12 21 31 41 06 13 51 61 07 22 71 14 32 81 91 a1 08 23 42 b1 c1 15 52 d1 f0"
    "24 33 62 72 82 09 0a 16 17 18 19 1a 25 26 27 28 29 2a 34 35 36 37 38 39 3a 43 44 45 46 47 48 49"
    "4a 53 54 55 56 57 58 59 5a 63 64 65 66 67 68 69 6a 73 74 75 76 77 78 79 7a 83 84 85 86 87 88 89"
    "8a 92 93 94 95 96 97 98 99 9a a2 a3 a4 a5 a6 a7 a8 a9 aa b2 b3 b4 b5 b6 b7 b8 b9 ba c2 c3 c4 c5"
    "c6 c7 c8 c9 ca d2 d3 d4 d5 d6 d7 d8 d9 da e1 e2 e3 e4 e5 e6 e7 e8 e9 ea f1 f2 f3 f4 f5 f6 f7 f8"
    "f9 fa"))
AC_CHROMA = ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77), bytes.fromhex(
    "00 01 02 03 11 04 05 21 31 06 12 41 51 07 61 71 13 22 32 81 08 14 42 91 a1 b1 c1 09 23 33 52 f0"
    "15 62 72 d1 0a 16 24 34 e1 25 f1 17 18 19 1a 26 27 28 29 2a 35 36 37 38 39 3a 43 44 45 46 47 48"
    "49 4a 53 54 55 56 57 58 59 5a 63 64 65 66 67 68 69 6a 73 74 75 76 77 78 79 7a 82 83 84 85 86 87"
    "88 89 8a 92 93 94 95 96 97 98 99 9a a2 a3 a4 a5 a6 a7 a8 a9 aa b2 b3 b4 b5 b6 b7 b8 b9 ba c2 c3"
    "c4 c5 c6 c7 c8 c9 ca d2 d3 d4 d5 d6 d7 d8 d9 da e2 e3 e4 e5 e6 e7 e8 e9 ea f2 f3 f4 f5 f6 f7 f8"
    "f9 fa"))


def _zigzag() -> Tuple[int, ...]:
    order = sorted(range(64), key=lambda i: (i // 8 + i % 8, i // 8 if (i // 8 + i % 8) & 1 else i % 8))
    return tuple(order)


ZIGZAG = _zigzag()  # ZIGZAG[k] = natural (row-major) index of the k-th coefficient of the scan

DEFAULT_WORKSPACE = 1 << 30


def _check_quality(quality) -> int:
    if isinstance(quality, bool) or int(quality) != quality or not 1 <= int(quality) <= 100:
        raise ValueError(f"quality: expected an integer in 1..100, got {quality!r}")
    return int(quality)


def quant_tables(quality: int) -> Tuple[Tuple[int, ...], Tuple[int, ...]]:
    """The luma and chroma tables (natural order) libjpeg's jpeg_set_quality(q, force_baseline) derives from Annex K."""
    q = _check_quality(quality)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(tuple(min(max((b * s + 50) // 100, 1), 255) for b in base) for base in (QUANT_LUMA, QUANT_CHROMA))


def jpeg_header(h: int, w: int, quality: int) -> bytes:
    """Everything of the file before the entropy-coded segment: SOI, JFIF APP0, two DQT, SOF0 (4:2:0), four DHT, SOS."""
    if not (1 <= int(h) <= 65535 and 1 <= int(w) <= 65535):
        raise ValueError(f"jpeg_header: image size {w} x {h} outside 1..65535")
    out = [b"\xff\xd8", b"\xff\xe0" + struct.pack(">H5sBBBHHBB", 16, b"JFIF\0", 1, 1, 0, 1, 1, 0, 0)]
    for i, tab in enumerate(quant_tables(quality)):
        out.append(b"\xff\xdb" + struct.pack(">HB", 67, i) + bytes(tab[z] for z in ZIGZAG))
    out.append(b"\xff\xc0" + struct.pack(">HBHHB", 17, 8, int(h), int(w), 3) + bytes((1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1)))
    for tc_th, (bits, vals) in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out.append(b"\xff\xc4" + struct.pack(">HB", 19 + len(vals), tc_th) + bytes(bits) + bytes(vals))
    out.append(b"\xff\xda" + struct.pack(">HB", 12, 3) + bytes((1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0)))
    return b"".join(out)


def canvas_size(h: int, w: int, crop: Optional[Sequence[int]]) -> Tuple[int, int]:
    """(height, width) of what restore_cropped_image returns for an h x w image."""
    if crop is None or len(crop) == 4:
        return int(h), int(w)
    if len(crop) == 6:
        return int(crop[4]), int(crop[5])
    raise ValueError(f"Invalid crop_param: {tuple(crop)}")


def _mcus(h: int, w: int) -> int:
    return ((h + 15) // 16) * ((w + 15) // 16)


def _image_bytes(img, crop, hw) -> int:
    """Device bytes one image of a batch needs: canvas + resize scratch + encoder workspace + its share of the blob."""
    m = _mcus(*hw)
    n = m * (768 + 8 + _l.JPEG_MCU_UNSTUFFED + _l.JPEG_MCU_BOUND) + 64
    if crop is not None:
        n += _l.align16(hw[0] * hw[1] * 3) + _l.align16(img.shape[0] * int(crop[3]) * 3)
    return n


def restore_crops(pixels: torch.Tensor, items, device) -> Tuple[torch.Tensor, list]:
    """``imgwrite.restore_cropped_image`` of a batch on the device (dm4d_restore_crop_u8, two launches): items = [(byte offset of the
    uint8 [H, W, 3] image in `pixels`, H, W, (ct, cl, ch, cw), (canvas h, canvas w))] -> (uint8 buffer of the canvases, their byte
    offsets in it).  The coefficient tables are Pillow's (host/resample.py)."""
    _req(pixels, "pixels", torch.uint8)
    desc = torch.zeros((len(items), _l.RESTORE_FIELDS), dtype=torch.int64)
    tables, scratch_len, canvas_len, places = TableSet(), 0, 0, []
    for i, (src, H, W, (ct, cl, ch, cw), (h, w)) in enumerate(items):
        htab, hk = tables.add(W, cw)
        vtab, vk = tables.add(H, ch)
        desc[i, :15] = torch.tensor([src, H, W, ct, cl, ch, cw, h, w, htab, hk, vtab, vk, scratch_len, canvas_len])
        places.append(canvas_len)
        scratch_len += _l.align16(H * cw * 3)
        canvas_len += _l.align16(h * w * 3)
    tab = torch.from_numpy(tables.array())
    scratch = torch.empty(scratch_len, dtype=torch.uint8, device=device)
    canvases = torch.empty(canvas_len, dtype=torch.uint8, device=device)
    desc_dev, tab_dev = desc.to(device), tab.to(device)
    _l.call("dm4d_restore_crop_u8", _stream(), _p(pixels), pixels.numel(), desc.data_ptr(), _p(desc_dev), len(items), tab.data_ptr(),
            _p(tab_dev), tab.numel(), _p(scratch), scratch.numel(), _p(canvases), canvases.numel())
    return canvases, places


def jpeg_encode_chunk(images, crops, sizes, qtab) -> list:
    """Entropy-coded JPEG segments (bytes) of device uint8 [H, W, 3] tensors, each first restored onto its canvas where crops[k] is
    not None (sizes[k] = the canvas' (h, w)); qtab: 128 integers, luma then chroma quantisation table in natural order.
    Images that are views of one storage are read in place, otherwise they are gathered into one buffer first.  One host
    synchronisation (the lengths) and one copy of exactly the bytes produced."""
    lib = _l.load()
    dev = images[0].device
    for k, img in enumerate(images):
        _req(img, f"images[{k}]", torch.uint8)
        if img.device != dev or img.dim() != 3 or img.shape[2] != 3 or not img.is_contiguous():
            raise _l.Dm4dError(f"images[{k}]: expected a contiguous uint8 [H, W, 3] tensor on {dev}, got {tuple(img.shape)} on {img.device}")
    with torch.cuda.device(dev):
        pixels, at = _c.gather(images, 3)
        at = [off for off, _ in at]  # the images are contiguous: a row stride is the row
        n = len(images)
        cropped = [k for k in range(n) if crops[k] is not None]
        canvases, places = None, {}
        if cropped:
            canvases, where = restore_crops(pixels, [(at[k], images[k].shape[0], images[k].shape[1], tuple(crops[k][:4]), sizes[k])
                                                     for k in cropped], dev)
            places = dict(zip(cropped, where))
        desc = torch.zeros((n, _l.JPEG_FIELDS), dtype=torch.int64)
        mcu0 = chunk0 = bound = 0
        for k, (h, w) in enumerate(sizes):
            mcus = ((h + 15) // 16) * ((w + 15) // 16)
            b = int(lib.dm4d_jpeg_scan_bound(h, w))
            if b == 0:
                raise _l.Dm4dError(f"images[{k}]: size {h} x {w} is out of range for the JPEG encoder")
            desc[k, :6] = torch.tensor([1, places[k], h, w, mcu0, chunk0] if k in places else [0, at[k], h, w, mcu0, chunk0])
            mcu0, chunk0, bound = mcu0 + mcus, chunk0 + (mcus * _l.JPEG_MCU_UNSTUFFED + _l.JPEG_CHUNK - 1) // _l.JPEG_CHUNK, bound + b
        nbytes = int(lib.dm4d_jpeg_ws_bytes(mcu0, n))
        if nbytes == 0:
            raise _l.Dm4dError(f"jpeg_encode_chunk: {n} images with {mcu0} MCUs are out of range for one call")
        ws = _c.workspace(nbytes, dev)
        blob = torch.empty(bound, dtype=torch.uint8, device=dev)
        out = torch.empty(2 * n, dtype=torch.int64, device=dev)
        q = torch.tensor([int(v) for v in qtab], dtype=torch.int16)  # values 1..255: the same bytes as uint16
        desc_dev, q_dev = desc.to(dev), q.to(dev)
        _l.call("dm4d_jpeg_encode_rgb_u8", _stream(), _p(pixels) if pixels.numel() else None, pixels.numel(), _p(canvases),
                0 if canvases is None else canvases.numel(), desc.data_ptr(), _p(desc_dev), n, q.data_ptr(), _p(q_dev), _p(ws),
                ws.numel() * 8, _p(blob), blob.numel(), _p(out))
        return _c.read_back(blob, out)


def encode_jpeg_batch(images, quality: int = 90, crops: Optional[Sequence] = None, workspace_bytes: int = DEFAULT_WORKSPACE) -> List[bytes]:
    """Device uint8 [H, W, 3] tensors (any sizes) -> the JPEG files Pillow writes for them at `quality`, as bytes.

    crops: per image None or the dataset's ``(ct, cl, ch, cw[, h, w])``: the image is first restored onto its white canvas on the
    device.  The batch is processed in chunks whose device memory stays below `workspace_bytes` (a chunk holds at least one image).
    One synchronisation and one device-to-host copy per chunk."""
    q = _check_quality(quality)
    images = list(images)
    crops = [None] * len(images) if crops is None else [None if c is None else tuple(int(v) for v in c) for c in crops]
    if len(crops) != len(images):
        raise ValueError(f"crops: {len(crops)} entries for {len(images)} images")
    sizes = []
    for k, (img, crop) in enumerate(zip(images, crops)):
        _c.require_device_u8(img, f"images[{k}]")
        if img.dim() != 3 or img.shape[2] != 3 or not img.is_contiguous():
            raise _l.Dm4dError(f"images[{k}]: expected a contiguous uint8 [H, W, 3] tensor, got {img.dtype} {tuple(img.shape)}")
        if crop is not None and (len(crop) not in (4, 6) or crop[2] < 1 or crop[3] < 1):
            raise ValueError(f"Invalid crop_param: {crop}")
        hw = canvas_size(img.shape[0], img.shape[1], crop)
        if not (1 <= hw[0] <= 65535 and 1 <= hw[1] <= 65535 and 1 <= img.shape[0] <= 65535 and 1 <= img.shape[1] <= 65535):
            raise ValueError(f"images[{k}]: size {tuple(img.shape[:2])} -> canvas {hw} outside 1..65535")
        sizes.append(hw)
    files: List[bytes] = []
    qtab = [v for tab in quant_tables(q) for v in tab]
    for first, last in _c.chunks([_image_bytes(*it) for it in zip(images, crops, sizes)], workspace_bytes):
        scans = jpeg_encode_chunk(images[first:last], crops[first:last], sizes[first:last], qtab)
        files += [jpeg_header(hw[0], hw[1], q) + s + b"\xff\xd9" for hw, s in zip(sizes[first:last], scans)]
    return files
