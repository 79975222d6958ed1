"""The JPEG files the device decoder's tests share: written once per process by Pillow (and two by tests/jpeg_model.encode), named
after what they hold.  Sizes with partial and dummy blocks, one-pixel images, chroma planes too narrow for the triangle filter,
4:2:0 / 4:2:2 / 4:4:4 / grayscale, quality 30 / 90 / 100, standard and optimised Huffman tables, noise / smooth-plus-noise / all-white
content.  ``malformed()`` are three files of the supported set whose scans are broken, and ``unsupported()`` files ``probe`` refuses."""
from __future__ import annotations

import functools
import io
from typing import List, Tuple

import numpy as np
from PIL import Image

SIZES = [(1, 1), (7, 5), (17, 17), (37, 53), (2, 70), (50, 3), (20, 2), (9, 4), (40, 72)]
BIG = (320, 576)
CONTENTS = ("noise", "smooth", "white")
QUALITIES = (30, 90, 100)
SAMPLINGS = ("420", "422", "444", "gray")
_SUB = {"444": 0, "422": 1, "420": 2}


def content(kind: str, h: int, w: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "white":
        return np.full((h, w, 3), 255, dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 100 * np.sin(x / 9.0 + 1), 128 + 90 * np.cos(y / 7.0), 60 + 1.5 * (x + y)], axis=-1)
    return np.clip(base + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)


def save(a: np.ndarray, sampling: str, quality: int, optimize: bool, **kw) -> bytes:
    f = io.BytesIO()
    if sampling == "gray":
        Image.fromarray(a[..., 1]).save(f, "JPEG", quality=quality, optimize=optimize, **kw)
    else:
        Image.fromarray(a).save(f, "JPEG", quality=quality, optimize=optimize, subsampling=_SUB[sampling], **kw)
    return f.getvalue()


@functools.lru_cache(maxsize=None)
def supported() -> List[Tuple[str, bytes]]:
    from jpeg_model import encode
    out = []
    i = 0
    for h, w in SIZES:
        for sampling in SAMPLINGS:  # every size with every sampling; content, quality and tables rotate through their values
            kind, q, opt = CONTENTS[i % 3], QUALITIES[(i // 3) % 3], bool((i // 2) & 1)
            out.append((f"{h}x{w}-{sampling}-{kind}-q{q}-{'opt' if opt else 'std'}", save(content(kind, h, w, i), sampling, q, opt)))
            i += 1
    for kind in CONTENTS:  # 40 x 72 (the results of the golden demo): every content at every quality
        for q in QUALITIES:
            out.append((f"40x72-420-{kind}-q{q}-std-b", save(content(kind, 40, 72, 100 + i), "420", q, False)))
            i += 1
    out.append(("40x72-444-noise-q100-opt", save(content("noise", 40, 72, 7), "444", 100, True)))
    h, w = BIG  # result-sized files: more than one tile of subsequences
    out.append((f"{h}x{w}-420-smooth-q90-std", save(content("smooth", h, w, 1), "420", 90, False)))
    out.append((f"{h}x{w}-422-noise-q30-opt", save(content("noise", h, w, 2), "422", 30, True)))
    out.append(("37x53-model-q90", encode(content("smooth", 37, 53, 3), 90)))
    out.append(("40x72-model-q30", encode(content("noise", 40, 72, 4), 30)))
    return out


def _scan_range(data: bytes) -> Tuple[int, int]:
    from diffuman4d_amd.host.jpegdec import probe
    return probe(data).scan


@functools.lru_cache(maxsize=None)
def malformed() -> List[Tuple[str, bytes]]:
    """Files `probe` accepts and the decoder must refuse by status: a scan cut short (EOI kept), a flipped byte that leaves a window
    no Huffman code starts, and a DC difference that takes a dequantised coefficient out of [-8192, 8191]."""
    good = save(content("smooth", 40, 72, 11), "420", 90, False)
    s, e = _scan_range(good)
    cut = good[:s + (e - s) // 2] + good[e:]
    if cut[s + (e - s) // 2 - 1] == 0xFF:  # never end on half a stuffed pair
        cut = good[:s + (e - s) // 2 - 1] + good[e:]
    flipped = bytearray(good)
    at = s + 40
    while flipped[at - 1] == 0xFF:  # never split a stuffed pair
        at += 1
    flipped[at:at + 16] = b"\xff\x00" * 8  # 64 one-bits: a symbol starts with at least 16 of them ahead, and no code is 16 ones
    # all-white at quality 30: every block is a lone DC, and the first one is re-written far too large
    white = _range_file(save(content("white", 16, 16, 0), "gray", 30, False))
    return [("cut", bytes(cut)), ("flipped", bytes(flipped)), ("range", white)]


def _range_file(data: bytes) -> bytes:
    """A 16 x 16 grayscale file whose four blocks are lone DCs, re-written with a first DC difference of 2047 (category 11): times the
    table's quantiser it leaves the IDCT's input range.  Standard tables; the scan is rebuilt bit by bit."""
    from diffuman4d_amd.host.jpeg import AC_LUMA, DC_LUMA
    from jpeg_model import _Bits, huff_codes
    s, e = _scan_range(data)
    dc, ac = huff_codes(DC_LUMA), huff_codes(AC_LUMA)
    bw = _Bits()
    for diff in (2047, 0, 0, 0):
        n = abs(diff).bit_length()
        bw.put(*dc[n])
        if n:
            bw.put(diff, n)
        bw.put(*ac[0])
    bw.flush()
    return data[:s] + bytes(bw.out) + data[e:]


@functools.lru_cache(maxsize=None)
def unsupported() -> List[Tuple[str, bytes]]:
    a = content("smooth", 24, 40, 5)
    prog = save(a, "420", 90, False, progressive=True)
    f = io.BytesIO()
    Image.fromarray(a).convert("CMYK").save(f, "JPEG", quality=90)
    cmyk = f.getvalue()
    rst = save(a, "420", 90, False, restart_marker_rows=1)
    # Adobe transform 0 (the three components are RGB): the JFIF APP0 of a 4:4:4 file is replaced by an APP14 of the same role
    base = save(a, "444", 90, False)
    assert base[2:4] == b"\xff\xe0"
    n = int.from_bytes(base[4:6], "big")
    adobe0 = base[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00" + base[4 + n:]
    f = io.BytesIO()
    Image.fromarray(a).save(f, "PNG")
    return [("progressive", prog), ("cmyk", cmyk), ("restart", rst), ("adobe0", adobe0), ("png", f.getvalue())]
