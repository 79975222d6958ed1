"""A plain numpy restatement of the baseline JPEG file Pillow / libjpeg-turbo writes for ``Image.fromarray(a).save(f, "JPEG",
quality=q)`` (RGB, 4:2:0, standard Huffman tables, no restart markers), and of ``imgwrite.restore_cropped_image``.

Integer arithmetic throughout; this is the definition the device encoder (csrc/jpeg.hip) is held to, byte for byte, and it is itself
held to Pillow on the CPU (tests/test_jpeg_cpu.py).  ``encode`` also counts what a set of test images exercises: ZRL symbols, stuffed
bytes, the largest DC / AC category and dummy blocks.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from diffuman4d_amd.host.jpeg import AC_CHROMA, AC_LUMA, DC_CHROMA, DC_LUMA, ZIGZAG, jpeg_header, quant_tables

CONST_BITS, PASS1_BITS = 13, 2
F_0_298, F_0_390, F_0_541, F_0_765, F_0_899, F_1_175 = 2446, 3196, 4433, 6270, 7373, 9633
F_1_501, F_1_847, F_1_961, F_2_053, F_2_562, F_3_072 = 12299, 15137, 16069, 16819, 20995, 25172


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _dct_1d(d, first: bool):
    """jfdctint.c, one pass over the last axis of d [..., 8] (int64)."""
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    out = np.empty_like(d)
    n = CONST_BITS - PASS1_BITS if first else CONST_BITS + PASS1_BITS
    if first:
        out[..., 0] = (t10 + t11) << PASS1_BITS
        out[..., 4] = (t10 - t11) << PASS1_BITS
    else:
        out[..., 0] = _descale(t10 + t11, PASS1_BITS)
        out[..., 4] = _descale(t10 - t11, PASS1_BITS)
    z1 = (t12 + t13) * F_0_541
    out[..., 2] = _descale(z1 + t13 * F_0_765, n)
    out[..., 6] = _descale(z1 - t12 * F_1_847, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F_1_175
    t4, t5, t6, t7 = t4 * F_0_298, t5 * F_2_053, t6 * F_3_072, t7 * F_1_501
    z1, z2, z3, z4 = -z1 * F_0_899, -z2 * F_2_562, -z3 * F_1_961 + z5, -z4 * F_0_390 + z5
    out[..., 7] = _descale(t4 + z1 + z3, n)
    out[..., 5] = _descale(t5 + z2 + z4, n)
    out[..., 3] = _descale(t6 + z2 + z3, n)
    out[..., 1] = _descale(t7 + z1 + z4, n)
    return out


def fdct_islow(blocks: np.ndarray) -> np.ndarray:
    """blocks [..., 8, 8] level-shifted samples -> coefficients scaled by 8 (rows first, then columns)."""
    x = _dct_1d(blocks.astype(np.int64), True)
    return np.swapaxes(_dct_1d(np.swapaxes(x, -1, -2), False), -1, -2)


def quantise(coef: np.ndarray, q: np.ndarray) -> np.ndarray:
    """coef [..., 8, 8], q [8, 8] (natural order): sign(c) * ((|c| + (8 q >> 1)) // (8 q))."""
    d = q.astype(np.int64) * 8
    return np.sign(coef) * ((np.abs(coef) + (d >> 1)) // d)


def planes(a: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """RGB uint8 [h, w, 3] -> (Y [16 my, 16 mx], Cb, Cr [8 my, 8 mx]) int64, padded as libjpeg pads them."""
    h, w = a.shape[:2]
    my, mx = (h + 15) // 16, (w + 15) // 16
    r, g, b = (a[..., c].astype(np.int64) for c in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    rows = np.minimum(np.arange(16 * my), h - 1)
    cols = np.minimum(np.arange(16 * mx), w - 1)
    yp = y[rows][:, cols]
    # chroma: true rows padded by replication to an even count, columns replicated to the MCU width, then the DOWNSAMPLED last row
    # is replicated
    crow = np.minimum(np.arange(8 * my), (h + 1) // 2 - 1)
    r0, r1 = np.minimum(2 * crow, h - 1), np.minimum(2 * crow + 1, h - 1)
    ccol = np.arange(8 * mx)
    c0, c1 = np.minimum(2 * ccol, w - 1), np.minimum(2 * ccol + 1, w - 1)
    bias = 1 + (ccol & 1)

    def down(p):
        return (p[r0][:, c0] + p[r0][:, c1] + p[r1][:, c0] + p[r1][:, c1] + bias[None, :]) >> 2
    return yp, down(cb), down(cr)


def coefficients(a: np.ndarray, quality: int, counters: Optional[Dict[str, int]] = None) -> np.ndarray:
    """-> int64 [my, mx, 6, 64]: the quantised coefficients of every MCU's blocks (Y00 Y01 Y10 Y11 Cb Cr) in zig-zag order."""
    h, w = a.shape[:2]
    my, mx = (h + 15) // 16, (w + 15) // 16
    ql, qc = quant_tables(quality)
    yp, cb, cr = planes(a)

    def blocks(p, n):  # [8 n my, 8 n mx] -> [my, mx, n, n, 8, 8]
        return p.reshape(my, n, 8, mx, n, 8).transpose(0, 3, 1, 4, 2, 5)
    yq = quantise(fdct_islow(blocks(yp - 128, 2)), np.asarray(ql).reshape(8, 8)).reshape(my, mx, 4, 64)
    cbq = quantise(fdct_islow(blocks(cb - 128, 1)), np.asarray(qc).reshape(8, 8)).reshape(my, mx, 1, 64)
    crq = quantise(fdct_islow(blocks(cr - 128, 1)), np.asarray(qc).reshape(8, 8)).reshape(my, mx, 1, 64)
    out = np.concatenate([yq, cbq, crq], axis=2)
    bw, bh = (w + 7) // 8, (h + 7) // 8
    dummies = 0
    for j in range(my):
        for i in range(mx):
            for b in range(1, 4):  # a luma block outside the component: zero AC, DC of the preceding block of the MCU
                if 2 * i + (b & 1) >= bw or 2 * j + (b >> 1) >= bh:
                    out[j, i, b, :] = 0
                    out[j, i, b, 0] = out[j, i, b - 1, 0]
                    dummies += 1
    if counters is not None:
        counters["dummy_blocks"] = counters.get("dummy_blocks", 0) + dummies
        if bw & 1:
            counters["dummy_cols"] = counters.get("dummy_cols", 0) + 1
        if bh & 1:
            counters["dummy_rows"] = counters.get("dummy_rows", 0) + 1
    return out[..., ZIGZAG]


def huff_codes(spec) -> Dict[int, Tuple[int, int]]:
    """Annex C: (bits[16], values) -> {symbol: (code, length)}."""
    bits, vals = spec
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()
        self.stuffed = 0

    def put(self, code: int, length: int) -> None:
        self.acc = (self.acc << length) | (code & ((1 << length) - 1))
        self.n += length
        while self.n >= 8:
            byte = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)
                self.stuffed += 1
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self) -> None:
        if self.n:
            self.put(0x7F, 8 - self.n)  # the final partial byte is filled with 1-bits


def scan_bytes(coefs: np.ndarray, counters: Optional[Dict[str, int]] = None) -> bytes:
    """The entropy-coded segment of coefficients [my, mx, 6, 64] (zig-zag): interleaved MCUs, stuffed, padded with 1-bits."""
    tabs = [(huff_codes(DC_LUMA), huff_codes(AC_LUMA))] * 4 + [(huff_codes(DC_CHROMA), huff_codes(AC_CHROMA))] * 2
    comp = [0, 0, 0, 0, 1, 2]
    pred = [0, 0, 0]
    bw = _Bits()
    zrl = dc_cat = ac_cat = 0
    for mcu in coefs.reshape(-1, 6, 64).tolist():
        for b, blk in enumerate(mcu):
            dc_tab, ac_tab = tabs[b]
            diff = blk[0] - pred[comp[b]]
            pred[comp[b]] = blk[0]
            n = abs(diff).bit_length()
            dc_cat = max(dc_cat, n)
            bw.put(*dc_tab[n])
            if n:
                bw.put(diff if diff >= 0 else diff - 1, n)
            run = 0
            for k in range(1, 64):
                v = blk[k]
                if v == 0:
                    run += 1
                    continue
                while run > 15:
                    bw.put(*ac_tab[0xF0])
                    zrl += 1
                    run -= 16
                n = abs(v).bit_length()
                ac_cat = max(ac_cat, n)
                bw.put(*ac_tab[(run << 4) | n])
                bw.put(v if v >= 0 else v - 1, n)
                run = 0
            if run:
                bw.put(*ac_tab[0x00])
    bw.flush()
    if counters is not None:
        counters["zrl"] = counters.get("zrl", 0) + zrl
        counters["stuffed"] = counters.get("stuffed", 0) + bw.stuffed
        counters["max_dc_category"] = max(counters.get("max_dc_category", 0), dc_cat)
        counters["max_ac_category"] = max(counters.get("max_ac_category", 0), ac_cat)
    return bytes(bw.out)


def encode(a: np.ndarray, quality: int = 90, counters: Optional[Dict[str, int]] = None) -> bytes:
    """RGB uint8 [h, w, 3] -> the whole file."""
    a = np.asarray(a)
    assert a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 3
    h, w = a.shape[:2]
    return jpeg_header(h, w, quality) + scan_bytes(coefficients(a, quality, counters), counters) + b"\xff\xd9"


# -- restore_cropped_image ----------------------------------------------------------------------------------------------------------
def _resample_axis(x: np.ndarray, out_size: int) -> np.ndarray:
    """Pillow's bicubic pass over axis 1 of x uint8 [rows, in, 3] -> uint8 [rows, out, 3]."""
    from diffuman4d_amd.host.capture import PRECISION_BITS, bicubic_table
    bounds, k = bicubic_table(x.shape[1], out_size)
    out = np.empty((x.shape[0], out_size, 3), dtype=np.uint8)
    xi = x.astype(np.int64)
    for o in range(out_size):
        lo, n = int(bounds[o, 0]), int(bounds[o, 1])
        acc = (1 << (PRECISION_BITS - 1)) + (xi[:, lo:lo + n, :] * k[o, :n].astype(np.int64)[None, :, None]).sum(axis=1)
        out[:, o, :] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def restore(a: np.ndarray, crop: Optional[Sequence[int]]) -> np.ndarray:
    """``np.asarray(restore_cropped_image(Image.fromarray(a), crop))``: horizontal pass, rounding to uint8, vertical pass, paste at
    (cl, ct) of a white canvas with clipping."""
    if crop is None:
        return a
    crop = tuple(int(v) for v in crop)
    if len(crop) == 4:
        (ct, cl, ch, cw), (h, w) = crop, a.shape[:2]
    elif len(crop) == 6:
        ct, cl, ch, cw, h, w = crop
    else:
        raise ValueError(f"Invalid crop_param: {crop}")
    patch = _resample_axis(a, cw)
    patch = _resample_axis(patch.transpose(1, 0, 2), ch).transpose(1, 0, 2)
    canvas = np.full((h, w, 3), 255, dtype=np.uint8)
    y0, y1, x0, x1 = max(ct, 0), min(ct + ch, h), max(cl, 0), min(cl + cw, w)
    if y1 > y0 and x1 > x0:
        canvas[y0:y1, x0:x1] = patch[y0 - ct:y1 - ct, x0 - cl:x1 - cl]
    return canvas
