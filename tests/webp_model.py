"""The definition of the device lossless-WebP encoder (csrc/webp.hip, host/webp.py) in numpy: the device equals ``encode`` byte for byte.

A file is: ``RIFF`` | le32(4 + 8 + padded payload) | ``WEBP`` | ``VP8L`` | le32(payload bytes) | payload | one zero byte if the payload
is odd.  The payload is a VP8L bit stream (bits least significant first): 0x2f, 14 bits w - 1, 14 bits h - 1, alpha_is_used 0, version
0 (3 bits); no transform (0), no colour cache (0), no meta prefix image (0); the five prefix codes; the tokens.

Tokens.  The pixels are numbered p = y * w + x.  A pixel's kind is a function of the pixels alone: U if p >= w and it equals pixel
p - w, else L if p >= 1 and it equals pixel p - 1, else literal (pixel 0 is a literal).  The pixels are cut into stripes of
``STRIPE_PIXELS`` consecutive pixels (the last stripe takes what is left).  Within a stripe a maximal run of n pixels of kind U (or L)
becomes n // 4096 backward references of length 4096 and one of n % 4096 if that is not 0, all with distance plane code 1 = the pixel
above (or 2 = the pixel to the left); a run ends at the stripe's end, though what it refers to may lie in an earlier stripe.  A literal
pixel is one token: its green, red, blue and alpha (always 255) symbols.

Codes.  One group of five codes per image -- green + length prefixes (280 symbols), red, blue, alpha (256 each), distance (40) -- from
the histograms of all the image's tokens.  ``code_lengths`` is tests/png_model.py's rule (limit 15; 7 for the code-length code) and the
codes are canonical, written bit-reversed.  A code whose used symbols are at most two and all below 256 is sent as a simple code (an
alphabet with no used symbol: the one symbol 0; two symbols in ascending order; is_8bit = 1 unless the first symbol is below 2).
Any other code is a normal code: all 19 code-length code lengths in the format's order, no max_symbol, then every symbol's length through
that code, without the repeat codes 16, 17 and 18.  A code with one used symbol costs 0 bits per use, the code-length code included.

A backward reference is: the symbol 256 + prefix(length) of the green code, the length's extra bits, the symbol prefix(plane code) of
the distance code (plane codes 1 and 2 have no extra bits).

Bound.  A literal costs at most 3 * 15 bits, a backward reference at most 15 + 10 + 15 for at least one pixel; the five code tables at
most 43 + 3 * (62 + 280 * 7) + 11 bits < 780 bytes: ``bound`` = 800 + 6 * h * w covers the 20 bytes of framing and the pad byte as well.
"""
import struct

import numpy as np

import png_model

STRIPE_PIXELS = 8192
MAX_SIDE = 16383
MAX_LENGTH = 4096
LITERAL, UP, LEFT = 0, 1, 2
CL_ORDER = (17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
ALPHABETS = (280, 256, 256, 256, 40)  # green + length, red, blue, alpha, distance

code_lengths = png_model.code_lengths


def stripe_pixels(h: int, w: int) -> int:
    """Pixels of one stripe of an h x w image (the last one may be shorter)."""
    return STRIPE_PIXELS


def n_stripes(h: int, w: int) -> int:
    return (h * w + stripe_pixels(h, w) - 1) // stripe_pixels(h, w)


def bound(h: int, w: int) -> int:
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        return 0
    return 800 + 6 * h * w


def prefix(v: int):
    """value >= 1 (a length, or a distance plane code) -> (prefix symbol, extra bits, their value)"""
    if v <= 4:
        return v - 1, 0, 0
    v -= 1
    hb = v.bit_length() - 1
    extra = hb - 1
    return 2 * hb + ((v >> (hb - 1)) & 1), extra, v & ((1 << extra) - 1)


def kinds(rgb: np.ndarray) -> np.ndarray:
    """uint8 [h, w, 3] -> the kind of every pixel, uint8 [h * w]."""
    h, w, _ = rgb.shape
    px = rgb.reshape(h * w, 3)
    n = h * w
    k = np.zeros(n, dtype=np.uint8)
    k[1:][(px[1:] == px[:-1]).all(axis=1)] = LEFT
    if n > w:
        k[w:][(px[w:] == px[:-w]).all(axis=1)] = UP
    return k


def tokens(rgb: np.ndarray):
    """uint8 [h, w, 3] -> (pos, kind, length): int64 arrays, one entry per token in stream order.  A literal has length 1."""
    h, w, _ = rgb.shape
    k = kinds(rgb)
    n = k.size
    p = np.arange(n)
    start = np.ones(n, dtype=bool)
    start[1:] = (k[1:] != k[:-1]) | (k[1:] == LITERAL) | (p[1:] % stripe_pixels(h, w) == 0)
    first = np.flatnonzero(start)                       # run starts
    end = np.append(first[1:], n)
    run = np.cumsum(start) - 1
    j = p - first[run]
    tok = j % MAX_LENGTH == 0
    pos = p[tok]
    return pos, k[pos].astype(np.int64), np.minimum(MAX_LENGTH, end[run[pos]] - pos)


def histograms(rgb: np.ndarray, pos, kind, length):
    """The five histograms of the tokens (lists of ints, ALPHABETS long)."""
    px = rgb.reshape(-1, 3)
    lit = pos[kind == LITERAL]
    g = np.bincount(px[lit, 1], minlength=280)
    for v in length[kind != LITERAL].tolist():
        g[256 + prefix(v)[0]] += 1
    r = np.bincount(px[lit, 0], minlength=256)
    b = np.bincount(px[lit, 2], minlength=256)
    a = np.zeros(256, dtype=np.int64)
    a[255] = lit.size
    d = np.zeros(40, dtype=np.int64)
    d[0], d[1] = int((kind == UP).sum()), int((kind == LEFT).sum())
    return [x.tolist() for x in (g, r, b, a, d)]


def code_table(hist):
    """histogram -> (values, bit counts of the code's description; lens: bits per use of each symbol; codes as they enter the stream)"""
    used = [s for s, c in enumerate(hist) if c]
    lens = code_lengths(hist, 15)
    codes = png_model.canonical(lens)
    if len(used) <= 2 and all(s < 256 for s in used):
        syms = used or [0]
        wide = 0 if syms[0] < 2 else 1
        vals, bits = [1, len(syms) - 1, wide, syms[0]], [1, 1, 1, 8 if wide else 1]
        if len(syms) == 2:
            vals.append(syms[1]), bits.append(8)
    else:
        clfreq = [0] * 19
        for v in lens:
            clfreq[v] += 1
        cllens = code_lengths(clfreq, 7)
        clcodes = png_model.canonical(cllens)
        one = sum(1 for c in clfreq if c) == 1
        vals, bits = [0, 15], [1, 4]
        for s in CL_ORDER:
            vals.append(cllens[s]), bits.append(3)
        vals.append(0), bits.append(1)
        for v in lens:
            vals.append(0 if one else clcodes[v]), bits.append(0 if one else cllens[v])
    if len(used) <= 1:
        lens = [0] * len(hist)
        codes = [0] * len(hist)
    return vals, bits, lens, codes


def payload(rgb: np.ndarray) -> bytes:
    h, w, _ = rgb.shape
    pos, kind, length = tokens(rgb)
    vals, bits = [0x2f, w - 1, h - 1, 0, 0, 0, 0, 0], [8, 14, 14, 1, 3, 1, 1, 1]
    lens, codes = [], []
    for hist in histograms(rgb, pos, kind, length):
        v, b, l, c = code_table(hist)
        vals += v
        bits += b
        lens.append(np.array(l, dtype=np.int64)), codes.append(np.array(c, dtype=np.int64))
    # every token as one value: a literal is green | red | blue (alpha costs 0 bits); a reference is length symbol | extra | distance symbol
    px = rgb.reshape(-1, 3).astype(np.int64)[pos]
    g, r, b = px[:, 1], px[:, 0], px[:, 2]
    lv = codes[0][g] | (codes[1][r] << lens[0][g]) | (codes[2][b] << (lens[0][g] + lens[1][r]))
    lb = lens[0][g] + lens[1][r] + lens[2][b] + lens[3][255]
    pre = np.array([prefix(v) for v in range(1, MAX_LENGTH + 1)], dtype=np.int64)[length - 1]
    sym, ds = 256 + pre[:, 0], np.where(kind == UP, 0, 1)
    mv = codes[0][sym] | (pre[:, 2] << lens[0][sym]) | (codes[4][ds] << (lens[0][sym] + pre[:, 1]))
    mb = lens[0][sym] + pre[:, 1] + lens[4][ds]
    is_lit = kind == LITERAL
    tv, tb = np.where(is_lit, lv, mv), np.where(is_lit, lb, mb)
    return png_model.pack_bits(np.concatenate([np.array(vals, dtype=np.int64), tv]), np.concatenate([np.array(bits, dtype=np.int64), tb]))


def encode(rgb: np.ndarray) -> bytes:
    """uint8 [h, w, 3] -> the lossless WebP file."""
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    if rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError(f"expected [h, w, 3], got {rgb.shape}")
    h, w = rgb.shape[:2]
    if bound(h, w) == 0:
        raise ValueError(f"size {w} x {h} is outside 1..{MAX_SIDE}")
    data = payload(rgb)
    pad = b"\x00" * (len(data) & 1)
    return b"RIFF" + struct.pack("<I", 12 + len(data) + len(pad)) + b"WEBPVP8L" + struct.pack("<I", len(data)) + data + pad
