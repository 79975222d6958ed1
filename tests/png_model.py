"""The definition of the device PNG encoder (csrc/png.hip, host/png.py) in numpy: the device equals ``encode`` byte for byte.

A file is: signature | IHDR (8 bit, colour type 0 = L or 6 = RGBA, no interlace) | one IDAT chunk per stripe | IEND.

Filter.  Every row is Paeth-filtered (type 4; row 0 against a zero row); a row of the filtered stream is the type byte then w * channels
bytes, R = 1 + w * channels bytes in all.

Stripes.  The stream is cut into stripes of ``stripe_rows(h, w, channels) = max(1, STRIPE_BYTES // R)`` whole rows (the last stripe
takes the rows that are left).

Tokens.  Within a stripe a maximal run of n equal bytes becomes: the literal; then, with m = n - 1, m // 258 matches (distance 1, length
258); then, with r = m % 258, one match of length r if r >= 3, else r literals.  Runs end at the stripe's end.

Code.  A stripe is one dynamic-Huffman block (BFINAL 0) with HLIT = 286 codes, HDIST = 2 codes (both of length 1; distance 1 is code
0) and all 19 code-length code lengths.  Histogram: the tokens' literal / length symbols and one end-of-block.  ``code_lengths`` is the
rule for both alphabets (limit 15, and 7 for the code-length alphabet): sort the used symbols by (count, symbol); build the Huffman
tree with two queues (sorted leaves, internal nodes in order of creation), always taking the lighter head and the leaf on a tie; a
symbol's length is its leaf's depth (a single used symbol gets length 1); if the deepest leaf is beyond the limit, replace every
non-zero count c by (c + 1) >> 1 and start again.  Codes are canonical (RFC 1951 3.2.2).  The 288 lengths (286 + the two 1s) are sent
as: a run of zeros of length z >= 11 -> symbol 18 with min(z, 138) (the rest of the run is looked at afresh); 3 <= z <= 10 -> symbol
17; anything else -> the length itself (symbol 16 is never used).

Joining.  After the end-of-block symbol comes an empty stored block (its three header bits -- BFINAL 1 in the last stripe --, zero bits
up to the byte boundary, 00 00 FF FF), so every stripe's deflate data is whole bytes and is its own IDAT chunk.  The first chunk starts
with the zlib header 78 01, the last ends with the Adler-32 of the filtered stream.

Bound.  A token costs at most 15 bits per byte it covers (a literal: 15; a match: 15 + 5 + 1 for at least 3 bytes), the block header at
most 17 + 57 + 288 * 14 bits, end-of-block 15, the stored block 42: a stripe of S bytes is at most 540 + 1.875 S bytes with its chunk
framing, zlib header and Adler-32.  ``bound`` = 64 + 576 * stripes + 2 * h * R covers signature, IHDR and IEND (45 bytes) as well.
"""
import struct
import zlib

import numpy as np

STRIPE_BYTES = 32768
MAX_SIDE = 16384
SIGNATURE = b"\x89PNG\r\n\x1a\n"
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def stripe_rows(h: int, w: int, channels: int) -> int:
    return max(1, STRIPE_BYTES // (1 + w * channels))


def n_stripes(h: int, w: int, channels: int) -> int:
    rows = stripe_rows(h, w, channels)
    return (h + rows - 1) // rows


def bound(h: int, w: int, channels: int) -> int:
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE and channels in (1, 4)):
        return 0
    return 64 + 576 * n_stripes(h, w, channels) + 2 * h * (1 + w * channels)


def paeth_filter(img: np.ndarray) -> np.ndarray:
    """uint8 [h, w] or [h, w, c] -> the filtered scanlines, uint8 [h, 1 + w * c]."""
    img = img[:, :, None] if img.ndim == 2 else img
    h, w, c = img.shape
    x = np.zeros((h + 1, w + 1, c), dtype=np.int32)
    x[1:, 1:] = img
    a, b, cc = x[1:, :-1], x[:-1, 1:], x[:-1, :-1]
    p = a + b - cc
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - cc)
    pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, cc))
    out = np.empty((h, 1 + w * c), dtype=np.uint8)
    out[:, 0] = 4
    out[:, 1:] = ((x[1:, 1:] - pred) & 255).astype(np.uint8).reshape(h, w * c)
    return out


def length_symbol(length: int):
    """match length 3..258 -> (symbol 257..285, extra bits, their value)"""
    k = max(i for i, b in enumerate(LEN_BASE) if b <= length)
    return 257 + k, LEN_EXTRA[k], length - LEN_BASE[k]


def tokens(stripe: np.ndarray):
    """The stripe's bytes -> [(byte, None) | (None, match length)] by the run rule."""
    s = np.asarray(stripe, dtype=np.uint8).reshape(-1)
    starts = np.concatenate([[0], np.flatnonzero(s[1:] != s[:-1]) + 1, [s.size]])
    out = []
    for a, e in zip(starts[:-1].tolist(), starts[1:].tolist()):
        v = int(s[a])
        out.append((v, None))
        full, r = divmod(e - a - 1, 258)
        out += [(None, 258)] * full
        out += [(None, r)] if r >= 3 else [(v, None)] * r
    return out


def code_lengths(freq, limit: int):
    f = [int(v) for v in freq]
    while True:
        used = sorted((c, s) for s, c in enumerate(f) if c > 0)
        n = len(used)
        lens = [0] * len(f)
        if n == 0:
            return lens
        if n == 1:
            lens[used[0][1]] = 1
            return lens
        w = [c for c, _ in used]
        nw, pl, pn = [], [0] * n, [0] * (n - 1)
        li = ni = 0
        for k in range(n - 1):
            wt = 0
            for _ in range(2):
                if li < n and (ni >= len(nw) or w[li] <= nw[ni]):
                    pl[li] = k
                    wt += w[li]
                    li += 1
                else:
                    pn[ni] = k
                    wt += nw[ni]
                    ni += 1
            nw.append(wt)
        dn = [0] * (n - 1)
        for k in range(n - 3, -1, -1):
            dn[k] = dn[pn[k]] + 1
        for i, (_, s) in enumerate(used):
            lens[s] = dn[pl[i]] + 1
        if max(lens) <= limit:
            return lens
        f = [(c + 1) >> 1 if c else 0 for c in f]


def canonical(lens):
    """code lengths -> the codes as they enter the bit stream (bit-reversed: deflate packs Huffman codes from their first bit)."""
    count = [0] * 17
    for v in lens:
        count[v] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = [0] * len(lens)
    for s, v in enumerate(lens):
        if v:
            out[s] = int(format(nxt[v], f"0{v}b")[::-1], 2)
            nxt[v] += 1
    return out


def length_sequence(seq):
    """the 288 code lengths -> [(code-length symbol, extra bits, value)]"""
    out, i = [], 0
    while i < len(seq):
        v = seq[i]
        if v == 0:
            z = 1
            while i + z < len(seq) and seq[i + z] == 0:
                z += 1
            if z >= 11:
                z = min(z, 138)
                out.append((18, 7, z - 11))
            elif z >= 3:
                out.append((17, 3, z - 3))
            else:
                z = 1
                out.append((0, 0, 0))
            i += z
        else:
            out.append((v, 0, 0))
            i += 1
    return out


def pack_bits(values, nbits) -> bytes:
    """values[k] in nbits[k] bits each, least significant bit first, back to back; zero bits to the byte boundary."""
    values, nbits = np.asarray(values, dtype=np.int64), np.asarray(nbits, dtype=np.int64)
    pos = np.cumsum(nbits) - nbits
    which = np.repeat(np.arange(values.size), nbits)
    bit = np.arange(int(nbits.sum())) - np.repeat(pos, nbits)
    return np.packbits(((values[which] >> bit) & 1).astype(np.uint8), bitorder="little").tobytes()


def deflate_stripe(stripe: np.ndarray, last: bool) -> bytes:
    toks = tokens(stripe)
    hist = [0] * 286
    for lit, length in toks:
        hist[lit if length is None else length_symbol(length)[0]] += 1
    hist[256] = 1
    lens = code_lengths(hist, 15)
    codes = canonical(lens)
    seq = length_sequence(lens + [1, 1])
    clfreq = [0] * 19
    for s, _, _ in seq:
        clfreq[s] += 1
    cllens = code_lengths(clfreq, 7)
    clcodes = canonical(cllens)
    vals, bits = [0, 2, 29, 1, 15], [1, 2, 5, 5, 4]
    for s in CL_ORDER:
        vals.append(cllens[s]), bits.append(3)
    for s, eb, ev in seq:
        vals.append(clcodes[s] | (ev << cllens[s])), bits.append(cllens[s] + eb)
    for lit, length in toks:
        if length is None:
            vals.append(codes[lit]), bits.append(lens[lit])
        else:
            s, eb, ev = length_symbol(length)
            vals.append(codes[s] | (ev << lens[s])), bits.append(lens[s] + eb + 1)  # + the distance code: one 0 bit
    vals.append(codes[256]), bits.append(lens[256])
    vals += [1 if last else 0, 0]
    bits += [1, 2]
    return pack_bits(vals, bits) + b"\x00\x00\xff\xff"


def chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def encode(img: np.ndarray) -> bytes:
    """uint8 [h, w] (L) or [h, w, 4] (RGBA) -> the PNG file."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    if not (img.ndim == 2 or (img.ndim == 3 and img.shape[2] == 4)):
        raise ValueError(f"expected [h, w] or [h, w, 4], got {img.shape}")
    h, w = img.shape[:2]
    ch = 1 if img.ndim == 2 else 4
    if bound(h, w, ch) == 0:
        raise ValueError(f"size {w} x {h} is outside 1..{MAX_SIDE}")
    filt = paeth_filter(img)
    rows, n = stripe_rows(h, w, ch), n_stripes(h, w, ch)
    out = [SIGNATURE, chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0 if ch == 1 else 6, 0, 0, 0))]
    for s in range(n):
        data = deflate_stripe(filt[s * rows: (s + 1) * rows], s == n - 1)
        if s == 0:
            data = b"\x78\x01" + data
        if s == n - 1:
            data += struct.pack(">I", zlib.adler32(filt.tobytes()))
        out.append(chunk(b"IDAT", data))
    out.append(chunk(b"IEND", b""))
    return b"".join(out)
