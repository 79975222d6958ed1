"""The definition of the device PNG decoder (diffuman4d_amd/csrc/pngdec.hip) in numpy and plain Python: the container, zlib / DEFLATE
(RFC 1950 / 1951, table validity as zlib's inflate_table) and the five row filters.

``decode_status(data)`` is the straightforward decode: bytes appended to a list, rows unfiltered one after another.
``decode_status(data, scheme="device")`` is an emulation of exactly the device's scheme: the 64 KiB window ring whose halves are
flushed to the workspace and summed into the Adler-32 chunk by chunk, literals gathered 64 at a time, a match copied by 64 lanes in
steps (byte i = window[start - dist + i mod dist]), and the unfilter as a skewed wavefront over bands of 64 rows with the band's
last row kept aside.  Both walk the bits in the same order with the same checks, so they give the same status words; the tests hold
the emulation to the straightforward decode and that to Pillow.
"""
from __future__ import annotations

import struct
import zlib
from typing import Optional, Tuple

import numpy as np

RING = 65536            # DM4D_PNGDEC_RING_BYTES
HALF = RING // 2
MAX_ROW_BYTES = 32768   # DM4D_PNGDEC_MAX_ROW_BYTES
MAX_STREAM_BYTES = 1 << 28
ST_HEADER, ST_BLOCK, ST_CODE, ST_DISTANCE, ST_END, ST_ADLER, ST_FILTER = 1, 2, 4, 8, 16, 32, 64
SIGNATURE = b"\x89PNG\r\n\x1a\n"
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CHANNELS = {0: 1, 2: 3, 6: 4}


# -- container -----------------------------------------------------------------------------------------------------------------------
def probe(data: bytes) -> Optional[dict]:
    """{"h", "w", "channels", "idat": [(start, end)]} of a file of the supported set, or None."""
    data = bytes(data)
    if data[:8] != SIGNATURE:
        return None
    pos, ihdr, idat, after_idat = 8, None, [], False
    while True:
        if pos + 12 > len(data):
            return None
        length, kind = struct.unpack_from(">I4s", data, pos)
        end = pos + 8 + length
        if end + 4 > len(data) or zlib.crc32(data[pos + 4:end]) != struct.unpack_from(">I", data, end)[0]:
            return None
        if ihdr is None:
            if kind != b"IHDR" or length != 13:
                return None
            ihdr = struct.unpack(">IIBBBBB", data[pos + 8:end])
        elif kind == b"IDAT":
            if after_idat:
                return None
            idat.append((pos + 8, end))
        elif kind == b"IEND":
            break
        elif kind in (b"IHDR", b"tRNS", b"acTL", b"CgBI") or not kind.isalpha() or kind[:1].isupper():
            return None
        elif idat:
            after_idat = True
        pos = end + 4
    w, h, depth, colour, comp, filt, lace = ihdr
    if depth != 8 or colour not in CHANNELS or comp or filt or lace or w < 1 or h < 1 or not idat:
        return None
    ch = CHANNELS[colour]
    total = sum(e - s for s, e in idat)
    if w * ch > MAX_ROW_BYTES or not 2 <= total < MAX_STREAM_BYTES or h * (1 + w * ch) >= 1 << 31:
        return None
    return {"h": h, "w": w, "channels": ch, "idat": idat}


# -- bits ----------------------------------------------------------------------------------------------------------------------------
class Bits:
    """The stream, least significant bit first; bits beyond its length read as zeros."""

    def __init__(self, stream: bytes):
        self.n = len(stream)
        self.buf = bytes(stream) + bytes(16)
        self.pos = 0

    def peek(self, n: int) -> int:
        p = min(self.pos >> 3, self.n + 7)
        return (int.from_bytes(self.buf[p:p + 8], "little") >> (self.pos & 7)) & ((1 << n) - 1)

    def take(self, n: int) -> int:
        v = self.peek(n)
        self.pos += n
        return v

    def align(self):
        self.pos = (self.pos + 7) & ~7

    def over(self) -> bool:
        return self.pos > 8 * self.n

    def byte(self, i: int) -> int:
        return self.buf[i] if i < self.n else 0


class Code:
    """A canonical prefix code from code lengths, with zlib's verdict: ``state`` 0 complete, 1 over-subscribed, 2 incomplete."""

    def __init__(self, lens):
        count = [0] * 16
        for l in lens:
            count[l] += 1
        count[0] = 0
        left, self.max_len = 1, 0
        for l in range(1, 16):
            left = 2 * left - count[l]
            if left < 0:
                self.state = 1
                return
            if count[l]:
                self.max_len = l
        self.state = 2 if left > 0 else 0
        self.by_len = [dict() for _ in range(16)]  # [l][code, first bit on top] -> symbol
        code, nxt = 0, [0] * 16
        for l in range(1, 16):
            code = (code + count[l - 1]) << 1
            nxt[l] = code
        for sym, l in enumerate(lens):
            if l:
                self.by_len[l][nxt[l]] = sym
                nxt[l] += 1

    def decode(self, bits: Bits) -> Tuple[int, int]:
        """(symbol, length) of the code the next bits start; length 0 = none does"""
        window = bits.peek(15)
        code = 0
        for l in range(1, self.max_len + 1):
            code = (code << 1) | ((window >> (l - 1)) & 1)
            sym = self.by_len[l].get(code)
            if sym is not None:
                return sym, l
        return 0, 0


FIXED_LENS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8 + [5] * 32


# -- where the bytes go ------------------------------------------------------------------------------------------------------------------
class PlainSink:
    """The straightforward output: one growing array, the checksum from zlib."""

    def __init__(self, expect: int):
        self.out = bytearray()
        self.expect = expect

    @property
    def total(self) -> int:
        return len(self.out)

    def literal(self, b: int):
        self.out.append(b)

    def stored(self, data: bytes):
        self.out += data

    def match(self, dist: int, length: int):
        start = len(self.out) - dist
        for i in range(length):
            self.out.append(self.out[start + i])

    def finish(self) -> int:
        return zlib.adler32(bytes(self.out))

    def result(self) -> bytes:
        return bytes(self.out)


class DeviceSink:
    """The device's output scheme: a ring of RING bytes for the window, halves flushed to the workspace with their Adler-32 share,
    pending literals held one per lane, every copy done by 64 lanes a step."""
    LANES = 64

    def __init__(self, expect: int):
        self.ring = np.zeros(RING, dtype=np.uint8)
        self.ws = np.full(expect, 0xEE, dtype=np.uint8)  # what was never flushed stays visible
        self.expect = expect
        self.pos = 0
        self.s1, self.s2 = 1, 0
        self.pending = []
        self.flushes = 0

    @property
    def total(self) -> int:
        return self.pos + len(self.pending)

    def _flush(self, k: int, n: int):
        src = self.ring[(k & 1) * HALF:(k & 1) * HALF + n]
        assert k * HALF + n <= self.expect  # every store is below the image's expected size
        self.ws[k * HALF:k * HALF + n] = src
        v = src.astype(np.uint64)
        weighted = int((v * (n - np.arange(n, dtype=np.uint64))).sum())
        self.s2 = (self.s2 + n * self.s1 + weighted) % 65521
        self.s1 = (self.s1 + int(v.sum())) % 65521
        self.flushes += 1

    def _produced(self, n: int):
        assert n <= HALF
        to = self.pos + n
        if to // HALF != self.pos // HALF:
            self._flush(self.pos // HALF, HALF)
        self.pos = to

    def _flush_literals(self):
        if self.pending:
            idx = (self.pos + np.arange(len(self.pending))) % RING
            self.ring[idx] = self.pending
            self._produced(len(self.pending))
            self.pending = []

    def literal(self, b: int):
        self.pending.append(b)
        if len(self.pending) == self.LANES:
            self._flush_literals()

    def stored(self, data: bytes):
        self._flush_literals()
        for off in range(0, len(data), self.LANES):
            part = np.frombuffer(data[off:off + self.LANES], dtype=np.uint8)
            self.ring[(self.pos + np.arange(len(part))) % RING] = part
            self._produced(len(part))

    def match(self, dist: int, length: int):
        self._flush_literals()
        for c in range(0, length, self.LANES):  # 64 lanes a step; every source lies before pos, so no step reads what another stores
            i = np.arange(c, min(c + self.LANES, length))
            src = (self.pos - dist + (i if dist >= length else i % dist)) % RING
            assert ((src - self.pos) % RING >= RING - HALF).all()
            self.ring[(self.pos + i) % RING] = self.ring[src]
        self._produced(length)

    def finish(self) -> int:
        self._flush_literals()
        k = self.pos // HALF
        if self.pos > k * HALF:
            self._flush(k, self.pos - k * HALF)
        return (self.s2 << 16) | self.s1

    def result(self) -> bytes:
        return self.ws.tobytes()


def inflate(stream: bytes, expect: int, sink) -> int:
    """The zlib stream into `sink` -> the status word.  The order of the checks is the device's."""
    bits = Bits(stream)
    cmf, flg = bits.take(8), bits.take(8)
    if (cmf & 15) != 8 or (cmf >> 4) > 7 or ((cmf << 8) | flg) % 31 or (flg & 32):
        return ST_HEADER
    last = False
    while not last:
        if bits.over():
            return ST_END
        last = bool(bits.take(1))
        kind = bits.take(2)
        if kind == 3:
            return ST_BLOCK
        if kind == 0:
            bits.align()
            n, nn = bits.take(16), bits.take(16)
            if n != (~nn & 0xFFFF):
                return ST_BLOCK
            at = bits.pos >> 3
            if n > expect - sink.total:
                return ST_END
            sink.stored(bytes(bits.byte(at + i) for i in range(n)))
            bits.pos += 8 * n
            if bits.over():
                return ST_END
            continue
        if kind == 1:
            lens, nl = FIXED_LENS, 288
        else:
            nl, nd, ncl = 257 + bits.take(5), 1 + bits.take(5), 4 + bits.take(4)
            if nl > 286 or nd > 30:
                return ST_BLOCK
            cl = [0] * 19
            for i in range(ncl):
                cl[CL_ORDER[i]] = bits.take(3)
            clc = Code(cl)
            if clc.state != 0:
                return ST_BLOCK
            lens, prev = [], 0
            while len(lens) < nl + nd:
                sym, l = clc.decode(bits)
                if l == 0:
                    return ST_BLOCK
                bits.pos += l
                if sym < 16:
                    rep, val = 1, sym
                elif sym == 16:
                    if not lens:
                        return ST_BLOCK
                    rep, val = 3 + bits.take(2), prev
                elif sym == 17:
                    rep, val = 3 + bits.take(3), 0
                else:
                    rep, val = 11 + bits.take(7), 0
                if len(lens) + rep > nl + nd:
                    return ST_BLOCK
                lens += [val] * rep
                prev = val
            if bits.over():
                return ST_END
            if lens[256] == 0:
                return ST_BLOCK
        lit, dst = Code(lens[:nl]), Code(lens[nl:])
        if lit.state == 1 or (lit.state == 2 and lit.max_len != 1):
            return ST_BLOCK
        if dst.state == 1 or (dst.state == 2 and dst.max_len > 1):
            return ST_BLOCK
        while True:
            if bits.over():
                return ST_END
            sym, l = lit.decode(bits)
            if l == 0 or sym >= 286:
                return ST_CODE
            bits.pos += l
            if sym < 256:
                if sink.total >= expect:
                    return ST_END
                sink.literal(sym)
                continue
            if sym == 256:
                break
            length = LEN_BASE[sym - 257] + bits.take(LEN_EXTRA[sym - 257])
            dsym, l = dst.decode(bits)
            if l == 0 or dsym >= 30:
                return ST_CODE
            bits.pos += l
            dist = DIST_BASE[dsym] + bits.take(DIST_EXTRA[dsym])
            if dist > sink.total:
                return ST_DISTANCE
            if length > expect - sink.total:
                return ST_END
            sink.match(dist, length)
    adler = sink.finish()
    if sink.total != expect:
        return ST_END
    bits.align()
    want = int.from_bytes(bytes(bits.byte((bits.pos >> 3) + i) for i in range(4)), "big")
    bits.pos += 32
    if bits.over():
        return ST_END
    return 0 if want == adler else ST_ADLER


# -- filters ---------------------------------------------------------------------------------------------------------------------------
def paeth(a, b, c):
    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
    return a if pa <= pb and pa <= pc else b if pb <= pc else c


def unfilter_plain(filtered: bytes, h: int, w: int, bpp: int) -> Tuple[np.ndarray, int]:
    rb = w * bpp
    out = np.zeros((h, rb), dtype=np.uint8)
    prev = [0] * rb
    status = 0
    for y in range(h):
        line = filtered[y * (rb + 1):(y + 1) * (rb + 1)]
        ft, cur = line[0], [0] * rb
        if ft > 4:
            status = ST_FILTER
        for i in range(rb):
            a = cur[i - bpp] if i >= bpp else 0
            b = prev[i]
            c = prev[i - bpp] if i >= bpp else 0
            pred = (0, a, b, (a + b) >> 1, paeth(a, b, c))[ft] if ft <= 4 else 0
            cur[i] = (line[1 + i] + pred) & 255
        out[y] = cur
        prev = cur
    return out, status


def unfilter_device(filtered: bytes, h: int, w: int, bpp: int) -> Tuple[np.ndarray, int]:
    """The wavefront: lane j has row 64 b + j and works on pixel t - j at step t; the pixel above is what lane j - 1 decoded a step
    earlier, the pixel above-left what this lane received a step before; `above` holds the last row of the band before."""
    rb = w * bpp
    f = np.frombuffer(filtered, dtype=np.uint8).reshape(h, rb + 1).astype(np.int64)
    out = np.zeros((h, w, bpp), dtype=np.uint8)
    above = np.zeros((w, bpp), dtype=np.int64)
    lanes = np.arange(64)
    bad = False
    for row0 in range(0, h, 64):
        rows = row0 + lanes
        live = rows < h
        rr = np.minimum(rows, h - 1)
        ft = np.where(live, f[rr, 0], 0)
        bad |= bool((ft > 4).any())
        left = np.zeros((64, bpp), dtype=np.int64)
        corner = np.zeros((64, bpp), dtype=np.int64)
        mine = np.zeros((64, bpp), dtype=np.int64)
        for t in range(w + 63):
            x = t - lanes
            up = np.roll(mine, 1, axis=0)
            up[0] = above[t] if t < w else 0
            act = live & (x >= 0) & (x < w)
            xx = np.clip(x, 0, w - 1)
            raw = f[rr[:, None], 1 + xx[:, None] * bpp + np.arange(bpp)[None, :]]
            a, b, c = left, up, corner
            pa, pb, pc = np.abs(b - c), np.abs(a - c), np.abs(a + b - 2 * c)
            pth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
            k = ft[:, None]
            pred = np.where(k == 1, a, np.where(k == 2, b, np.where(k == 3, (a + b) >> 1, np.where(k == 4, pth, 0))))
            v = (raw + pred) & 255
            m = act[:, None]
            out[rr[act], xx[act]] = v[act]
            if act[63]:
                above[xx[63]] = v[63]  # 63 steps after lane 0 read it
            corner = np.where(m, up, corner)
            left = np.where(m, v, left)
            mine = np.where(m, v, mine)
    return out.reshape(h, rb), ST_FILTER if bad else 0


def decode_status(data: bytes, scheme: str = "plain") -> Tuple[Optional[np.ndarray], int]:
    """(pixels as np.asarray(Image.open(.)) shapes them, status) of a file `probe` accepts; a nonzero status leaves the pixels
    unspecified (None when the stream did not inflate)."""
    plan = probe(data)
    assert plan is not None, "not a file of the supported set"
    h, w, ch = plan["h"], plan["w"], plan["channels"]
    stream = b"".join(data[s:e] for s, e in plan["idat"])
    expect = h * (1 + w * ch)
    sink = DeviceSink(expect) if scheme == "device" else PlainSink(expect)
    status = inflate(stream, expect, sink)
    if status:
        return None, status  # the unfilter launch skips the image
    px, status = (unfilter_device if scheme == "device" else unfilter_plain)(sink.result(), h, w, ch)
    return (px.reshape(h, w) if ch == 1 else px.reshape(h, w, ch)), status


def decode(data: bytes) -> np.ndarray:
    px, status = decode_status(data)
    assert status == 0, status
    return px
