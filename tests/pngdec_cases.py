"""The files that tests/test_pngdec_cpu.py (the model against Pillow) and tests/test_pngdec_gpu.py (the device against Pillow and
the model) share, all built in memory: hand-filtered rows compressed with zlib, hand-coded DEFLATE blocks, Pillow's own files and
the files of the device encoder's model (tests/png_model.py).  Deterministic.  The cases are the smallest at which each mechanism
of csrc/pngdec.hip can go wrong: band seams of the unfilter wavefront (heights around 64 and 128), the five filters with ties and
carries, stored / fixed / dynamic blocks, the longest codes, the ring's wrap (output above 64 KiB and 128 KiB), the farthest and
the nearest match, IDAT payloads cut anywhere."""
import functools
import io
import struct
import zlib
from typing import List, Sequence, Tuple

import numpy as np
from PIL import Image

import png_cases
import png_model
from pngdec_model import DIST_BASE, DIST_EXTRA, FIXED_LENS

SIGNATURE = b"\x89PNG\r\n\x1a\n"
COLOUR = {1: 0, 3: 2, 4: 6}
WIDTHS = (1, 2, 63, 64, 65)
HEIGHTS = (1, 63, 64, 65, 129)


# -- container -----------------------------------------------------------------------------------------------------------------------
def chunk(kind: bytes, body: bytes) -> bytes:
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def ihdr(h: int, w: int, bpp: int, depth: int = 8, colour=None, interlace: int = 0, compression: int = 0, filtering: int = 0) -> bytes:
    return chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, COLOUR[bpp] if colour is None else colour, compression, filtering, interlace))


def png(h: int, w: int, bpp: int, stream: bytes, cuts: Sequence[int] = (), before: bytes = b"", after: bytes = b"") -> bytes:
    """A file around a zlib stream; `cuts` are the positions at which the stream is split into IDAT chunks."""
    edges = [0, *cuts, len(stream)]
    idat = b"".join(chunk(b"IDAT", stream[a:b]) for a, b in zip(edges[:-1], edges[1:]))
    return SIGNATURE + ihdr(h, w, bpp) + before + idat + after + chunk(b"IEND", b"")


def split_chunks(data: bytes) -> List[Tuple[bytes, bytes]]:
    out, pos = [], 8
    while pos < len(data):
        n, kind = struct.unpack_from(">I4s", data, pos)
        out.append((kind, data[pos + 8:pos + 8 + n]))
        pos += 12 + n
    return out


def join_chunks(chunks) -> bytes:
    return SIGNATURE + b"".join(chunk(k, b) for k, b in chunks)


def idat_stream(data: bytes) -> bytes:
    return b"".join(b for k, b in split_chunks(data) if k == b"IDAT")


def with_stream(data: bytes, stream: bytes) -> bytes:
    """The file with its IDAT payload replaced (one chunk, CRC recomputed)."""
    out, done = [], False
    for k, b in split_chunks(data):
        if k != b"IDAT":
            out.append((k, b))
        elif not done:
            out.append((k, stream))
            done = True
    return join_chunks(out)


# -- filters -------------------------------------------------------------------------------------------------------------------------
def _paeth(a, b, c):
    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
    return a if pa <= pb and pa <= pc else b if pb <= pc else c


def filter_rows(img: np.ndarray, types: Sequence[int]) -> bytes:
    """The filtered scanlines of uint8 [h, w] or [h, w, bpp] with row y filtered by types[y % len(types)], by hand."""
    h = img.shape[0]
    bpp = 1 if img.ndim == 2 else img.shape[2]
    rows = img.reshape(h, -1).astype(np.int64)
    rb = rows.shape[1]
    out = bytearray()
    for y in range(h):
        t = types[y % len(types)]
        cur = rows[y]
        up = rows[y - 1] if y else np.zeros(rb, dtype=np.int64)
        left = np.concatenate([np.zeros(bpp, dtype=np.int64), cur[:-bpp]]) if rb > bpp else np.zeros(rb, dtype=np.int64)
        corner = np.concatenate([np.zeros(bpp, dtype=np.int64), up[:-bpp]]) if rb > bpp else np.zeros(rb, dtype=np.int64)
        if t == 0:
            pred = np.zeros(rb, dtype=np.int64)
        elif t == 1:
            pred = left
        elif t == 2:
            pred = up
        elif t == 3:
            pred = (left + up) >> 1
        else:
            pred = np.array([_paeth(int(a), int(b), int(c)) for a, b, c in zip(left, up, corner)], dtype=np.int64)
        out.append(t)
        out += ((cur - pred) & 255).astype(np.uint8).tobytes()
    return bytes(out)


def image(kind: str, h: int, w: int, bpp: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    shape = (h, w) if bpp == 1 else (h, w, bpp)
    if kind == "noise":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if kind == "extremes":  # Average with carries (255 + 255), Paeth ties (equal neighbours)
        return rng.choice(np.array([0, 1, 127, 128, 254, 255], dtype=np.uint8), size=shape)
    if kind == "ties":  # every pixel equals a neighbour: pa == pb == pc over and over
        a = np.repeat(np.repeat(rng.integers(0, 256, ((h + 1) // 2, (w + 1) // 2) + shape[2:], dtype=np.uint8), 2, axis=0), 2, axis=1)
        return np.ascontiguousarray(a[:h, :w])
    y, x = np.mgrid[0:h, 0:w]
    base = (x * 3 + y * 5 + (x * y) // 7) & 255
    if bpp == 1:
        return base.astype(np.uint8)
    return np.stack([(base + 40 * c) & 255 for c in range(bpp)], axis=-1).astype(np.uint8)


def by_hand(img: np.ndarray, types: Sequence[int], level: int = 6, **kw) -> bytes:
    bpp = 1 if img.ndim == 2 else img.shape[2]
    co = zlib.compressobj(level, **kw)
    raw = filter_rows(img, types)
    return png(img.shape[0], img.shape[1], bpp, co.compress(raw) + co.flush())


def by_pillow(img: np.ndarray, **kw) -> bytes:
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="PNG", **kw)
    return buf.getvalue()


# -- DEFLATE by hand -----------------------------------------------------------------------------------------------------------------
class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, value: int, n: int):  # least significant bit first
        self.acc |= value << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code: int, n: int):  # a Huffman code: first bit first
        self.bits(int(format(code, f"0{n}b")[::-1], 2), n)

    def done(self) -> bytes:
        if self.n:
            self.bits(0, 8 - self.n)
        return bytes(self.out)


def canonical(lens):
    """{symbol: (code, length)} of a canonical code"""
    out, code = {}, 0
    for l in range(1, 16):
        for s, sl in enumerate(lens):
            if sl == l:
                out[s] = (code, l)
                code += 1
        code <<= 1
    return out


def _tokens(bw: BitWriter, tokens, lit, dist):
    """tokens: ints = literals, (length, distance) = matches, ("lit", symbol) = a raw literal/length symbol, (length, (symbol,)) = a
    match whose distance is the raw distance symbol without extra bits; the end-of-block code follows"""
    for t in tokens:
        if isinstance(t, int):
            bw.code(*lit[t])
        elif t[0] == "lit":
            bw.code(*lit[t[1]])
        else:
            length, d = t
            k = max(i for i, b in enumerate(png_model.LEN_BASE) if b <= length)
            bw.code(*lit[257 + k])
            bw.bits(length - png_model.LEN_BASE[k], png_model.LEN_EXTRA[k])
            if isinstance(d, tuple):  # a raw distance symbol
                bw.code(*dist[d[0]])
                continue
            j = max(i for i, b in enumerate(DIST_BASE) if b <= d)
            bw.code(*dist[j])
            bw.bits(d - DIST_BASE[j], DIST_EXTRA[j])
    bw.code(*lit[256])


def fixed_block(bw: BitWriter, tokens, last: bool = True):
    bw.bits(int(last), 1)
    bw.bits(1, 2)
    _tokens(bw, tokens, canonical(FIXED_LENS[:288]), canonical(FIXED_LENS[288:]))


def dynamic_block(bw: BitWriter, tokens, lit_lens, dist_lens, last: bool = True):
    """A dynamic block whose header spells every code length out (code-length code: symbols 0 .. 15 in 4 bits each)."""
    bw.bits(int(last), 1)
    bw.bits(2, 2)
    bw.bits(len(lit_lens) - 257, 5)
    bw.bits(len(dist_lens) - 1, 5)
    bw.bits(19 - 4, 4)
    for s in png_model.CL_ORDER:
        bw.bits(4 if s < 16 else 0, 3)
    cl = canonical([4] * 16)
    for l in list(lit_lens) + list(dist_lens):
        bw.code(*cl[l])
    _tokens(bw, tokens, canonical(lit_lens), canonical(dist_lens))


CL_COMPLETE = [4] * 13 + [5] * 6  # a complete code-length code over all 19 symbols: 13 / 16 + 6 / 32


def dynamic_header(nl: int, nd: int, cl_lens, seq) -> BitWriter:
    """The header of a final dynamic block by hand: HLIT / HDIST from nl / nd, the code-length code's 19 lengths `cl_lens` (by symbol),
    then `seq` = [(code-length symbol, value of its extra bits)]."""
    bw = BitWriter()
    bw.bits(1, 1), bw.bits(2, 2), bw.bits(nl - 257, 5), bw.bits(nd - 1, 5), bw.bits(19 - 4, 4)
    for s in png_model.CL_ORDER:
        bw.bits(cl_lens[s], 3)
    cl = canonical(cl_lens)
    for sym, extra in seq:
        bw.code(*cl[sym])
        if sym >= 16:
            bw.bits(extra, {16: 2, 17: 3, 18: 7}[sym])
    return bw


def complete_lit_lens() -> list:
    """286 literal/length code lengths of a complete code: the fixed code's, with the two 8-bit codes that 286 and 287 would have had
    given to 284 and 285 (7 bits each)."""
    lens = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 6
    lens[284], lens[285] = 7, 7
    return lens


def zwrap(deflate: bytes, raw: bytes, adler=None) -> bytes:
    return b"\x78\x9c" + deflate + struct.pack(">I", zlib.adler32(raw) if adler is None else adler)


def far_match() -> bytes:
    """130 rows of 256 bytes: the last 512 bytes are a copy of the first 512, at distance 32768 (zlib itself never looks that far)."""
    rng = np.random.default_rng(77)
    raw = bytearray(rng.integers(0, 256, 32768, dtype=np.uint8).tobytes())
    raw[0::256] = bytes(128)  # the filter bytes: None
    co = zlib.compressobj(6, wbits=-15)
    first = co.compress(bytes(raw)) + co.flush(zlib.Z_FULL_FLUSH)  # ends on a byte boundary, not final
    bw = BitWriter()
    fixed_block(bw, [(258, 32768), (254, 32768)])
    full = bytes(raw) + bytes(raw[:512])
    return png(130, 255, 1, zwrap(first + bw.done(), full))


def one_distance_code(n_codes: int) -> bytes:
    """A dynamic block whose distance set has one 1-bit code (incomplete, accepted) or no code at all (all literals)."""
    h, w = 3, 40
    if n_codes == 1:
        raw = bytes([0] + [9] * w) * h  # per row: a literal 0, a literal 9, then a match at distance 1
        tokens = [0, 9, (w - 1, 1)] * h
        dist_lens = [1]
    else:
        raw = bytes([0] + list(range(1, w + 1))) * h
        tokens = list(raw)
        dist_lens = [0]
    lit_lens = complete_lit_lens()
    bw = BitWriter()
    dynamic_block(bw, tokens, lit_lens, dist_lens)
    return png(h, w, 1, zwrap(bw.done(), raw))


def soft_mask(h: int, w: int) -> np.ndarray:
    from PIL import ImageFilter
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    inside = ((x - w / 2) / (0.33 * w)) ** 2 + ((y - h / 2) / (0.42 * h)) ** 2 <= 1.0
    return np.asarray(Image.fromarray((inside * 255).astype(np.uint8)).filter(ImageFilter.GaussianBlur(3)))


@functools.lru_cache(maxsize=None)
def supported() -> List[Tuple[str, bytes]]:
    out = []
    seed = 0
    for bpp in (1, 3, 4):
        for h in HEIGHTS:
            for w in WIDTHS:
                seed += 1
                out.append((f"{h}x{w}x{bpp}-mix", by_hand(image("extremes" if seed % 2 else "noise", h, w, bpp, seed), (4, 3, 2, 1, 0, 4, 4, 3))))
        for t in range(5):
            out.append((f"37x29x{bpp}-filter{t}", by_hand(image("extremes", 37, 29, bpp, 100 + t), (t,))))
            out.append((f"70x33x{bpp}-filter{t}-ties", by_hand(image("ties", 70, 33, bpp, 200 + t), (t,))))
        out.append((f"66x35x{bpp}-smooth-mix", by_hand(image("smooth", 66, 35, bpp, 0), (0, 1, 2, 3, 4))))
    noise300 = image("noise", 300, 300, 1, 300)
    smooth520 = image("smooth", 260, 520, 1, 0)
    out.append(("300x300-stored", by_pillow(noise300, compress_level=0)))  # 90 300 bytes: several stored blocks, the ring wraps
    out.append(("40x50x3-stored", by_pillow(image("noise", 40, 50, 3, 301), compress_level=0)))
    out.append(("300x300-fixed", by_hand(image("smooth", 300, 300, 1, 0), (1, 2, 4), strategy=zlib.Z_FIXED)))
    out.append(("65x40x4-fixed-noise", by_hand(image("noise", 65, 40, 4, 302), (0,), strategy=zlib.Z_FIXED)))
    for level in (1, 6, 9):
        out.append((f"260x520-level{level}", by_pillow(smooth520, compress_level=level)))  # 135 460 bytes: the ring wraps twice
        out.append((f"100x90x3-level{level}", by_pillow(image("smooth", 100, 90, 3, 0), compress_level=level)))
    out.append(("260x520-optimize", by_pillow(smooth520, optimize=True)))
    out.append(("300x300-noise", by_pillow(noise300)))  # all literals
    out.append(("260x520-noise", by_pillow(image("noise", 260, 520, 1, 303))))
    # several dynamic blocks: a full flush after every part (each leaves an empty stored block behind, too)
    raw = filter_rows(image("smooth", 120, 200, 3, 0), (4, 1))
    co = zlib.compressobj(6)
    parts = b"".join(co.compress(raw[a:a + 9001]) + co.flush(zlib.Z_FULL_FLUSH) for a in range(0, len(raw), 9001)) + co.flush()
    out.append(("120x200x3-blocks", png(120, 200, 3, parts)))
    out.append(("300x300-constant", by_hand(np.full((300, 300), 201, dtype=np.uint8), (0,), level=9)))  # distance 1, length 258
    out.append(("64x64x4-constant", by_hand(np.full((64, 64, 4), 7, dtype=np.uint8), (2,))))
    out.append(("130x255-far-match", far_match()))
    out.append(("3x40-one-distance-code", one_distance_code(1)))
    out.append(("3x40-no-distance-code", one_distance_code(0)))
    out.append(("fibonacci", png_model.encode(png_cases.fibonacci_image())))  # 15-bit codes
    rgb, mask = png_cases.result_like(96, 120)
    out.append(("96x120-result-rgb", by_pillow(rgb)))
    out.append(("96x120-result-mask", by_pillow(mask)))
    out.append(("200x230-soft-mask", by_pillow(soft_mask(200, 230))))
    out.append(("encoder-L", png_model.encode(png_cases.striped("L"))))
    out.append(("encoder-RGBA", png_model.encode(np.dstack([rgb, mask]))))
    # the container: IDAT cut everywhere, ancillary chunks, bytes after the stream
    base = by_pillow(image("smooth", 70, 65, 3, 0))
    stream = idat_stream(base)
    out.append(("70x65x3-idat-bytes", png(70, 65, 3, stream, cuts=list(range(1, 40)) + [41, 41, 100, len(stream) - 1])))  # an empty chunk too
    text = chunk(b"tEXt", b"Comment\0built by hand")
    out.append(("70x65x3-ancillary", png(70, 65, 3, stream, before=chunk(b"gAMA", struct.pack(">I", 45455)) + chunk(b"pHYs", struct.pack(">IIB", 2835, 2835, 1)) + text,
                                         after=text + chunk(b"tIME", struct.pack(">HBBBBB", 2024, 1, 2, 3, 4, 5)))))
    out.append(("70x65x3-trailing", png(70, 65, 3, stream + b"\x00\xff\x55 trailing")))
    return out


# -- files the device does not take ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def unsupported() -> List[Tuple[str, bytes]]:
    rng = np.random.default_rng(9)
    g = rng.integers(0, 256, (20, 30), dtype=np.uint8)
    rgb = rng.integers(0, 256, (20, 30, 3), dtype=np.uint8)
    good = by_pillow(rgb)
    chunks = split_chunks(good)
    stream = idat_stream(good)
    out = [("palette", _save(Image.fromarray(rgb).quantize(16), bits=8))]
    out.append(("1-bit", _save(Image.fromarray(g > 128))))
    out.append(("16-bit", _save(Image.fromarray(g.astype(np.uint16) * 257))))
    out.append(("gray-alpha", _save(Image.fromarray(np.dstack([g, g]), "LA"))))
    out.append(("4-bit-palette", _save(Image.fromarray(rgb).quantize(16), bits=4)))
    # Adam7: the header says so (Pillow writes no interlaced files; it refuses or decodes this one on its own route)
    out.append(("interlaced", SIGNATURE + ihdr(20, 30, 3, interlace=1) + chunk(b"IDAT", stream) + chunk(b"IEND", b"")))
    out.append(("compression-method", SIGNATURE + ihdr(20, 30, 3, compression=1) + chunk(b"IDAT", stream) + chunk(b"IEND", b"")))
    out.append(("filter-method", SIGNATURE + ihdr(20, 30, 3, filtering=1) + chunk(b"IDAT", stream) + chunk(b"IEND", b"")))
    bad_crc = bytearray(good)
    bad_crc[-5 - 12] ^= 1  # the last byte of the IDAT chunk's CRC
    out.append(("bad-crc", bytes(bad_crc)))
    out.append(("ihdr-not-first", SIGNATURE + chunk(b"gAMA", struct.pack(">I", 45455)) + b"".join(chunk(k, b) for k, b in chunks)))
    out.append(("no-idat", join_chunks([c for c in chunks if c[0] != b"IDAT"])))
    half = len(stream) // 2
    out.append(("idat-not-consecutive", SIGNATURE + ihdr(20, 30, 3) + chunk(b"IDAT", stream[:half]) + chunk(b"tEXt", b"k\0v") +
                chunk(b"IDAT", stream[half:]) + chunk(b"IEND", b"")))
    out.append(("no-iend", join_chunks([c for c in chunks if c[0] != b"IEND"])))
    out.append(("zero-width", SIGNATURE + ihdr(20, 0, 3) + chunk(b"IDAT", stream) + chunk(b"IEND", b"")))
    wide = np.zeros((1, 32768 // 3 + 1, 3), dtype=np.uint8)
    out.append(("row-too-long", by_pillow(wide)))
    out.append(("trns", join_chunks([chunks[0], (b"tRNS", bytes(6))] + chunks[1:])))
    out.append(("apng", join_chunks([chunks[0], (b"acTL", struct.pack(">II", 1, 0))] + chunks[1:])))
    out.append(("cgbi", SIGNATURE + chunk(b"CgBI", bytes(4)) + b"".join(chunk(k, b) for k, b in chunks)))
    out.append(("truncated-file", good[:len(good) // 2]))
    out.append(("not-a-png", b"\xff\xd8\xff\xe0" + bytes(64)))
    return out


def _save(im, **kw) -> bytes:
    buf = io.BytesIO()
    im.save(buf, format="PNG", **kw)
    return buf.getvalue()


# -- files `probe` accepts and the decoder must flag ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def malformed() -> List[Tuple[str, bytes, int]]:
    """(name, file, the status bit it must raise), one per bit of DM4D_PNGDEC_ST_*, then further ones per rule."""
    import pngdec_model as M
    img = image("smooth", 40, 33, 1, 0)
    good = by_hand(img, (4, 1, 2), level=6)
    stream = idat_stream(good)
    raw = filter_rows(img, (4, 1, 2))
    h, w = img.shape
    out = []
    out.append(("zlib-fcheck", with_stream(good, b"\x78\x9d" + stream[2:]), M.ST_HEADER))
    out.append(("block-type-3", png(h, w, 1, b"\x78\x9c" + bytes([0b111]) + bytes(40)), M.ST_BLOCK))
    bw = BitWriter()
    fixed_block(bw, [0, 1, 2, ("lit", 286)])
    out.append(("reserved-literal", png(h, w, 1, zwrap(bw.done(), raw)), M.ST_CODE))
    bw = BitWriter()
    fixed_block(bw, [0, 1, 2, (3, 4)])
    out.append(("distance-too-far", png(h, w, 1, zwrap(bw.done(), raw)), M.ST_DISTANCE))
    out.append(("truncated-stream", with_stream(good, stream[:len(stream) // 2]), M.ST_END))
    out.append(("adler", with_stream(good, stream[:-1] + bytes([stream[-1] ^ 1])), M.ST_ADLER))
    bad_filter = bytearray(raw)
    bad_filter[(w + 1) * 7] = 5
    out.append(("filter-5", png(h, w, 1, zlib.compress(bytes(bad_filter))), M.ST_FILTER))
    # further rules
    out.append(("zlib-method", with_stream(good, bytes([0x79, (31 - 0x7900 % 31) % 31]) + stream[2:]), M.ST_HEADER))
    out.append(("zlib-dictionary", with_stream(good, b"\x78" + bytes([0x20 + (31 - (0x7820 % 31)) % 31]) + stream[2:]), M.ST_HEADER))
    out.append(("stored-length", png(h, w, 1, b"\x78\x9c" + bytes([1]) + struct.pack("<HH", 5, 5) + bytes(40)), M.ST_BLOCK))
    short = zlib.compress(raw[:-(w + 1)])
    out.append(("stream-too-short", png(h, w, 1, short), M.ST_END))
    out.append(("stream-too-long", png(h, w, 1, zlib.compress(raw + raw[:w + 1])), M.ST_END))
    bw = BitWriter()
    fixed_block(bw, [0, 1, 2, (3, (30,))])
    out.append(("reserved-distance", png(h, w, 1, zwrap(bw.done(), raw)), M.ST_CODE))
    bw = BitWriter()
    ok = complete_lit_lens()
    dynamic_block(bw, [0, 1], ok[:284] + [8, 8], [1])  # incomplete literal/length set: two 8-bit codes are missing
    out.append(("incomplete-set", png(h, w, 1, zwrap(bw.done(), raw)), M.ST_BLOCK))
    bw = BitWriter()
    dynamic_block(bw, [1], [7] + ok[1:], [1])
    out.append(("over-subscribed-set", png(h, w, 1, zwrap(bw.done(), raw)), M.ST_BLOCK))
    # the rules of a dynamic block's header, one file each
    many = [(18, 127), (18, 127)]  # 138 zeros twice: past the 258 lengths
    no_eob = [(8, 0)] * 256 + [(0, 0), (0, 0)]  # a complete set of 256 literals, nothing for symbol 256
    for name, args in (("hlit-287", (287, 1, CL_COMPLETE, [])), ("hdist-31", (257, 31, CL_COMPLETE, [])),
                       ("repeat-without-previous", (257, 1, CL_COMPLETE, [(16, 0)])), ("repeat-past-the-end", (257, 1, CL_COMPLETE, many)),
                       ("no-end-of-block", (257, 1, CL_COMPLETE, no_eob)),
                       ("incomplete-code-length-code", (257, 1, [4] * 15 + [0] * 4, [])),
                       ("over-subscribed-code-length-code", (257, 1, [4] * 16 + [1, 0, 0], []))):
        out.append((name, png(h, w, 1, zwrap(dynamic_header(*args).done() + bytes(16), raw)), M.ST_BLOCK))
    # an undefined code: the distance set has the single code 0; a match that sends the bit 1
    bw = BitWriter()
    bw.bits(1, 1), bw.bits(2, 2), bw.bits(286 - 257, 5), bw.bits(0, 5), bw.bits(15, 4)
    for s in png_model.CL_ORDER:
        bw.bits(4 if s < 16 else 0, 3)
    cl = canonical([4] * 16)
    for l in ok + [1]:
        bw.code(*cl[l])
    codes = canonical(ok)
    bw.code(*codes[0]), bw.code(*codes[257]), bw.bits(1, 1)
    out.append(("undefined-distance-code", png(h, w, 1, zwrap(bw.done() + bytes(8), raw)), M.ST_CODE))
    return out


def mutations(n: int = 160, seed: int = 1234) -> List[Tuple[str, bytes]]:
    """Single-byte mutations of the IDAT data of a few supported files, CRC recomputed."""
    rng = np.random.default_rng(seed)
    bases = [d for name, d in supported() if name in ("66x35x1-smooth-mix", "66x35x3-smooth-mix", "40x50x3-stored", "65x40x4-fixed-noise",
                                                       "100x90x3-level9", "3x40-one-distance-code", "96x120-result-mask")]
    out = []
    for i in range(n):
        data = bases[i % len(bases)]
        stream = bytearray(idat_stream(data))
        at = int(rng.integers(len(stream))) if i % 3 else int(rng.integers(min(len(stream), 24)))  # a third of them in the headers
        stream[at] ^= 1 << int(rng.integers(8)) if i % 2 else int(rng.integers(1, 256))
        out.append((f"mutation{i}@{at}", with_stream(data, bytes(stream))))
    return out
