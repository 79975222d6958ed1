"""CPU: the definition of the device PNG encoder (tests/png_model.py) against independent decoders.  Every file must load in Pillow
(which verifies the chunk CRCs while zlib verifies the Adler-32) to exactly the input; every chunk CRC must be zlib.crc32's; the
concatenated IDAT data must inflate to the Paeth-filtered scanlines, which this file computes by the PNG specification's own loop."""
import functools
import heapq
import io
import struct
import zlib

import numpy as np
import pytest
from PIL import Image

import png_cases
import png_model as M


@functools.lru_cache(maxsize=None)
def all_cases():
    return png_cases.cases()


def names():
    return sorted(png_cases.cases())


def chunks(f: bytes):
    assert f[:8] == b"\x89PNG\r\n\x1a\n"
    at, out = 8, []
    while at < len(f):
        n, = struct.unpack(">I", f[at:at + 4])
        kind, data = f[at + 4:at + 8], f[at + 8:at + 8 + n]
        crc, = struct.unpack(">I", f[at + 8 + n:at + 12 + n])
        out.append((kind, data, crc))
        at += 12 + n
    assert at == len(f)
    return out


def spec_filter(img: np.ndarray) -> bytes:
    """Filter type 4 on every row, written as the specification's loop (bytes, not pixels: the left neighbour is bpp bytes back)."""
    h, w = img.shape[:2]
    bpp = 1 if img.ndim == 2 else img.shape[2]
    raw = img.reshape(h, w * bpp).tolist()
    prior, out = [0] * (w * bpp), bytearray()
    for row in raw:
        out.append(4)
        for i, x in enumerate(row):
            a = row[i - bpp] if i >= bpp else 0
            b = prior[i]
            c = prior[i - bpp] if i >= bpp else 0
            p = a + b - c
            pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
            out.append((x - (a if pa <= pb and pa <= pc else b if pb <= pc else c)) & 255)
        prior = row
    return bytes(out)


def unrestricted_depth(hist) -> int:
    """Depth of the deepest leaf of a Huffman tree of the non-zero counts (heapq: an implementation of its own)."""
    heap = [(c, 0) for c in hist if c > 0]
    heapq.heapify(heap)
    while len(heap) > 1:
        (c1, d1), (c2, d2) = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (c1 + c2, max(d1, d2) + 1))
    return heap[0][1]


def histogram(stripe) -> list:
    hist = [0] * 286
    for lit, length in M.tokens(stripe):
        hist[lit if length is None else M.length_symbol(length)[0]] += 1
    hist[256] = 1
    return hist


@pytest.mark.parametrize("name", names())
def test_model_file_decodes_to_the_input(name):
    from diffuman4d_amd.host import lib as L
    img = all_cases()[name]
    f = M.encode(img)
    im = Image.open(io.BytesIO(f))
    im.load()
    assert im.mode == ("L" if img.ndim == 2 else "RGBA") and im.size == (img.shape[1], img.shape[0])
    assert np.array_equal(np.asarray(im), img)
    cs = chunks(f)
    assert [k for k, _, _ in cs] == [b"IHDR"] + [b"IDAT"] * M.n_stripes(img.shape[0], img.shape[1], 1 if img.ndim == 2 else 4) + [b"IEND"]
    for kind, data, crc in cs:
        assert crc == zlib.crc32(kind + data)
    assert zlib.decompress(b"".join(d for k, d, _ in cs if k == b"IDAT")) == spec_filter(img) == M.paeth_filter(img).tobytes()
    bound = L.load().dm4d_png_bound(img.shape[0], img.shape[1], 1 if img.ndim == 2 else 4)
    assert bound == M.bound(img.shape[0], img.shape[1], 1 if img.ndim == 2 else 4) and len(f) <= bound


def test_premises_of_the_trap_cases():
    cs = all_cases()
    for kind in ("L", "RGBA"):
        noise = M.tokens(M.paeth_filter(cs[f"{kind}_noise"]))
        assert all(length is None for _, length in noise)                 # a stripe with no match at all
        assert any(length is not None for _, length in M.tokens(M.paeth_filter(cs[f"{kind}_constant"])))
        assert M.n_stripes(*cs[f"{kind}_striped"].shape[:2], 1 if kind == "L" else 4) == 3
    for n in png_cases.RUNS:
        filt = M.paeth_filter(cs[f"L_run{n}"]).reshape(-1)
        assert filt.tolist() == [4, 9, 200] + [77] * n + [31, 5]
    assert M.tokens(M.paeth_filter(cs["L_onerun"])) == [(4, None), (None, 258), (None, 258), (None, 84)]  # a stripe that is one run
    want = {2: [], 3: [], 258: [257], 259: [258], 260: [258], 261: [258], 516: [258, 257], 517: [258, 258]}
    for n, lengths in want.items():
        toks = M.tokens(M.paeth_filter(cs[f"L_run{n}"]))
        assert [length for _, length in toks if length is not None] == lengths
        assert sum(1 if length is None else length for _, length in toks) == n + 5
    # the Fibonacci-shaped histogram: an unrestricted Huffman code is deeper than 15 bits, the model's is not
    hist = histogram(M.paeth_filter(cs["L_fibonacci"]))
    assert sum(1 for c in hist if c) >= 17 and unrestricted_depth(hist) > 15
    assert max(M.code_lengths(hist, 15)) <= 15
    # the code-length alphabet's limit is exercised too
    assert max(M.code_lengths([1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89], 7)) <= 7 < unrestricted_depth([1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89])


def test_code_lengths_are_complete_prefix_codes():
    rng = np.random.default_rng(3)
    for _ in range(50):
        hist = (rng.integers(0, 2000, 286) * (rng.random(286) < rng.random())).tolist()
        hist[256] = 1
        hist[0] += 1
        lens = M.code_lengths(hist, 15)
        assert all((c > 0) == (v > 0) for c, v in zip(hist, lens)) and max(lens) <= 15
        assert sum(2 ** (15 - v) for v in lens if v) == 2 ** 15  # Kraft with equality: a complete code
    assert M.code_lengths([0, 7, 0], 15) == [0, 1, 0]


def test_bound_is_zero_out_of_range():
    from diffuman4d_amd.host import lib as L
    lib = L.load()
    for h, w, ch in [(0, 1, 1), (1, 0, 1), (16385, 1, 1), (1, 16385, 4), (1, 1, 3), (1, 1, 0), (-1, 5, 4)]:
        assert lib.dm4d_png_bound(h, w, ch) == 0 and M.bound(h, w, ch) == 0
    assert lib.dm4d_png_bound(16384, 16384, 4) == M.bound(16384, 16384, 4) > 0


def test_size_against_zlib_rle_on_a_result_like_pair():
    """The model's files are at most 1.10 x what zlib itself makes of the same filtered bytes under the same scheme (level 6, Z_RLE:
    distance-1 matches only, dynamic Huffman) plus the PNG framing.  The margin covers fixed stripes against zlib's adaptive block
    splitting and the per-stripe code tables."""
    rgb, mask = png_cases.result_like(256, 320)
    for img in (np.dstack([rgb, mask]), mask):
        f = M.encode(img)
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(f))), img)
        co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
        ref = len(co.compress(M.paeth_filter(img).tobytes()) + co.flush()) + 8 + 25 + 12 + 12
        print(f"{'RGBA' if img.ndim == 3 else 'L'}: model {len(f)} bytes, zlib Z_RLE {ref} bytes, ratio {len(f) / ref:.4f}")
        assert len(f) <= 1.10 * ref
