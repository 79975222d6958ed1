"""CPU: argument validation of dm4d_jpeg_decode_u8 and its size query.  Like every entry point it returns DM4D_ERR_ARG (-1) with a
message in dm4d_last_error() BEFORE anything is launched: the "device" pointers are fake aligned addresses that are never
dereferenced, the descriptor / table host copies are real.  And the constants host/lib.py mirrors equal the header's."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import jpegdec_cases as cases

P = 0x10000
ERR_ARG = -1
FIELDS, TABLE_BYTES = 16, 1104


@pytest.fixture(scope="module")
def lib():
    from diffuman4d_amd.host import lib as L
    return L.load()


def last(lib):
    return lib.dm4d_last_error().decode()


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def good_tables(n=1):
    from diffuman4d_amd.host.jpegdec import probe
    t = np.frombuffer(probe(cases.supported()[12][1]).tables, dtype=np.uint8)
    return np.ascontiguousarray(np.tile(t, (n, 1)))


def decode(lib, desc, tab=None, scans_bytes=1 << 20, ws_bytes=1 << 30, out_bytes=1 << 30, scans=P, ws=P, status=P):
    desc = np.ascontiguousarray(desc, dtype=np.int64)
    tab = good_tables(len(desc)) if tab is None else tab
    return lib.dm4d_jpeg_decode_u8(None, scans, scans_bytes, ptr(desc), P, len(desc), ptr(tab), P, ws, ws_bytes, P, out_bytes, status)


#       scan bytes h   w   nc hs vs out ch block0
GOOD = [0, 100, 17, 33, 3, 2, 2, 0, 3, 0] + [0] * 6


def bad(**kw):
    d = list(GOOD)
    for k, v in kw.items():
        d[int(k[1:])] = v
    return [d]


def test_size_query(lib):
    assert lib.dm4d_jpeg_decode_ws_bytes(1, 1) == 128
    assert lib.dm4d_jpeg_decode_ws_bytes(6 * 720, 48) == 6 * 720 * 128
    for blocks, n in [(0, 1), (-1, 1), (1, 0), (1, 65536), ((1 << 25) + 1, 1)]:
        assert lib.dm4d_jpeg_decode_ws_bytes(blocks, n) == 0


def test_decode_rejects_bad_arguments(lib):
    assert decode(lib, [GOOD], ws_bytes=2 * 3 * 6 * 128 - 1) == ERR_ARG and "workspace too small" in last(lib)
    for h, w in [(0, 16), (16, 0), (65536, 16), (16, 65536)]:
        assert decode(lib, bad(f2=h, f3=w)) == ERR_ARG and "1..65535" in last(lib)
    for nc, hs, vs in [(2, 1, 1), (4, 1, 1), (1, 2, 2), (3, 1, 2), (3, 2, 4), (3, 4, 1), (3, 0, 0)]:
        assert decode(lib, bad(f4=nc, f5=hs, f6=vs)) == ERR_ARG and "supported set" in last(lib)
    assert decode(lib, bad(f8=1)) == ERR_ARG and "channels" in last(lib)  # one byte a pixel is for grayscale
    assert decode(lib, bad(f8=4)) == ERR_ARG and "channels" in last(lib)
    assert decode(lib, bad(f1=0)) == ERR_ARG and "scan" in last(lib)
    assert decode(lib, bad(f1=1 << 28), scans_bytes=1 << 30) == ERR_ARG and "scan" in last(lib)
    assert decode(lib, bad(f0=2)) == ERR_ARG and "misaligned" in last(lib)
    assert decode(lib, bad(f0=-4)) == ERR_ARG and "scan" in last(lib)
    assert decode(lib, [GOOD], scans_bytes=99) == ERR_ARG and "scan" in last(lib)
    assert decode(lib, [GOOD], out_bytes=17 * 33 * 3 - 1) == ERR_ARG and "output buffer" in last(lib)
    assert decode(lib, bad(f7=-1)) == ERR_ARG and "output buffer" in last(lib)
    assert decode(lib, bad(f9=1)) == ERR_ARG and "running sum" in last(lib)
    second = list(GOOD)
    second[0], second[7], second[9] = 100, 17 * 33 * 3, 2 * 3 * 6 - 1
    assert decode(lib, [GOOD, second]) == ERR_ARG and "running sum" in last(lib)
    assert decode(lib, bad(f12=7)) == ERR_ARG and "spare" in last(lib)
    gray = bad(f4=1, f5=1, f6=1, f8=1)
    assert decode(lib, gray, ws_bytes=3 * 5 * 128 - 1) == ERR_ARG and "workspace too small" in last(lib)  # valid up to the workspace
    desc = np.asarray([GOOD], dtype=np.int64)
    tab = good_tables()
    assert lib.dm4d_jpeg_decode_u8(None, P, 1 << 20, ptr(desc), P, 0, ptr(tab), P, P, 1 << 30, P, 1 << 30, P) == ERR_ARG and "batch" in last(lib)
    assert lib.dm4d_jpeg_decode_u8(None, P, 1 << 20, None, P, 1, ptr(tab), P, P, 1 << 30, P, 1 << 30, P) == ERR_ARG and "null" in last(lib)
    assert lib.dm4d_jpeg_decode_u8(None, P, 1 << 20, ptr(desc), P, 1, ptr(tab), P, P, 1 << 30, P, 1 << 30, None) == ERR_ARG and "null" in last(lib)
    assert decode(lib, [GOOD], ws=P + 8) == ERR_ARG and "aligned" in last(lib)
    assert decode(lib, [GOOD], scans=P + 2) == ERR_ARG and "aligned" in last(lib)
    assert decode(lib, [GOOD], status=P + 2) == ERR_ARG and "aligned" in last(lib)


def test_decode_rejects_bad_huffman_tables(lib):
    tab = good_tables()
    tab[0, 0] = 3  # three codes of length 1
    assert decode(lib, [GOOD], tab=tab) == ERR_ARG and "Huffman" in last(lib)
    tab = good_tables()
    tab[0, 16 + 3] = 16  # a DC category above 15
    assert decode(lib, [GOOD], tab=tab) == ERR_ARG and "Huffman" in last(lib)
    tab = good_tables()
    tab[0, 2 * 304 + 32 + 15] = 255  # the third component's AC table: more codes of length 16 than fit
    tab[0, 2 * 304 + 32 + 14] = 255
    assert decode(lib, [GOOD], tab=tab) == ERR_ARG and "Huffman" in last(lib)


def test_mirrored_constants_equal_the_header():
    from diffuman4d_amd.host import lib as L
    header = (Path(__file__).resolve().parent.parent / "include" / "dm4d.h").read_text()
    found = dict(re.findall(r"^#define DM4D_(JPEGDEC_\w+)[ \t]+(\S[^\n]*)$", header, flags=re.M))
    assert set(found) == {"JPEGDEC_FIELDS", "JPEGDEC_TABLE_BYTES", "JPEGDEC_SUB_BITS", "JPEGDEC_TILE_LANES", "JPEGDEC_MAX_SCAN_BYTES",
                          "JPEGDEC_ST_BAD_CODE", "JPEGDEC_ST_ZIGZAG", "JPEGDEC_ST_END", "JPEGDEC_ST_RANGE"}
    for name, text in found.items():
        m = re.fullmatch(r"\((\d+) << (\d+)\)|(\d+)", text.strip())
        value = int(m.group(1)) << int(m.group(2)) if m.group(1) else int(m.group(3))
        assert getattr(L, name) == value, name
    assert (L.JPEGDEC_FIELDS, L.JPEGDEC_TABLE_BYTES) == (FIELDS, TABLE_BYTES)
    from diffuman4d_amd.host import jpegdec
    assert jpegdec.MAX_SCAN_BYTES == L.JPEGDEC_MAX_SCAN_BYTES
