"""CPU: argument validation of dm4d_png_decode_u8, its size query and dm4d_vhull_pack_masks_u8.  Like every entry point they return
DM4D_ERR_ARG (-1) with a message in dm4d_last_error() BEFORE anything is launched: the "device" pointers are fake aligned addresses
that are never dereferenced, the descriptor's host copy is real."""
import ctypes

import numpy as np
import pytest

P = 0x10000
ERR_ARG = -1


@pytest.fixture(scope="module")
def lib():
    from diffuman4d_amd.host import lib as L
    return L.load()


def last(lib):
    return lib.dm4d_last_error().decode()


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def decode(lib, desc, streams_bytes=1 << 20, ws_bytes=1 << 30, out_bytes=1 << 30, streams=P, ws=P, status=P):
    desc = np.ascontiguousarray(desc, dtype=np.int64)
    return lib.dm4d_png_decode_u8(None, streams, streams_bytes, ptr(desc), P, len(desc), ws, ws_bytes, P, out_bytes, status)


#       stream bytes h   w   ch out och ws0
GOOD = [0, 100, 17, 33, 3, 0, 3, 0]
FILTERED = 17 * (1 + 33 * 3)  # 1700 -> 1712 in the workspace


def bad(**kw):
    d = list(GOOD)
    for k, v in kw.items():
        d[int(k[1:])] = v
    return [d]


def test_size_query(lib):
    assert lib.dm4d_png_decode_ws_bytes(1, 1) == 16
    assert lib.dm4d_png_decode_ws_bytes(1712, 48) == 1712
    for total, n in [(0, 1), (-1, 1), (16, 0), (16, 65536), ((1 << 40) + 1, 1)]:
        assert lib.dm4d_png_decode_ws_bytes(total, n) == 0


def test_decode_rejects_bad_arguments(lib):
    assert decode(lib, [GOOD], ws_bytes=1711) == ERR_ARG and "workspace too small" in last(lib)
    for h, w in [(0, 16), (16, 0), (16, 32768 // 3 + 1), (1 << 31, 16), (70000, 10922)]:
        assert decode(lib, bad(f2=h, f3=w)) == ERR_ARG and "dimension" in last(lib)
    for ch in (0, 2, 5):
        assert decode(lib, bad(f4=ch, f6=ch)) == ERR_ARG and "channels" in last(lib)
    assert decode(lib, bad(f6=4)) == ERR_ARG and "output channels" in last(lib)
    assert decode(lib, bad(f6=1)) == ERR_ARG and "output channels" in last(lib)
    assert decode(lib, bad(f1=1)) == ERR_ARG and "stream" in last(lib)
    assert decode(lib, bad(f1=1 << 28), streams_bytes=1 << 30) == ERR_ARG and "stream" in last(lib)
    assert decode(lib, bad(f0=2)) == ERR_ARG and "misaligned" in last(lib)
    assert decode(lib, bad(f0=-4)) == ERR_ARG and "stream" in last(lib)
    assert decode(lib, [GOOD], streams_bytes=99) == ERR_ARG and "stream" in last(lib)
    assert decode(lib, bad(f1=98), streams_bytes=99) == ERR_ARG and "padding" in last(lib)  # the words of a stream are read whole
    assert decode(lib, [GOOD], out_bytes=17 * 33 * 3 - 1) == ERR_ARG and "output buffer" in last(lib)
    assert decode(lib, bad(f5=-1)) == ERR_ARG and "output buffer" in last(lib)
    assert decode(lib, bad(f5=8), out_bytes=17 * 33 * 3 + 7) == ERR_ARG and "output buffer" in last(lib)
    assert decode(lib, bad(f7=16)) == ERR_ARG and "running sum" in last(lib)
    second = list(GOOD)
    second[0], second[5], second[7] = 100, 17 * 33 * 3, FILTERED  # not rounded up to 16
    assert decode(lib, [GOOD, second]) == ERR_ARG and "running sum" in last(lib)
    second[7] = 1712
    assert decode(lib, [GOOD, second], ws_bytes=2 * 1712 - 1) == ERR_ARG and "workspace too small" in last(lib)  # valid up to there
    desc = np.asarray([GOOD], dtype=np.int64)
    for n in (0, -1, 65536):
        assert lib.dm4d_png_decode_u8(None, P, 1 << 20, ptr(desc), P, n, P, 1 << 30, P, 1 << 30, P) == ERR_ARG and "batch" in last(lib)
    assert lib.dm4d_png_decode_u8(None, P, 1 << 20, None, P, 1, P, 1 << 30, P, 1 << 30, P) == ERR_ARG and "null" in last(lib)
    assert lib.dm4d_png_decode_u8(None, None, 1 << 20, ptr(desc), P, 1, P, 1 << 30, P, 1 << 30, P) == ERR_ARG and "null" in last(lib)
    assert lib.dm4d_png_decode_u8(None, P, 1 << 20, ptr(desc), P, 1, None, 1 << 30, P, 1 << 30, P) == ERR_ARG and "null" in last(lib)
    assert lib.dm4d_png_decode_u8(None, P, 1 << 20, ptr(desc), P, 1, P, 1 << 30, None, 1 << 30, P) == ERR_ARG and "null" in last(lib)
    assert lib.dm4d_png_decode_u8(None, P, 1 << 20, ptr(desc), P, 1, P, 1 << 30, P, 1 << 30, None) == ERR_ARG and "null" in last(lib)
    assert decode(lib, [GOOD], ws=P + 8) == ERR_ARG and "aligned" in last(lib)
    assert decode(lib, [GOOD], streams=P + 2) == ERR_ARG and "aligned" in last(lib)
    assert decode(lib, [GOOD], status=P + 2) == ERR_ARG and "aligned" in last(lib)


def test_pack_masks_u8_rejects_bad_arguments(lib):
    assert lib.dm4d_vhull_pack_masks_u8(None, P, P, 1, 4, 4, 0) == ERR_ARG and "threshold" in last(lib)
    assert lib.dm4d_vhull_pack_masks_u8(None, P, P, 1, 4, 4, 256) == ERR_ARG and "threshold" in last(lib)
    assert lib.dm4d_vhull_pack_masks_u8(None, None, P, 1, 4, 4, 128) == ERR_ARG and "null" in last(lib)
    assert lib.dm4d_vhull_pack_masks_u8(None, P, P, 0, 4, 4, 128) == ERR_ARG and "shape" in last(lib)
    assert lib.dm4d_vhull_pack_masks_u8(None, P + 1, P, 1, 4, 4, 128) == ERR_ARG and "aligned" in last(lib)
