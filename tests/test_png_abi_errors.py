"""CPU: argument validation of dm4d_png_encode_u8 and its size queries.  Like every entry point it returns DM4D_ERR_ARG (-1) with a
message in dm4d_last_error() BEFORE anything is launched: the "device" pointers are fake aligned addresses that are never dereferenced,
the descriptor host copy is real."""
import ctypes

import numpy as np
import pytest

import png_model as M

P = 0x10000
ERR_ARG = -1
L_KIND, RGBA_KIND = 0, 1


@pytest.fixture(scope="module")
def lib():
    from diffuman4d_amd.host import lib as L
    return L.load()


def last(lib):
    return lib.dm4d_last_error().decode()


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def row(kind, h, w, pix=0, pstride=None, alpha=0, astride=None, filt0=0, stripe0=0, spare=0):
    pstride = (w * (3 if kind == RGBA_KIND else 1)) if pstride is None else pstride
    astride = (w if kind == RGBA_KIND else 0) if astride is None else astride
    return [kind, h, w, pix, pstride, alpha, astride, filt0, stripe0, 0, 0, 0, 0, 0, 0, spare]


def encode(lib, desc, planes=P, planes_bytes=1 << 20, rgb=P, rgb_bytes=1 << 20, ws=P, ws_bytes=1 << 30, blob=P, blob_bytes=1 << 30, out=P,
           desc_dev=P, n=None):
    desc = np.ascontiguousarray(desc, dtype=np.int64)
    return lib.dm4d_png_encode_u8(None, planes, planes_bytes, rgb, rgb_bytes, ptr(desc), desc_dev, len(desc) if n is None else n, ws, ws_bytes,
                                  blob, blob_bytes, out)


def test_size_queries(lib):
    from diffuman4d_amd.host import lib as L
    assert L.PNG_STRIPE_BYTES == M.STRIPE_BYTES and L.MATTING_MAX_SIDE == M.MAX_SIDE
    for h, w, ch in [(1, 1, 1), (1, 1, 4), (17, 19, 4), (2448, 2048, 4), (2448, 2048, 1), (16384, 16384, 4)]:
        assert lib.dm4d_png_bound(h, w, ch) == M.bound(h, w, ch) > 0
    for h, w, ch in [(0, 8, 1), (8, 0, 1), (16385, 8, 1), (8, 16385, 4), (8, 8, 2), (8, 8, 3), (-1, 8, 1)]:
        assert lib.dm4d_png_bound(h, w, ch) == 0
    assert lib.dm4d_png_ws_bytes(0, 1, 1) == 0 and lib.dm4d_png_ws_bytes(2, 0, 1) == 0 and lib.dm4d_png_ws_bytes(2, 1, 0) == 0
    assert lib.dm4d_png_ws_bytes(2, 1, 65536) == 0 and lib.dm4d_png_ws_bytes(100, 1, 2) == 0
    one = lib.dm4d_png_ws_bytes(2, 1, 1)
    assert one >= 2 + 4 + L.PNG_STRIPE_REC + 4 + 4 and one % 16 == 0
    assert lib.dm4d_png_ws_bytes(1 << 20, 40, 3) >= 3 * (1 << 20) + 40 * L.PNG_STRIPE_REC


def test_encode_rejects_bad_arguments(lib):
    ok = [row(L_KIND, 16, 16)]
    for kw in (dict(planes=None), dict(ws=None), dict(blob=None), dict(out=None), dict(desc_dev=None)):
        assert encode(lib, ok, **kw) == ERR_ARG and "null" in last(lib)
    assert lib.dm4d_png_encode_u8(None, P, 1 << 20, P, 0, None, P, 1, P, 1 << 30, P, 1 << 30, P) == ERR_ARG and "null" in last(lib)
    assert encode(lib, [row(RGBA_KIND, 16, 16)], rgb=None, rgb_bytes=0) == ERR_ARG and "outside its buffer" in last(lib)
    assert encode(lib, ok, n=0) == ERR_ARG and "batch" in last(lib)
    assert encode(lib, ok, n=65536) == ERR_ARG and "batch" in last(lib)
    assert encode(lib, ok, ws=P + 4) == ERR_ARG and "aligned" in last(lib)
    assert encode(lib, ok, out=P + 4) == ERR_ARG and "aligned" in last(lib)
    assert encode(lib, ok, planes_bytes=0) == ERR_ARG and "not positive" in last(lib)
    # sizes of 0 or above the maximum, and a kind that does not exist
    for h, w in [(0, 16), (16, 0), (M.MAX_SIDE + 1, 16), (16, M.MAX_SIDE + 1), (-1, 16)]:
        for kind in (L_KIND, RGBA_KIND):
            assert encode(lib, [row(kind, h, w)], planes_bytes=1 << 40, rgb_bytes=1 << 40) == ERR_ARG and "dimension" in last(lib)
    assert encode(lib, [row(2, 16, 16)]) == ERR_ARG and "kind" in last(lib)
    # a plane outside its buffer
    assert encode(lib, ok, planes_bytes=255) == ERR_ARG and "outside its buffer" in last(lib)
    assert encode(lib, [row(L_KIND, 16, 16, pix=1)], planes_bytes=256) == ERR_ARG and "outside its buffer" in last(lib)
    assert encode(lib, [row(L_KIND, 16, 16, pix=-1)]) == ERR_ARG and "outside its buffer" in last(lib)
    assert encode(lib, [row(L_KIND, 16, 16, pstride=15)]) == ERR_ARG and "outside its buffer" in last(lib)
    assert encode(lib, [row(L_KIND, 16, 16, pstride=20)], planes_bytes=15 * 20 + 15) == ERR_ARG and "outside its buffer" in last(lib)
    assert encode(lib, [row(L_KIND, 16, 16, alpha=1)]) == ERR_ARG and "outside its buffer" in last(lib)
    assert encode(lib, [row(RGBA_KIND, 16, 16)], rgb_bytes=16 * 48 - 1) == ERR_ARG and "outside its buffer" in last(lib)
    assert encode(lib, [row(RGBA_KIND, 16, 16)], planes_bytes=255) == ERR_ARG and "outside its buffer" in last(lib)
    assert encode(lib, [row(RGBA_KIND, 16, 16, pstride=47)]) == ERR_ARG and "outside its buffer" in last(lib)
    assert encode(lib, [row(RGBA_KIND, 16, 16, alpha=241)], planes_bytes=256 + 240) == ERR_ARG and "outside its buffer" in last(lib)
    # running sums and spare fields
    assert encode(lib, [row(L_KIND, 16, 16, filt0=1)]) == ERR_ARG and "running sum" in last(lib)
    assert encode(lib, [row(L_KIND, 16, 16, stripe0=1)]) == ERR_ARG and "running sum" in last(lib)
    two = [row(L_KIND, 16, 16), row(RGBA_KIND, 16, 16, filt0=16 * 17, stripe0=2)]
    assert encode(lib, two) == ERR_ARG and "running sum" in last(lib)
    two[1][8] = 1
    two[1][7] += 1
    assert encode(lib, two) == ERR_ARG and "running sum" in last(lib)
    assert encode(lib, [row(L_KIND, 16, 16, spare=7)]) == ERR_ARG and "spare" in last(lib)
    # a blob smaller than the bound, a workspace that is too small
    assert encode(lib, ok, blob_bytes=M.bound(16, 16, 1) - 1) == ERR_ARG and "blob capacity" in last(lib)
    two[1][7] -= 1
    assert encode(lib, two, blob_bytes=M.bound(16, 16, 1) + M.bound(16, 16, 4) - 1) == ERR_ARG and "blob capacity" in last(lib)
    need = lib.dm4d_png_ws_bytes(16 * 17, 1, 1)
    assert encode(lib, ok, ws_bytes=need - 1) == ERR_ARG and "workspace too small" in last(lib)
