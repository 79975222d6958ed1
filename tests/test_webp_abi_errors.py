"""CPU: argument validation of dm4d_webp_encode_u8 and its size queries.  Like every entry point it returns DM4D_ERR_ARG (-1) with a
message in dm4d_last_error() BEFORE anything is launched: the "device" pointers are fake aligned addresses that are never dereferenced,
the descriptor host copy is real.  Also: the symbols are declared in the header, the constants mirrored, the source in the build."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import webp_model as M

P = 0x10000
ERR_ARG = -1
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def lib():
    from diffuman4d_amd.host import lib as L
    return L.load()


def last(lib):
    return lib.dm4d_last_error().decode()


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def row(h, w, pix=0, stride=None, pix0=0, stripe0=0, spare=0):
    return [h, w, pix, 3 * w if stride is None else stride, pix0, stripe0, 0, spare]


def encode(lib, desc, rgb=P, rgb_bytes=1 << 20, ws=P, ws_bytes=1 << 30, blob=P, blob_bytes=1 << 30, out=P, desc_dev=P, n=None):
    desc = np.ascontiguousarray(desc, dtype=np.int64)
    return lib.dm4d_webp_encode_u8(None, rgb, rgb_bytes, ptr(desc), desc_dev, len(desc) if n is None else n, ws, ws_bytes, blob, blob_bytes, out)


def test_declared_mirrored_and_built():
    from diffuman4d_amd import build
    from diffuman4d_amd.host import lib as L
    header = (ROOT / "include" / "dm4d.h").read_text()
    for name in ("dm4d_webp_bound", "dm4d_webp_ws_bytes", "dm4d_webp_encode_u8"):
        assert re.search(rf"\b{name}\(", header) and name in L.SIGNATURES
    for name in ("FIELDS", "MAX_SIDE", "STRIPE_PIXELS", "STRIPE_REC", "IMAGE_REC"):
        m = re.search(rf"^#define DM4D_WEBP_{name} (\d+)$", header, re.M)
        assert m and int(m.group(1)) == getattr(L, f"WEBP_{name}")
    assert L.WEBP_STRIPE_PIXELS == M.STRIPE_PIXELS and L.WEBP_MAX_SIDE == M.MAX_SIDE == 16383
    assert "webp.hip" in build.SOURCES and (build.CSRC / "webp.hip").exists()


def test_size_queries(lib):
    from diffuman4d_amd.host import lib as L
    for h, w in [(1, 1), (17, 19), (1024, 1024), (16383, 16383)]:
        assert lib.dm4d_webp_bound(h, w) == M.bound(h, w) > 0
    for h, w in [(0, 8), (8, 0), (16384, 8), (8, 16384), (-1, 8)]:
        assert lib.dm4d_webp_bound(h, w) == 0
    assert lib.dm4d_webp_ws_bytes(0, 1, 1) == 0 and lib.dm4d_webp_ws_bytes(2, 0, 1) == 0 and lib.dm4d_webp_ws_bytes(2, 1, 0) == 0
    assert lib.dm4d_webp_ws_bytes(2, 1, 65536) == 0 and lib.dm4d_webp_ws_bytes(100, 1, 2) == 0 and lib.dm4d_webp_ws_bytes(1, 2, 1) == 0
    one = lib.dm4d_webp_ws_bytes(1, 1, 1)
    assert one >= 2 + L.WEBP_STRIPE_REC + L.WEBP_IMAGE_REC + 16 + 16 and one % 16 == 0
    assert lib.dm4d_webp_ws_bytes(1 << 20, 128, 3) >= 2 * (1 << 20) + 128 * L.WEBP_STRIPE_REC + 3 * L.WEBP_IMAGE_REC


def test_encode_rejects_bad_arguments(lib):
    ok = [row(16, 16)]
    for kw in (dict(rgb=None), dict(ws=None), dict(blob=None), dict(out=None), dict(desc_dev=None)):
        assert encode(lib, ok, **kw) == ERR_ARG and "null" in last(lib)
    assert lib.dm4d_webp_encode_u8(None, P, 1 << 20, None, P, 1, P, 1 << 30, P, 1 << 30, P) == ERR_ARG and "null" in last(lib)
    assert encode(lib, ok, n=0) == ERR_ARG and "batch" in last(lib)
    assert encode(lib, ok, n=65536) == ERR_ARG and "batch" in last(lib)
    assert encode(lib, ok, ws=P + 4) == ERR_ARG and "aligned" in last(lib)
    assert encode(lib, ok, out=P + 4) == ERR_ARG and "aligned" in last(lib)
    assert encode(lib, ok, rgb_bytes=0) == ERR_ARG and "not positive" in last(lib)
    # a side of 0 or above 16383
    for h, w in [(0, 16), (16, 0), (M.MAX_SIDE + 1, 16), (16, M.MAX_SIDE + 1), (-1, 16)]:
        assert encode(lib, [row(h, w)], rgb_bytes=1 << 40) == ERR_ARG and "dimension" in last(lib)
    # a stride below 3 w
    assert encode(lib, [row(16, 16, stride=47)]) == ERR_ARG and "stride" in last(lib)
    assert encode(lib, [row(16, 16, stride=0)]) == ERR_ARG and "stride" in last(lib)
    assert encode(lib, [row(16, 16, stride=(1 << 32) + 1)], rgb_bytes=1 << 40) == ERR_ARG and "stride" in last(lib)
    # a region outside the buffer
    assert encode(lib, ok, rgb_bytes=16 * 48 - 1) == ERR_ARG and "outside its buffer" in last(lib)
    assert encode(lib, [row(16, 16, pix=1)], rgb_bytes=16 * 48) == ERR_ARG and "outside its buffer" in last(lib)
    assert encode(lib, [row(16, 16, pix=-1)]) == ERR_ARG and "outside its buffer" in last(lib)
    assert encode(lib, [row(16, 16, pix=(1 << 20) + 1)]) == ERR_ARG and "outside its buffer" in last(lib)
    assert encode(lib, [row(16, 16, stride=60)], rgb_bytes=15 * 60 + 47) == ERR_ARG and "outside its buffer" in last(lib)
    # running sums and spare fields
    assert encode(lib, [row(16, 16, pix0=1)]) == ERR_ARG and "running sum" in last(lib)
    assert encode(lib, [row(16, 16, stripe0=1)]) == ERR_ARG and "running sum" in last(lib)
    two = [row(16, 16), row(100, 100, pix=768, pix0=256, stripe0=2)]
    assert encode(lib, two) == ERR_ARG and "running sum" in last(lib)
    two[1][5], two[1][4] = 1, 257
    assert encode(lib, two) == ERR_ARG and "running sum" in last(lib)
    assert encode(lib, [row(16, 16, spare=7)]) == ERR_ARG and "spare" in last(lib)
    # a blob smaller than the bound, a workspace that is too small
    two[1][4] = 256
    assert encode(lib, ok, blob_bytes=M.bound(16, 16) - 1) == ERR_ARG and "blob capacity" in last(lib)
    assert encode(lib, two, blob_bytes=M.bound(16, 16) + M.bound(100, 100) - 1) == ERR_ARG and "blob capacity" in last(lib)
    need = lib.dm4d_webp_ws_bytes(256, 1, 1)
    assert encode(lib, ok, ws_bytes=need - 1) == ERR_ARG and "workspace too small" in last(lib)
    need = lib.dm4d_webp_ws_bytes(256 + 10000, 3, 2)
    assert encode(lib, two, ws_bytes=need - 1) == ERR_ARG and "workspace too small" in last(lib)
