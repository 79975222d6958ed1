"""CPU: argument validation of dm4d_capture_plane_stats_u8 and dm4d_capture_fill_rects_u8.  Like every entry point they return
DM4D_ERR_ARG (-1) with a message in dm4d_last_error() BEFORE anything is launched: the "device" pointers are fake aligned addresses
that are never dereferenced, the descriptors' host copy is real.  And the constants in host/lib.py are the header's."""
import re
from pathlib import Path

import numpy as np
import pytest

P = 0x10000
ERR_ARG = -1
BLOB = 1 << 20


@pytest.fixture(scope="module")
def lib():
    from diffuman4d_amd.host import lib as L
    return L.load()


def last(lib):
    return lib.dm4d_last_error().decode()


def stats(lib, rows, **kw):
    desc = np.zeros((max(len(rows), 1), 8), dtype=np.int64)
    for d, r in zip(desc, rows):
        d[:len(r)] = r
    a = dict(blob=P, blob_bytes=BLOB, desc_host=desc.ctypes.data, desc_dev=2 * P, n=len(rows), out=3 * P, ws=4 * P, ws_bytes=1 << 30)
    a.update(kw)
    return lib.dm4d_capture_plane_stats_u8(None, a["blob"], a["blob_bytes"], a["desc_host"], a["desc_dev"], a["n"], a["out"], a["ws"], a["ws_bytes"])


def fill(lib, rows, **kw):
    desc = np.zeros((max(len(rows), 1), 8), dtype=np.int64)
    for d, r in zip(desc, rows):
        d[:len(r)] = r
    a = dict(blob=P, blob_bytes=BLOB, desc_host=desc.ctypes.data, desc_dev=2 * P, n=len(rows))
    a.update(kw)
    return lib.dm4d_capture_fill_rects_u8(None, a["blob"], a["blob_bytes"], a["desc_host"], a["desc_dev"], a["n"])


GOOD = (32, 10, 20, 3)


def test_plane_stats_rejects_bad_arguments(lib):
    for name in ("blob", "desc_host", "desc_dev", "out", "ws"):
        assert stats(lib, [GOOD], **{name: None}) == ERR_ARG and "null pointer" in last(lib)
    for n in (0, -1, 65536):
        assert stats(lib, [GOOD], n=n) == ERR_ARG and "n outside" in last(lib)
    assert stats(lib, [GOOD], blob_bytes=0) == ERR_ARG and "empty blob" in last(lib)
    assert stats(lib, [GOOD], blob=P + 8) == ERR_ARG and "aligned" in last(lib)
    assert stats(lib, [GOOD], out=3 * P + 4) == ERR_ARG and "aligned" in last(lib)
    for ch in (0, 2, 4):
        assert stats(lib, [GOOD, (32, 10, 20, ch)]) == ERR_ARG and "channels must be 1 or 3" in last(lib)
    for off in (8, 33, 47):
        assert stats(lib, [(off, 10, 20, 1)]) == ERR_ARG and "not 16-byte aligned" in last(lib)
    for h, w in ((0, 5), (5, 0), (-1, 5), (32769, 1), (1, 32769)):
        assert stats(lib, [(0, h, w, 1)]) == ERR_ARG and "size is outside" in last(lib)
    assert stats(lib, [(-16, 10, 20, 1)]) == ERR_ARG and "outside the blob" in last(lib)
    assert stats(lib, [(BLOB - 16, 1, 17, 1)]) == ERR_ARG and "outside the blob" in last(lib)       # one byte past the end
    assert stats(lib, [(0, 1024, 1024, 3)]) == ERR_ARG and "outside the blob" in last(lib)
    assert stats(lib, [GOOD, (BLOB + 16, 1, 1, 1)]) == ERR_ARG and "outside the blob" in last(lib)  # checked for every row
    assert stats(lib, [GOOD], ws_bytes=39) == ERR_ARG and "workspace" in last(lib)
    assert stats(lib, [(0, 512, 512, 1)], ws_bytes=8 * 40 - 1, blob_bytes=512 * 512) == ERR_ARG and "workspace" in last(lib)


def test_fill_rects_rejects_bad_arguments(lib):
    good = (5, 10, 20, 0, 0, 20, 10)
    for name in ("blob", "desc_host", "desc_dev"):
        assert fill(lib, [good], **{name: None}) == ERR_ARG and "null pointer" in last(lib)
    for n in (0, 65536):
        assert fill(lib, [good], n=n) == ERR_ARG and "n outside" in last(lib)
    assert fill(lib, [(BLOB - 199, 10, 20, 0, 0, 1, 1)]) == ERR_ARG and "outside the blob" in last(lib)
    assert fill(lib, [(-1, 10, 20, 0, 0, 1, 1)]) == ERR_ARG and "outside the blob" in last(lib)
    assert fill(lib, [(0, 0, 20, 0, 0, 0, 0)]) == ERR_ARG and "size is outside" in last(lib)
    for rect in ((0, 0, 21, 10), (0, 0, 20, 11), (-1, 0, 5, 5), (0, -1, 5, 5), (6, 0, 5, 5), (0, 6, 5, 5)):
        assert fill(lib, [good, (5, 10, 20, *rect)]) == ERR_ARG and "rectangle lies outside" in last(lib)


def test_workspace_query(lib):
    q = lib.dm4d_capture_plane_stats_ws_bytes
    assert q(1, 1) == 40 and q(3, 32768) == 120 and q(3, 32769) == 240 and q(2, 1 << 40) == 0 and q(0, 1) == 0 and q(1, 0) == 0
    assert q(1, 2902 * 2902) == 256 * 40  # the block count is capped


def test_constants_equal_the_header():
    from diffuman4d_amd.host import lib as L
    header = (Path(__file__).resolve().parent.parent / "include" / "dm4d.h").read_text()
    for name in ("CAPTURE_PLANE_FIELDS", "CAPTURE_RECT_FIELDS"):
        assert int(re.search(rf"^#define DM4D_{name}[ \t]+(\d+)", header, flags=re.M).group(1)) == getattr(L, name) == 8
