"""CPU: argument validation of dm4d_rectify_u8.  Like every entry point it returns DM4D_ERR_ARG (-1) with a message in dm4d_last_error()
BEFORE anything is launched: the "device" pointers are fake aligned addresses that are never dereferenced, the host copies of the
descriptors and the tables are real.  And the constants in host/lib.py are the header's."""
import re
from pathlib import Path

import numpy as np
import pytest

P = 0x10000
ERR_ARG = -1
STAGING = 1 << 20
OUT = 1 << 20


@pytest.fixture(scope="module")
def lib():
    from diffuman4d_amd.host import lib as L
    return L.load()


def last(lib):
    return lib.dm4d_last_error().decode()


def good_tab():
    """The tables of one 40 x 30 -> 20 x 15 image (scale 2) as host/rectify.py lays them out: horizontal, vertical, camera constants."""
    from diffuman4d_amd.host import rectify
    h, hk = rectify.area_table(40, 20)
    v, vk = rectify.area_table(30, 15)
    assert hk == vk == 2
    return np.concatenate([h, v, np.zeros(16, dtype=np.int32)]), h.size, h.size + v.size


def good_row(htab=0, vtab=80, cam=140):
    #       src  h   w   uh  uw  rh  rw  top left ch cw  htab hk vtab vk cam out
    return [32, 33, 47, 30, 40, 15, 20, 1, 2, 14, 18, htab, 2, vtab, 2, cam, 64]


def call(lib, rows, tab=None, **kw):
    from diffuman4d_amd.host import lib as L
    tab0, vtab, cam = good_tab()
    tab = tab0 if tab is None else tab
    desc = np.zeros((max(len(rows), 1), L.RECTIFY_FIELDS), dtype=np.int64)
    for d, r in zip(desc, rows):
        d[:len(r)] = r
    a = dict(staging=P, staging_bytes=STAGING, desc_host=desc.ctypes.data, desc_dev=2 * P, n=len(rows), tab_host=tab.ctypes.data, tab_dev=3 * P,
             tab_len=tab.size, lut_dev=4 * P, out=5 * P, out_bytes=OUT)
    a.update(kw)
    return lib.dm4d_rectify_u8(None, a["staging"], a["staging_bytes"], a["desc_host"], a["desc_dev"], a["n"], a["tab_host"], a["tab_dev"],
                               a["tab_len"], a["lut_dev"], a["out"], a["out_bytes"])


def changed(**fields):
    names = ["src", "h", "w", "uh", "uw", "rh", "rw", "top", "left", "ch", "cw", "htab", "hk", "vtab", "vk", "cam", "out"]
    row = good_row()
    for k, v in fields.items():
        row[names.index(k)] = v
    return row


def test_the_layout_of_the_good_row_is_the_hosts():
    _, vtab, cam = good_tab()
    assert (vtab, cam) == (80, 140)


def test_rejects_bad_arguments(lib):
    for name in ("staging", "desc_host", "desc_dev", "tab_host", "tab_dev", "lut_dev", "out"):
        assert call(lib, [good_row()], **{name: None}) == ERR_ARG and "null pointer" in last(lib)
    for n in (0, -1, 65536):
        assert call(lib, [good_row()], n=n) == ERR_ARG and "n outside" in last(lib)
    for name in ("staging_bytes", "tab_len", "out_bytes"):
        assert call(lib, [good_row()], **{name: 0}) == ERR_ARG and "empty" in last(lib)
    for name, v in (("staging", P + 8), ("out", 5 * P + 4), ("lut_dev", 4 * P + 8), ("tab_dev", 3 * P + 2), ("desc_dev", 2 * P + 4)):
        assert call(lib, [good_row()], **{name: v}) == ERR_ARG and "aligned" in last(lib)


def test_rejects_bad_descriptors(lib):
    for f in ("h", "w", "uh", "uw", "rh", "rw"):
        for v in (0, -1, 16385):
            assert call(lib, [good_row(), changed(**{f: v})]) == ERR_ARG and "image 1" in last(lib) and "outside 1..16384" in last(lib)
    for off in (8, 33, 47):
        assert call(lib, [changed(src=off)]) == ERR_ARG and "not 16-byte aligned" in last(lib)
        assert call(lib, [changed(out=off)]) == ERR_ARG and "not 16-byte aligned" in last(lib)
    assert call(lib, [changed(src=-16)]) == ERR_ARG and "negative" in last(lib)
    need = 33 * 47 * 3
    assert call(lib, [changed(src=STAGING)]) == ERR_ARG and "outside the staging buffer" in last(lib)
    assert call(lib, [good_row()], staging_bytes=32 + need - 1) == ERR_ARG and "outside the staging buffer" in last(lib)  # one byte short
    assert call(lib, [good_row()], out_bytes=64 + 14 * 18 * 3 - 1) == ERR_ARG and "outside the output buffer" in last(lib)
    for f, v in (("rw", 41), ("rw", 4), ("rh", 31), ("rh", 3)):
        assert call(lib, [changed(**{f: v})]) == ERR_ARG and "scale of an axis is outside 1..8" in last(lib)
    for crop in (dict(top=-1), dict(left=-1), dict(ch=0), dict(cw=0), dict(top=2), dict(left=3), dict(ch=15), dict(cw=19)):
        assert call(lib, [good_row(), changed(**crop)]) == ERR_ARG and "crop is empty or lies outside the resized image" in last(lib)
    for f, v in (("cam", -1), ("cam", 141), ("cam", 1 << 40)):
        assert call(lib, [changed(**{f: v})]) == ERR_ARG and "camera constants" in last(lib)


def test_rejects_bad_tables(lib):
    tab0, vtab, cam = good_tab()
    for f, v in (("htab", -1), ("htab", cam + 1), ("hk", 0), ("hk", 11)):
        assert call(lib, [changed(**{f: v})]) == ERR_ARG and "horizontal table" in last(lib)
    for f, v in (("vtab", -1), ("vtab", 1 << 40), ("vk", 0), ("vk", 11)):
        assert call(lib, [changed(**{f: v})]) == ERR_ARG and "vertical table" in last(lib)
    # windows: one past the undistorted image, a negative start, no taps, more taps than ksize, starts that go back
    for idx, v, which in ((2 * 19, 39, "horizontal"), (0, -1, "horizontal"), (1, 0, "horizontal"), (1, 3, "horizontal"), (2 * 5, 3, "horizontal"),
                          (vtab + 2 * 14, 29, "vertical"), (vtab + 2 * 14 + 1, 3, "vertical")):
        tab = tab0.copy()
        tab[idx] = v
        assert call(lib, [good_row()], tab=tab) == ERR_ARG and f"{which} table" in last(lib) and "tap window" in last(lib)


def test_constants_equal_the_header():
    from diffuman4d_amd.host import lib as L
    header = (Path(__file__).resolve().parent.parent / "include" / "dm4d.h").read_text()
    for name, want in (("RECTIFY_FIELDS", 20), ("RECTIFY_MAX_SIDE", 16384), ("RECTIFY_MAX_SCALE", 8)):
        assert int(re.search(rf"^#define DM4D_{name}[ \t]+(\d+)", header, flags=re.M).group(1)) == getattr(L, name) == want
