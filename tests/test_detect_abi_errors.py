"""CPU: argument validation of dm4d_detect_input_u8_f32 and dm4d_detect_select_f32.  Like every entry point they return DM4D_ERR_ARG
(-1) with a message in dm4d_last_error() BEFORE anything is launched: the "device" pointers are fake aligned addresses that are never
dereferenced, the host copies of the descriptors and the tables are real."""
import ctypes

import numpy as np
import pytest

P = 0x10000
ERR_ARG = -1
STAGING = 1 << 20
SIZE = (37, 50)  # h, w
SHAPE = (64, 64)


@pytest.fixture(scope="module")
def lib():
    from diffuman4d_amd.host import lib as L
    return L.load()


def last(lib):
    return lib.dm4d_last_error().decode()


def good_tab():
    from diffuman4d_amd.host import detect
    (tab,), nwnh, _ = detect.detector_tables([SIZE], SHAPE)
    return tab.copy(), int(nwnh[0, 0]), int(nwnh[0, 1])


def good_row(toff=0):
    #       image mask  h   w   table
    return [32, 5600, 37, 50, toff]


def call_input(lib, rows, tab=None, **kw):
    from diffuman4d_amd.host import lib as L
    tab = good_tab()[0] if tab is None else tab
    desc = np.zeros((max(len(rows), 1), L.POSE_FIELDS), dtype=np.int64)
    for d, r in zip(desc, rows):
        d[:len(r)] = r
    norm = np.array(kw.pop("norm", [100, 110, 120, 50, 55, 60]), dtype=np.float32)
    a = dict(staging=P, staging_bytes=STAGING, desc_host=desc.ctypes.data, desc_dev=2 * P, n=len(rows), tab_host=tab.ctypes.data, tab_dev=3 * P,
             tab_len=tab.size, norm_host=norm.ctypes.data, out=5 * P, H=SHAPE[0], W=SHAPE[1], pad_value=114, bgr=0)
    a.update(kw)
    return lib.dm4d_detect_input_u8_f32(None, a["staging"], a["staging_bytes"], a["desc_host"], a["desc_dev"], a["n"], a["tab_host"], a["tab_dev"],
                                        a["tab_len"], a["norm_host"], a["out"], a["H"], a["W"], a["pad_value"], a["bgr"])


def changed(**fields):
    names = ["image", "mask", "h", "w", "table", "spare5", "spare6", "spare7"]
    row = good_row() + [0, 0, 0]
    for k, v in fields.items():
        row[names.index(k)] = v
    return row


def test_input_rejects_bad_arguments(lib):
    for name in ("staging", "desc_host", "desc_dev", "tab_host", "tab_dev", "norm_host", "out"):
        assert call_input(lib, [good_row()], **{name: None}) == ERR_ARG and "null pointer" in last(lib)
    for n in (0, -1, 65536):
        assert call_input(lib, [good_row()], n=n) == ERR_ARG and "n outside" in last(lib)
    for name in ("H", "W"):
        for v in (0, -1, 4097):
            assert call_input(lib, [good_row()], **{name: v}) == ERR_ARG and "canvas size" in last(lib)
    for v in (-1, 256):
        assert call_input(lib, [good_row()], pad_value=v) == ERR_ARG and "pad_value" in last(lib)
    for name in ("staging_bytes", "tab_len"):
        assert call_input(lib, [good_row()], **{name: 0}) == ERR_ARG and "empty" in last(lib)
    for name, v in (("out", 5 * P + 2), ("tab_dev", 3 * P + 2), ("desc_dev", 2 * P + 4)):
        assert call_input(lib, [good_row()], **{name: v}) == ERR_ARG and "aligned" in last(lib)
    for norm in ([100, 110, np.nan, 50, 55, 60], [100, 110, 120, 50, 0, 60], [100, 110, 120, 50, 55, np.inf]):
        assert call_input(lib, [good_row()], norm=norm) == ERR_ARG and "mean must be finite" in last(lib)


def test_input_rejects_bad_descriptors(lib):
    for f in ("h", "w"):
        for v in (0, -1, 16385):
            assert call_input(lib, [good_row(), changed(**{f: v})]) == ERR_ARG and "row 1" in last(lib) and "outside 1..16384" in last(lib)
    for off in (8, 33, 47):  # a misaligned plane offset
        assert call_input(lib, [changed(image=off)]) == ERR_ARG and "not 16-byte aligned" in last(lib)
        assert call_input(lib, [changed(mask=off)]) == ERR_ARG and "not 16-byte aligned" in last(lib)
    need = 37 * 50 * 3
    for off in (-16, STAGING + 16, STAGING - need + 16):  # out of range
        assert call_input(lib, [changed(image=off)]) == ERR_ARG and "image outside the staging buffer" in last(lib)
    assert call_input(lib, [good_row()], staging_bytes=32 + need - 1) == ERR_ARG and "image outside the staging buffer" in last(lib)
    assert call_input(lib, [changed(mask=-2)]) == ERR_ARG and "mask offset is negative" in last(lib)
    assert call_input(lib, [changed(mask=STAGING - 37 * 50 + 16)]) == ERR_ARG and "mask outside the staging buffer" in last(lib)
    assert call_input(lib, [changed(spare6=1)]) == ERR_ARG and "spare fields" in last(lib)


def test_input_rejects_bad_tables(lib):
    tab0, nw, nh = good_tab()
    assert (nw, nh) == (64, 47)
    for toff in (-1, tab0.size - 1, tab0.size, 1 << 40):  # the table, or its tail, outside tab
        assert call_input(lib, [changed(table=toff)]) == ERR_ARG and "lies outside tab" in last(lib)
    assert call_input(lib, [good_row()], tab_len=tab0.size - 1) == ERR_ARG and "lies outside tab" in last(lib)
    # a canvas smaller than nw x nh; sizes that are empty
    assert call_input(lib, [good_row()], W=63) == ERR_ARG and "larger than the canvas" in last(lib)
    assert call_input(lib, [good_row()], H=46) == ERR_ARG and "larger than the canvas" in last(lib)
    for idx, v in ((0, 0), (1, 0), (0, -3), (1, 65)):
        tab = tab0.copy()
        tab[idx] = v
        assert call_input(lib, [good_row()], tab=tab) == ERR_ARG and "larger than the canvas" in last(lib)
    # a tap window outside its image: one past the last column / row, a negative one
    for idx, v in ((2 + nw - 1, 50), (2, -1), (2 + nw + nh - 1, 37), (2 + nw, -1)):
        tab = tab0.copy()
        tab[idx] = v
        assert call_input(lib, [good_row()], tab=tab) == ERR_ARG and "tap window lies outside its image" in last(lib)
    # weights outside 0..2048
    for idx, v in ((2 + nw + nh, 2049), (2 + nw + nh + 3, -1), (2 + 2 * nw + nh, 2049 << 16), (2 + 2 * nw + 2 * nh - 1, -1 << 16)):
        tab = tab0.copy()
        tab[idx] = v
        assert call_input(lib, [good_row()], tab=tab) == ERR_ARG and "resize weight" in last(lib)


def call_select(lib, **kw):
    a = dict(boxes=P, scores=2 * P, inv=3 * P, n=2, A=100, C=3, cat=0, score_thr=0.3, nms_thr=0.3, max_per_img=100, counts=4 * P, out=5 * P, idx=6 * P)
    a.update(kw)
    return lib.dm4d_detect_select_f32(None, a["boxes"], a["scores"], a["inv"], a["n"], a["A"], a["C"], a["cat"], ctypes.c_float(a["score_thr"]),
                                      ctypes.c_float(a["nms_thr"]), a["max_per_img"], a["counts"], a["out"], a["idx"])


def test_select_rejects_bad_arguments(lib):
    from diffuman4d_amd.host import lib as L
    assert (L.DETECT_MAX_ANCHORS, L.DETECT_MAX_KEEP) == (1 << 20, 256) and L.DETECT_MAX_ANCHORS >= 1 << 17
    for name in ("boxes", "scores", "inv", "counts", "out", "idx"):
        assert call_select(lib, **{name: None}) == ERR_ARG and "null pointer" in last(lib)
    for n in (0, -1, 65536):
        assert call_select(lib, n=n) == ERR_ARG and "n outside" in last(lib)
    for A in (0, -1, (1 << 20) + 1):
        assert call_select(lib, A=A) == ERR_ARG and "A outside" in last(lib)
    for C in (0, -1, 4097):
        assert call_select(lib, C=C) == ERR_ARG and "C outside" in last(lib)
    for cat in (-1, 3, 100):
        assert call_select(lib, cat=cat) == ERR_ARG and "cat outside" in last(lib)
    for k in (0, -1, 257):
        assert call_select(lib, max_per_img=k) == ERR_ARG and "max_per_img outside" in last(lib)
    for name in ("score_thr", "nms_thr"):
        for v in (float("nan"), float("inf"), float("-inf")):
            assert call_select(lib, **{name: v}) == ERR_ARG and "must be finite" in last(lib)
    for name, v in (("boxes", P + 8), ("scores", 2 * P + 2), ("inv", 3 * P + 1), ("counts", 4 * P + 2), ("out", 5 * P + 2), ("idx", 6 * P + 3)):
        assert call_select(lib, **{name: v}) == ERR_ARG and "aligned" in last(lib)
