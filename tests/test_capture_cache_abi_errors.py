"""CPU: argument validation of dm4d_capture_crop_resize_packed_u8 and dm4d_capture_unpack_cells_f32.  Like every entry point they return
DM4D_ERR_ARG (-1) with a message in dm4d_last_error() BEFORE anything is launched: the "device" pointers are fake aligned addresses
that are never dereferenced, the host copies of descriptors and tables are real.  What the packed entry checks about frames, tables and
scratch is the check of dm4d_capture_crop_resize_f32 (one function in capture.hip): both entries are asked the same questions here and
give the same answers.  And the new constant in host/lib.py is the header's."""
import re
from pathlib import Path

import numpy as np
import pytest

from diffuman4d_amd.host import capture

P = 0x10000
ERR_ARG = -1
H, W = 6, 8
CELL = H * W * 8
SLAB = 0x400000
SLAB_BYTES = 4 * CELL
SRC_H, SRC_W = 12, 20


@pytest.fixture(scope="module")
def lib():
    from diffuman4d_amd.host import lib as L
    return L.load()


def last(lib):
    return lib.dm4d_last_error().decode()


def frames(n=2):
    """A valid staging layout of n frames of 12 x 20 cropped whole and resized to 6 x 8 -> (desc, tab, staging bytes, scratch bytes)."""
    ts = capture.TableSet()
    ts.add(SRC_W, W)
    ts.add(SRC_H, H)
    tab = ts.array()
    (htab, hk), (vtab, vk) = ts.tables[(SRC_W, W)], ts.tables[(SRC_H, H)]
    vb = tab[vtab: vtab + 2 * H].reshape(H, 2)
    y_first, y_last = int(vb[0, 0]), int(vb[-1, 0] + vb[-1, 1])
    rows = y_last - y_first
    desc = np.zeros((n, capture.FIELDS), np.int64)
    plane = SRC_H * SRC_W
    for f in range(n):
        base = f * 7 * plane
        desc[f] = [base, base + 3 * plane, base + 4 * plane, SRC_H, SRC_W, 0, 0, SRC_H, SRC_W, htab, hk, vtab, vk, f * rows * W * 8, y_first, rows]
    return desc, tab, n * 7 * plane, n * rows * W * 8


def cells_of(rows):
    c = np.zeros((max(len(rows), 1), 4), np.int64)
    for d, r in zip(c, rows):
        d[:len(r)] = r
    return c


GOOD_CELLS = [(SLAB, SLAB_BYTES, 0, 0), (SLAB, SLAB_BYTES, CELL, 1)]


def packed(lib, cells=GOOD_CELLS, entry="packed", **kw):
    desc, tab, staging_bytes, scratch_bytes = frames(kw.pop("n_frames_built", 2))
    if "edit" in kw:
        kw.pop("edit")(desc, tab)
    c = cells_of(cells)
    a = dict(staging=P, staging_bytes=staging_bytes, desc_host=desc.ctypes.data, desc_dev=2 * P, n_frames=len(desc), tab_host=tab.ctypes.data,
             tab_dev=3 * P, tab_len=tab.size, scratch=4 * P, scratch_bytes=scratch_bytes, cell_host=c.ctypes.data, cell_dev=5 * P, H=H, W=W)
    a.update(kw)
    head = (None, a["staging"], a["staging_bytes"], a["desc_host"], a["desc_dev"], a["n_frames"], a["tab_host"], a["tab_dev"], a["tab_len"],
            a["scratch"], a["scratch_bytes"])
    if entry == "f32":  # the fused entry: two output pointers where the packed one has its cell descriptors
        return lib.dm4d_capture_crop_resize_f32(*head, 6 * P, 7 * P, a["H"], a["W"])
    return lib.dm4d_capture_crop_resize_packed_u8(*head, a["cell_host"], a["cell_dev"], a["H"], a["W"])


def unpack(lib, cells=GOOD_CELLS, **kw):
    c = cells_of(cells)
    a = dict(cell_host=c.ctypes.data, cell_dev=5 * P, n_rows=len(cells), pix=6 * P, skel=7 * P, n_out_rows=4, H=H, W=W)
    a.update(kw)
    return lib.dm4d_capture_unpack_cells_f32(None, a["cell_host"], a["cell_dev"], a["n_rows"], a["pix"], a["skel"], a["n_out_rows"], a["H"], a["W"])


BAD_CELLS = [  # (the second row of a call whose first is good, a word of the refusal)
    ((0, SLAB_BYTES, CELL, 1), "slab address"),
    ((SLAB + 8, SLAB_BYTES, CELL, 1), "slab address"),
    ((SLAB, SLAB_BYTES, -16, 1), "offset"),
    ((SLAB, SLAB_BYTES, CELL + 8, 1), "offset"),
    ((SLAB, SLAB_BYTES, SLAB_BYTES - CELL + 16, 1), "offset"),  # 16 bytes past the slab's end
    ((SLAB, CELL - 16, 0, 1), "offset"),                        # a slab smaller than one cell
    ((SLAB, -1, 0, 1), "offset"),
]


def test_packed_refuses_bad_cells(lib):
    for name in ("cell_host", "cell_dev", "staging", "desc_host", "desc_dev", "tab_host", "tab_dev", "scratch"):
        assert packed(lib, **{name: None}) == ERR_ARG and "null pointer" in last(lib), name
    assert packed(lib, W=6) == ERR_ARG and "W must be a multiple of 4" in last(lib)
    for kw in ({"H": 0}, {"W": 0}, {"H": 65536}, {"W": (1 << 20) + 4}, {"n_frames": 0}, {"n_frames": 65536}, {"staging_bytes": 0}, {"tab_len": 0},
               {"scratch_bytes": 0}):
        assert packed(lib, **kw) == ERR_ARG and "empty or oversized shape" in last(lib), kw
    assert packed(lib, scratch=4 * P + 8) == ERR_ARG and "16-byte aligned" in last(lib)
    assert packed(lib, cell_dev=5 * P + 4) == ERR_ARG and "cell_dev must be 8-byte aligned" in last(lib)
    for row, word in BAD_CELLS:
        assert packed(lib, [GOOD_CELLS[0], row]) == ERR_ARG and word in last(lib) and "capture_cells" in last(lib), row
    assert packed(lib, [GOOD_CELLS[0], GOOD_CELLS[0]]) == ERR_ARG and "two frames name the same cell" in last(lib)
    assert packed(lib, [GOOD_CELLS[0], (SLAB, 2 * SLAB_BYTES, 0, 7)]) == ERR_ARG and "two frames name the same cell" in last(lib)  # (slab, offset) decides


def edit(field, value, frame=1):
    def f(desc, tab):
        desc[frame, field] = value
    return f


FRAME_CASES = [  # what dm4d_capture_crop_resize_f32 checks about descriptors, tables and scratch
    (edit(3, 0), "bad frame or crop size"), (edit(8, 0), "bad frame or crop size"), (edit(5, (1 << 20) + 1), "bad frame or crop size"),
    (edit(0, -1), "outside the staging buffer"), (edit(1, 1 << 30), "outside the staging buffer"), (edit(2, 1 << 30), "outside the staging buffer"),
    (edit(9, 1 << 30), "coefficient table"), (edit(12, 0), "coefficient table"), (edit(7, SRC_H - 1), "coefficient table"),
    (edit(14, -1), "bad scratch row range"), (edit(15, 0), "bad scratch row range"), (lambda desc, tab: desc[1].__setitem__(15, desc[1, 15] - 1), "vertical window leaves"),
    (edit(13, 8), "scratch region"), (edit(13, 1 << 30), "scratch region"), (edit(13, -16), "scratch region"),
]


def test_packed_shares_the_frame_check_of_the_fused_entry(lib):
    for e, word in FRAME_CASES:
        texts = []
        for entry in ("f32", "packed"):
            assert packed(lib, entry=entry, edit=e) == ERR_ARG
            texts.append(last(lib))
        assert texts[0] == texts[1] and word in texts[0], texts


def test_unpack_refuses_bad_arguments(lib):
    for name in ("cell_host", "cell_dev", "pix", "skel"):
        assert unpack(lib, **{name: None}) == ERR_ARG and "null pointer" in last(lib), name
    assert unpack(lib, W=6) == ERR_ARG and "W must be a multiple of 4" in last(lib)
    for kw in ({"H": 0}, {"W": -4}, {"H": 65536}, {"W": (1 << 20) + 4}, {"n_rows": 0}, {"n_rows": 65536}, {"n_out_rows": 0}, {"n_out_rows": 65536}):
        assert unpack(lib, **kw) == ERR_ARG and "empty or oversized shape" in last(lib), kw
    for kw in ({"pix": 6 * P + 4}, {"skel": 7 * P + 8}, {"cell_dev": 5 * P + 4}):
        assert unpack(lib, **kw) == ERR_ARG and "must be aligned" in last(lib), kw
    for row, word in BAD_CELLS:
        assert unpack(lib, [GOOD_CELLS[0], row]) == ERR_ARG and word in last(lib) and "capture_cells" in last(lib), row
    for r in (-1, 4, 1 << 40):
        assert unpack(lib, [GOOD_CELLS[0], (SLAB, SLAB_BYTES, CELL, r)]) == ERR_ARG and "outside [0, n_out_rows)" in last(lib), r
    assert unpack(lib, [GOOD_CELLS[0], (SLAB, SLAB_BYTES, CELL, 0)]) == ERR_ARG and "two rows name the same output row" in last(lib)
    assert unpack(lib, [(SLAB, SLAB_BYTES, 0, 3), (SLAB, SLAB_BYTES, 0, 2)], n_out_rows=3) == ERR_ARG and "outside [0, n_out_rows)" in last(lib)


def test_the_constant_equals_the_header_and_the_signatures_are_declared():
    from diffuman4d_amd.host import lib as L
    from diffuman4d_amd.host import ops
    header = (Path(__file__).resolve().parent.parent / "include" / "dm4d.h").read_text()
    assert int(re.search(r"^#define DM4D_CAPTURE_CELL_FIELDS[ \t]+(\d+)", header, flags=re.M).group(1)) == L.CAPTURE_CELL_FIELDS == ops.CAPTURE_CELL_FIELDS == 4
    for name in ("dm4d_capture_crop_resize_packed_u8", "dm4d_capture_unpack_cells_f32"):
        assert name in L.SIGNATURES and re.search(rf"^int {name}\(", header, flags=re.M)
    assert len(L.SIGNATURES["dm4d_capture_crop_resize_packed_u8"][1]) == len(L.SIGNATURES["dm4d_capture_crop_resize_f32"][1]) == 15
