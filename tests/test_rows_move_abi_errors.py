"""CPU: argument validation of dm4d_rows_move and of the row-subset model-input entries.  Like every entry point they return
DM4D_ERR_ARG (-1) with a message in dm4d_last_error() BEFORE anything is launched: the "device" pointers are fake aligned addresses
that are never dereferenced.  And the job structure and its limit in host/lib.py are the header's."""
import ctypes
import re
from pathlib import Path

import pytest

P = 0x10000
ERR_ARG = -1


@pytest.fixture(scope="module")
def lib():
    from diffuman4d_amd.host import lib as L
    return L.load()


def last(lib):
    return lib.dm4d_last_error().decode()


def move(lib, jobs):
    from diffuman4d_amd.host import lib as L
    tab = (L.RowsMoveJob * max(1, len(jobs)))()
    for t, j in zip(tab, jobs):
        t.src, t.dst, t.src_row_idx, t.dst_row_idx, t.n_rows, t.row_bytes = j
    return lib.dm4d_rows_move(None, ctypes.cast(tab, ctypes.c_void_p), len(jobs))


GOOD = (P, 2 * P, 3 * P, 4 * P, 3, 640)


def bad(**kw):
    names = ("src", "dst", "src_row_idx", "dst_row_idx", "n_rows", "row_bytes")
    return tuple(kw.get(n, v) for n, v in zip(names, GOOD))


def test_rows_move_rejects_bad_arguments(lib):
    from diffuman4d_amd.host import lib as L
    assert lib.dm4d_rows_move(None, None, 1) == ERR_ARG and "no jobs" in last(lib)
    assert move(lib, []) == ERR_ARG and "no jobs" in last(lib)
    assert move(lib, [GOOD] * (L.ROWS_MOVE_MAX_JOBS + 1)) == ERR_ARG and "too many jobs" in last(lib)
    for field in ("src", "dst", "src_row_idx", "dst_row_idx"):
        assert move(lib, [GOOD, bad(**{field: None})]) == ERR_ARG and "null pointer" in last(lib)
    for rb in (8, 24, 641):
        assert move(lib, [bad(row_bytes=rb)]) == ERR_ARG and "multiple of 16" in last(lib)
    assert move(lib, [bad(row_bytes=0)]) == ERR_ARG and "empty rows" in last(lib)
    assert move(lib, [bad(n_rows=-1)]) == ERR_ARG and "negative row count" in last(lib)
    assert move(lib, [bad(src=P + 8)]) == ERR_ARG and "16-byte aligned" in last(lib)
    assert move(lib, [bad(dst=2 * P + 4)]) == ERR_ARG and "16-byte aligned" in last(lib)
    assert move(lib, [bad(src_row_idx=3 * P + 2)]) == ERR_ARG and "misaligned index" in last(lib)
    # nothing to move is no error, and launches nothing (the pointers of an empty job are not looked at)
    assert move(lib, [bad(n_rows=0, src=None, dst=None, src_row_idx=None, dst_row_idx=None)]) == 0


def test_pack_rows_rejects_bad_arguments(lib):
    for name in ("dm4d_pack_model_input_rows_bf16", "dm4d_pack_model_input_rows_f32_split", "dm4d_pack_model_input_rows_f32_f16"):
        fn = getattr(lib, name)
        args = lambda **kw: (None, P, P, P, P, P, P, P, kw.get("out_row", P), kw.get("out", P), 4, kw.get("Fo", 2), 16, kw.get("cpad", 32), 1)  # noqa: E731
        assert fn(*args(out_row=None)) == ERR_ARG and "row table" in last(lib)
        assert fn(*args(Fo=0)) == ERR_ARG and "row count" in last(lib)
        assert fn(*args(Fo=5)) == ERR_ARG and "row count" in last(lib)
        assert fn(*args(out=None)) == ERR_ARG and "null pointer" in last(lib)
        assert fn(*args(cpad=8)) == ERR_ARG and "cpad too small" in last(lib)


def test_job_structure_and_limit_equal_the_header():
    from diffuman4d_amd.host import lib as L
    header = (Path(__file__).resolve().parent.parent / "include" / "dm4d.h").read_text()
    assert int(re.search(r"^#define DM4D_ROWS_MOVE_MAX_JOBS[ \t]+(\d+)", header, flags=re.M).group(1)) == L.ROWS_MOVE_MAX_JOBS >= 16
    body = re.search(r"typedef struct \{(.*?)\} Dm4dRowsMoveJob;", header, flags=re.S).group(1)
    fields = [re.sub(r"\W", "", d.split()[-1]) for d in body.split(";") if d.strip()]
    assert fields == [n for n, _ in L.RowsMoveJob._fields_]
    assert ctypes.sizeof(L.RowsMoveJob) == 48
