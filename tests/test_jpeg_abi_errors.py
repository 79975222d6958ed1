"""CPU: argument validation of dm4d_jpeg_encode_rgb_u8, dm4d_restore_crop_u8 and their size queries.  Like every entry point they
return DM4D_ERR_ARG (-1) with a message in dm4d_last_error() BEFORE anything is launched: the "device" pointers are fake aligned
addresses that are never dereferenced, the descriptor / table host copies are real."""
import ctypes

import numpy as np
import pytest

P = 0x10000
ERR_ARG = -1
MCU_BOUND, MCU_UNSTUFFED, CHUNK = 2488, 1248, 4096


@pytest.fixture(scope="module")
def lib():
    from diffuman4d_amd.host import lib as L
    return L.load()


def last(lib):
    return lib.dm4d_last_error().decode()


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def encode(lib, desc, qtab=None, pixels_bytes=1 << 20, canvases=None, canvases_bytes=0, ws_bytes=1 << 30, blob_bytes=1 << 30):
    desc = np.ascontiguousarray(desc, dtype=np.int64)
    qtab = np.ones(128, dtype=np.uint16) if qtab is None else qtab
    return lib.dm4d_jpeg_encode_rgb_u8(None, P, pixels_bytes, canvases, canvases_bytes, ptr(desc), P, len(desc), ptr(qtab), P, P, ws_bytes, P, blob_bytes, P)


def test_size_queries(lib):
    assert lib.dm4d_jpeg_scan_bound(1, 1) == MCU_BOUND
    assert lib.dm4d_jpeg_scan_bound(320, 576) == 20 * 36 * MCU_BOUND
    assert lib.dm4d_jpeg_scan_bound(17, 33) == 2 * 3 * MCU_BOUND
    for h, w in [(0, 8), (8, 0), (65536, 8), (8, 65536), (-1, 8), (65535, 65535)]:  # the last: more bits than 32-bit positions hold
        assert lib.dm4d_jpeg_scan_bound(h, w) == 0
    assert lib.dm4d_jpeg_ws_bytes(0, 1) == 0 and lib.dm4d_jpeg_ws_bytes(1, 0) == 0 and lib.dm4d_jpeg_ws_bytes(1, 65536) == 0
    one = lib.dm4d_jpeg_ws_bytes(1, 1)
    assert one >= 768 + 8 + MCU_UNSTUFFED + 4 + 8 and one % 16 == 0
    assert lib.dm4d_jpeg_ws_bytes(720, 1) > 720 * (768 + 8 + MCU_UNSTUFFED)


def test_encode_rejects_bad_descriptors(lib):
    ok = [[0, 0, 16, 16, 0, 0, 0, 0]]
    assert encode(lib, ok, ws_bytes=16) == ERR_ARG and "workspace too small" in last(lib)
    assert encode(lib, ok, blob_bytes=MCU_BOUND - 1) == ERR_ARG and "blob capacity" in last(lib)
    for h, w in [(0, 16), (16, 0), (65536, 16), (16, 65536)]:
        assert encode(lib, [[0, 0, h, w, 0, 0, 0, 0]]) == ERR_ARG and "1..65535" in last(lib)
    assert encode(lib, [[0, 0, 65535, 65535, 0, 0, 0, 0]], pixels_bytes=1 << 40) == ERR_ARG and "32-bit" in last(lib)
    assert encode(lib, [[2, 0, 16, 16, 0, 0, 0, 0]]) == ERR_ARG and "neither" in last(lib)
    assert encode(lib, [[1, 0, 16, 16, 0, 0, 0, 0]]) == ERR_ARG and "outside its buffer" in last(lib)  # no canvases given
    assert encode(lib, [[0, 1, 16, 16, 0, 0, 0, 0]], pixels_bytes=768) == ERR_ARG and "outside its buffer" in last(lib)
    assert encode(lib, [[0, -1, 16, 16, 0, 0, 0, 0]]) == ERR_ARG and "outside its buffer" in last(lib)
    assert encode(lib, [[0, 0, 16, 16, 1, 0, 0, 0]]) == ERR_ARG and "running sum" in last(lib)
    two = [[0, 0, 16, 32, 0, 0, 0, 0], [0, 1536, 16, 16, 2, 0, 0, 0]]  # the second image's first chunk must be 1
    assert encode(lib, two) == ERR_ARG and "running sum" in last(lib)
    two[1][5] = (2 * MCU_UNSTUFFED + CHUNK - 1) // CHUNK
    two[1][4] = 1
    assert encode(lib, two) == ERR_ARG and "running sum" in last(lib)
    assert encode(lib, [[0, 0, 16, 16, 0, 0, 0, 7]]) == ERR_ARG
    q = np.ones(128, dtype=np.uint16)
    q[77] = 0
    assert encode(lib, ok, qtab=q) == ERR_ARG and "quantisation" in last(lib)
    q[77] = 256
    assert encode(lib, ok, qtab=q) == ERR_ARG and "quantisation" in last(lib)
    desc = np.zeros((1, 8), dtype=np.int64)
    assert lib.dm4d_jpeg_encode_rgb_u8(None, P, 1, None, 0, ptr(desc), P, 0, ptr(q), P, P, 1, P, 1, P) == ERR_ARG and "batch" in last(lib)
    assert lib.dm4d_jpeg_encode_rgb_u8(None, P, 1, None, 0, None, P, 1, ptr(q), P, P, 1, P, 1, P) == ERR_ARG and "null" in last(lib)
    assert lib.dm4d_jpeg_encode_rgb_u8(None, P, 1 << 20, None, 0, ptr(np.asarray(ok, dtype=np.int64)), P, 1, ptr(np.ones(128, dtype=np.uint16)), P, P + 4,
                                       1 << 30, P, 1 << 30, P) == ERR_ARG and "aligned" in last(lib)


def restore(lib, desc, tab, pixels_bytes=1 << 20, scratch_bytes=1 << 20, canvases_bytes=1 << 20):
    desc = np.ascontiguousarray(desc, dtype=np.int64)
    tab = np.ascontiguousarray(tab, dtype=np.int32)
    return lib.dm4d_restore_crop_u8(None, P, pixels_bytes, ptr(desc), P, len(desc), ptr(tab), P, len(tab), P, scratch_bytes, P, canvases_bytes)


def test_restore_rejects_bad_descriptors(lib):
    from diffuman4d_amd.host.capture import bicubic_table
    hb, hk = bicubic_table(8, 12)   # W 8 -> cw 12
    vb, vk = bicubic_table(6, 9)    # H 6 -> ch 9
    tab = np.concatenate([hb.reshape(-1), hk.reshape(-1), vb.reshape(-1), vk.reshape(-1)])
    vtab = hb.size + hk.size
    #       src H  W  ct cl ch cw  h   w   htab hk          vtab  vk          scratch dst spare
    good = [0, 6, 8, -2, 3, 9, 12, 10, 14, 0, hk.shape[1], vtab, vk.shape[1], 0, 0, 0]

    def bad(**kw):
        d = list(good)
        for k, v in kw.items():
            d[int(k[1:])] = v
        return [d]
    assert restore(lib, bad(f1=0), tab) == ERR_ARG and "1..65535" in last(lib)
    assert restore(lib, bad(f8=65536), tab) == ERR_ARG and "1..65535" in last(lib)
    assert restore(lib, bad(f3=1 << 21), tab) == ERR_ARG and "crop offset" in last(lib)
    assert restore(lib, [good], tab, pixels_bytes=6 * 8 * 3 - 1) == ERR_ARG and "source image" in last(lib)
    assert restore(lib, bad(f6=13), tab) == ERR_ARG and "coefficient table" in last(lib)      # 13 windows asked of a 12-window table region
    assert restore(lib, bad(f2=7), tab, pixels_bytes=1 << 20) == ERR_ARG and "coefficient table" in last(lib)  # windows leave a 7-wide image
    assert restore(lib, bad(f11=len(tab)), tab) == ERR_ARG and "coefficient table" in last(lib)
    assert restore(lib, [good], tab, scratch_bytes=6 * 12 * 3 - 1) == ERR_ARG and "scratch" in last(lib)
    assert restore(lib, [good], tab, canvases_bytes=10 * 14 * 3 - 1) == ERR_ARG and "canvas" in last(lib)
    second = list(good)
    second[14] = 10 * 14 * 3 - 1  # overlaps the first canvas
    assert restore(lib, [good, second], tab) == ERR_ARG and "overlaps" in last(lib)
    assert lib.dm4d_restore_crop_u8(None, None, 1, None, P, 1, None, P, 1, P, 1, P, 1) == ERR_ARG and "null" in last(lib)
