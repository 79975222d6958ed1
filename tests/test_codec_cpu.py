"""CPU: diffuman4d_amd/host/codec.py, what the image codecs and their consumers share: the chunker, the fallback step around one
``decode_plans`` call, and the routing of ``decode_*_batch`` between the device and Pillow.  No device: the codecs are stubs, the
buffers plain CPU tensors.  Every comparison is for equality."""
import io
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image


# -- the chunker -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("needs, budget, cap, want", [
    ([], 10, None, []),
    ([], 0, 3, []),
    ([5, 5, 5], 1, None, [(0, 1), (1, 2), (2, 3)]),
    ([5, 5, 5], 10, None, [(0, 2), (2, 3)]),
    ([5, 5, 5], 15, None, [(0, 3)]),
    ([20, 1, 1], 10, None, [(0, 1), (1, 3)]),  # an item over the budget stands alone
    ([1] * 7, 100, 3, [(0, 3), (3, 6), (6, 7)]),
])
def test_chunks(needs, budget, cap, want):
    from diffuman4d_amd.host.codec import chunks
    assert chunks(needs, budget, cap) == want
    if cap is None:
        assert chunks(needs, budget) == want


def test_the_decoders_cap_a_chunk_at_the_libraries_limit():
    from diffuman4d_amd.host import codec
    assert codec.MAX_DECODE_CHUNK == 65535
    assert codec.chunks([0] * 65537, 1, codec.MAX_DECODE_CHUNK) == [(0, 65535), (65535, 65537)]


# -- the fallback step -----------------------------------------------------------------------------------------------------------------
class _Spy:
    """A codec whose decode_plans records its arguments and answers `status`."""

    def __init__(self, status):
        self.status, self.calls = status, []

    def decode_plans(self, plans, files, out, offsets, channels):
        self.calls.append((list(plans), list(files), out, list(offsets), list(channels)))
        return list(self.status)


def test_decode_or_fallback_fills_only_the_refused_entry():
    from diffuman4d_amd.host.codec import decode_or_fallback
    spy = _Spy([0, 5, 0])
    buf = torch.full((100,), 0xA5, dtype=torch.uint8)
    entries = [("plan0", b"file0", 3, 1), ("plan1", b"file1", 21, 3), ("plan2", b"file2", 57, 1)]
    pixels = np.arange(24, dtype=np.uint8).reshape(2, 4, 3)[:, ::-1]  # not contiguous
    asked = []

    def fallback(k):
        asked.append(k)
        return pixels
    assert decode_or_fallback(spy, entries, buf, fallback) == [0, 5, 0]
    assert len(spy.calls) == 1
    plans, files, out, offsets, channels = spy.calls[0]
    assert (plans, files, offsets, channels) == (["plan0", "plan1", "plan2"], [b"file0", b"file1", b"file2"], [3, 21, 57], [1, 3, 1])
    assert out is buf
    assert asked == [1]
    want = np.full(100, 0xA5, dtype=np.uint8)
    want[21:45] = pixels.reshape(-1)
    assert np.array_equal(buf.numpy(), want)


def test_decode_or_fallback_raises_what_the_fallback_raises():
    from diffuman4d_amd.host.codec import decode_or_fallback
    buf = torch.full((16,), 0xA5, dtype=torch.uint8)

    def fallback(k):
        raise OSError("cannot identify image file")
    with pytest.raises(OSError, match="cannot identify image file"):
        decode_or_fallback(_Spy([0, 5, 0]), [("p", b"", 0, 1), ("p", b"", 4, 1), ("p", b"", 8, 1)], buf, fallback)
    assert bool((buf == 0xA5).all())
    assert decode_or_fallback(_Spy([0, 0, 0]), [("p", b"", 0, 1), ("p", b"", 4, 1), ("p", b"", 8, 1)], buf, fallback) == [0, 0, 0]


# -- the batch body --------------------------------------------------------------------------------------------------------------------
def _png(a) -> bytes:
    f = io.BytesIO()
    Image.fromarray(a).save(f, "PNG")
    return f.getvalue()


def test_decode_batch_routes_refused_files_to_pillow(monkeypatch):
    """The whole body of decode_*_batch with the device check answered by the host: the second file is refused by probe, the third
    by the decoder."""
    from diffuman4d_amd.host import codec, lib as L
    monkeypatch.setattr(L, "hip_device", lambda device, what: torch.device("cpu"))
    rng = np.random.default_rng(5)
    arrays = [rng.integers(0, 256, (3, 5), dtype=np.uint8), rng.integers(0, 256, (4, 2, 3), dtype=np.uint8),
              rng.integers(0, 256, (2, 3, 3), dtype=np.uint8)]
    datas = [_png(a) for a in arrays]
    plans = {datas[0]: SimpleNamespace(h=3, w=5, bytes_per_pixel=1, payload_len=11),
             datas[2]: SimpleNamespace(h=2, w=3, bytes_per_pixel=3, payload_len=13)}
    calls = []

    def decode_plans(ps, files, out, offsets, channels, workspace_bytes):
        calls.append((ps, files, offsets, channels, workspace_bytes))
        out[0:15] = torch.from_numpy(arrays[0].reshape(-1))  # the first file decodes; the second of the call is flagged
        return [0, 4]
    stub = SimpleNamespace(probe=plans.get, decode_plans=decode_plans)
    stats = {"device": 10, "pillow": 20, "bytes_uploaded": 1000}
    got = codec.decode_batch(stub, "decode_stub_batch", datas, "cuda", 77, stats)
    assert calls == [([plans[datas[0]], plans[datas[2]]], [datas[0], datas[2]], [0, 16], [1, 3], 77)]
    assert stats == {"device": 11, "pillow": 22, "bytes_uploaded": 1000 + 11 + 13 + arrays[1].nbytes + arrays[2].nbytes}
    for g, d, a in zip(got, datas, arrays):
        assert g.dtype == torch.uint8 and np.array_equal(g.numpy(), codec.pillow_pixels(d)) and np.array_equal(g.numpy(), a)
    assert codec.decode_batch(stub, "decode_stub_batch", [], "cuda", 77, None) == [] and len(calls) == 1


def test_both_plans_answer_the_drivers_questions():
    from diffuman4d_amd.host import jpegdec, pngdec
    p = jpegdec.Plan(17, 33, 3, 2, 2, b"", (100, 250))  # 2 x 3 MCUs of 4 + 2 blocks, 128 bytes of coefficients a block
    assert (p.bytes_per_pixel, p.workspace_need, p.payload_len) == (3, 36 * 128, 150)
    p = jpegdec.Plan(17, 33, 1, 1, 1, b"", (0, 7))
    assert (p.bytes_per_pixel, p.workspace_need, p.payload_len) == (1, 3 * 5 * 128, 7)
    p = pngdec.Plan(3, 6, 3, "RGB", ((10, 20), (32, 40)))  # 3 rows of 1 + 18 bytes, to the next multiple of 16
    assert (p.bytes_per_pixel, p.workspace_need, p.payload_len) == (3, 64, 18)


def test_read_file_takes_paths_and_bytes(tmp_path):
    from diffuman4d_amd.host import codec
    (tmp_path / "f.bin").write_bytes(b"\x00\x01\x02")
    assert codec.read_file(tmp_path / "f.bin") == codec.read_file(str(tmp_path / "f.bin")) == b"\x00\x01\x02"
    for data in (b"ab", bytearray(b"ab"), memoryview(b"ab")):
        assert codec.read_file(data) == b"ab" and type(codec.read_file(data)) is bytes


# -- the encoders' inputs --------------------------------------------------------------------------------------------------------------
def _rows(buf, off, stride, h, row):
    """The h rows of `row` bytes, `stride` apart, from byte `off` of a uint8 buffer."""
    return np.stack([buf.numpy()[off + y * stride: off + y * stride + row] for y in range(h)])


@pytest.mark.parametrize("bpp", [1, 3])
def test_gather_reads_views_of_one_storage_in_place(bpp):
    from diffuman4d_amd.host.codec import gather
    shape = (12, 20) if bpp == 1 else (12, 20, 3)
    wide = torch.from_numpy(np.random.default_rng(4).integers(0, 256, shape, dtype=np.uint8))
    views = [wide[2:9, 3:14], wide[0:12, 19:20], wide[5:6, 0:20], wide[11:12, 7:8], wide]
    buf, at = gather(views, bpp)
    assert buf.dtype == torch.uint8 and buf.dim() == 1 and buf.data_ptr() == wide.data_ptr() and buf.numel() == wide.numel()  # no copy
    for v, (off, stride) in zip(views, at):
        h, w = v.shape[:2]
        assert off == v.storage_offset() and stride >= w * bpp and (h == 1 or stride == 20 * bpp)
        assert off + (h - 1) * stride + w * bpp <= buf.numel()
        assert np.array_equal(_rows(buf, off, stride, h, w * bpp), v.numpy().reshape(h, w * bpp))


@pytest.mark.parametrize("bpp", [1, 3])
def test_gather_takes_the_stride_of_a_one_row_view_for_nothing(bpp):
    """The stride of a dimension of size 1 is arbitrary: a [1, w] view that reports a stride below its row is still read in place."""
    from diffuman4d_amd.host.codec import gather
    shape = (6, 10) if bpp == 1 else (6, 10, 3)
    wide = torch.arange(6 * 10 * bpp, dtype=torch.uint8).reshape(shape)
    row = wide[4:5, 2:9]
    odd = row.as_strided(row.shape, (1,) + tuple(row.stride()[1:]), row.storage_offset())  # the same bytes, row stride 1
    assert odd.stride(0) == 1 and torch.equal(odd, row)
    buf, at = gather([odd, wide[1:3, 0:4]], bpp)
    assert buf.data_ptr() == wide.data_ptr()
    assert at == [(row.storage_offset(), 7 * bpp), (10 * bpp, 10 * bpp)]
    assert np.array_equal(_rows(buf, *at[0], 1, 7 * bpp), row.numpy().reshape(1, 7 * bpp))


@pytest.mark.parametrize("bpp", [1, 3])
def test_gather_copies_what_is_not_rows_of_one_storage(bpp):
    from diffuman4d_amd.host.codec import gather
    shape = (12, 20) if bpp == 1 else (12, 20, 3)
    wide = torch.from_numpy(np.random.default_rng(5).integers(0, 256, shape, dtype=np.uint8))
    views = [wide[2:9, 3:14], wide[5:6, 0:20], wide[0:12, 19:20]]
    for tensors in ([v.clone() for v in views],            # different storages
                    [views[0], wide[:, ::2], views[2]]):   # one storage, but pixels that are not contiguous within a row
        buf, at = gather(tensors, bpp)
        assert buf.dtype == torch.uint8 and buf.numel() == sum(t.numel() for t in tensors) and buf.data_ptr() != wide.data_ptr()
        off = 0
        for t, place in zip(tensors, at):
            h, w = t.shape[:2]
            assert place == (off, w * bpp)  # back to back
            assert np.array_equal(_rows(buf, off, w * bpp, h, w * bpp), t.numpy().reshape(h, w * bpp))
            off += t.numel()


def test_require_device_u8_names_the_tensor_and_what_is_wrong():
    from diffuman4d_amd.host import codec
    from diffuman4d_amd.host import lib as L
    with pytest.raises(L.Dm4dError, match=r"^images\[3\]: expected a tensor on a HIP device"):
        codec.require_device_u8(torch.zeros(2, 2, dtype=torch.uint8), "images[3]")
    with pytest.raises(L.Dm4dError, match=r"^mask: expected a tensor on a HIP device"):
        codec.require_device_u8(np.zeros((2, 2), np.uint8), "mask")

    from unittest import mock
    t = mock.Mock(spec=torch.Tensor, device=SimpleNamespace(type="cuda"), dtype=torch.float32)  # what the second check sees
    with pytest.raises(L.Dm4dError, match=r"^planes\[0\]: expected uint8, got torch.float32$"):
        codec.require_device_u8(t, "planes[0]")
    with pytest.raises(L.Dm4dError, match="HIP device"):  # the device is asked about first
        codec.require_device_u8(torch.zeros(2, 2), "planes[0]")
    t.dtype = torch.uint8
    assert codec.require_device_u8(t, "planes[0]") is t
