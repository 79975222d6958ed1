"""GPU: baseline JPEG files decoded on the device (csrc/jpegdec.hip through diffuman4d_amd/host/jpegdec.py) against Pillow's pixels AND
the numpy model's (tests/jpegdec_model.py), byte for byte: the shared case list as one mixed batch, every file alone (batch
invariance), two runs (repeatability), output at offsets of a larger buffer, batches that mix in files of the Pillow route, and
malformed scans that must come back with a nonzero status."""
import functools
import io

import numpy as np
import pytest
import torch
from PIL import Image

import jpegdec_cases as cases
import jpegdec_model as model
from diffuman4d_amd.host import jpegdec
from diffuman4d_amd.host import lib as L

pytestmark = pytest.mark.gpu


def pillow(data):
    return np.asarray(Image.open(io.BytesIO(data)))


@functools.lru_cache(maxsize=None)
def expected():
    """[(name, file, Pillow's pixels)]; the model's pixels are checked against them here, once."""
    out = []
    for name, data in cases.supported():
        want = pillow(data)
        assert np.array_equal(model.decode(data), want), name
        out.append((name, data, want))
    return out


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """The whole list in one call: (tensors as numpy, stats)."""
    stats = {}
    got = jpegdec.decode_jpeg_batch([d for _, d, _ in expected()], "cuda", stats=stats)
    return [g.cpu().numpy() for g in got], stats


def test_mixed_batch_equals_pillow_and_no_file_takes_the_pillow_route():
    got, stats = mixed_batch()
    assert stats["pillow"] == 0 and stats["device"] == len(expected())
    for (name, _, want), g in zip(expected(), got):
        assert g.shape == want.shape and g.dtype == np.uint8, name
        assert np.array_equal(g, want), f"{name}: {int((g != want).sum())} bytes differ"


def test_each_file_alone_and_twice():
    got, _ = mixed_batch()
    for (name, data, _), g in zip(expected(), got):
        stats = {}
        alone = jpegdec.decode_jpeg_batch([data], "cuda", stats=stats)[0].cpu().numpy()
        assert stats["pillow"] == 0, name
        assert np.array_equal(alone, g), f"{name}: alone differs from the batch"
    again = jpegdec.decode_jpeg_batch([d for _, d, _ in expected()], "cuda")
    for (name, _, _), g, a in zip(expected(), got, again):
        assert np.array_equal(a.cpu().numpy(), g), f"{name}: the second run differs"


def test_small_workspace_chunks_the_batch():
    sub = expected()[8:20]
    got = jpegdec.decode_jpeg_batch([d for _, d, _ in sub], "cuda", workspace_bytes=1)  # one file a call
    for (name, _, want), g in zip(sub, got):
        assert np.array_equal(g.cpu().numpy(), want), name


def test_output_at_offsets_leaves_the_bytes_around_it_untouched():
    sub = [e for e in expected() if e[0].startswith(("37x53", "7x5", "40x72-gray", "2x70"))]
    plans = [jpegdec.probe(d) for _, d, _ in sub]
    offsets, channels, total = [], [], 37  # odd gaps: nothing is aligned
    for p in plans:
        offsets.append(total)
        channels.append(3)  # grayscale replicated, as convert("RGB") does
        total += p.h * p.w * 3 + 29
    buf = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")
    st = jpegdec.decode_plans(plans, [d for _, d, _ in sub], buf, offsets, channels)
    assert st == [0] * len(sub)
    host = buf.cpu().numpy()
    covered = np.zeros(total, dtype=bool)
    for (name, data, _), p, at in zip(sub, plans, offsets):
        want = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        assert np.array_equal(host[at:at + want.size].reshape(want.shape), want), name
        covered[at:at + want.size] = True
    assert (host[~covered] == 0xA5).all()


def test_unsupported_files_in_a_batch_return_pillows_pixels():
    files = [cases.supported()[12][1]] + [d for _, d in cases.unsupported()] + [cases.supported()[40][1]]
    stats = {}
    got = jpegdec.decode_jpeg_batch(files, "cuda", stats=stats)
    assert stats["pillow"] == len(cases.unsupported()) and stats["device"] == 2
    for data, g in zip(files, got):
        assert np.array_equal(g.cpu().numpy(), pillow(data))


def test_malformed_scans_report_a_status_and_take_the_pillow_route():
    bad = cases.malformed()
    plans = [jpegdec.probe(d) for _, d in bad]
    assert all(p is not None for p in plans)
    offsets, total = [], 0
    for p in plans:
        offsets.append(total)
        total += p.h * p.w * 3
    buf = torch.zeros(total, dtype=torch.uint8, device="cuda")
    st = jpegdec.decode_plans(plans, [d for _, d in bad], buf, offsets, [3] * len(bad))
    for (name, data), s in zip(bad, st):
        assert s != 0, name
        assert s == model.decode_status(data)[1], name
    assert st[0] & L.JPEGDEC_ST_END and st[1] & L.JPEGDEC_ST_BAD_CODE and st[2] & L.JPEGDEC_ST_RANGE
    stats = {}
    good = cases.supported()[13][1]
    got = jpegdec.decode_jpeg_batch([d for _, d in bad] + [good], "cuda", stats=stats)
    assert stats["pillow"] == len(bad)
    for data, g in zip([d for _, d in bad] + [good], got):
        assert np.array_equal(g.cpu().numpy(), pillow(data))
    with pytest.raises(Exception) as dev_err:
        jpegdec.decode_jpeg_batch([good[:200]], "cuda")  # Pillow cannot read it either
    with pytest.raises(type(dev_err.value)):
        pillow(good[:200])


def test_a_host_device_is_an_error():
    with pytest.raises(L.Dm4dError, match="HIP device"):
        jpegdec.decode_jpeg_batch([cases.supported()[0][1]], "cpu")
