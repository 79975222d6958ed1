"""GPU: 8-bit PNG files decoded on the device (csrc/pngdec.hip through diffuman4d_amd/host/pngdec.py) against Pillow's pixels, byte
for byte: the shared case list as one mixed batch, every file alone (batch invariance), two runs (repeatability), a workspace that
chunks the batch, output at offsets of a larger buffer, batches that mix in files of the Pillow route, malformed streams that must
come back with exactly the model's status, and the gray-mask packer of the carving stage."""
import functools
import io

import numpy as np
import pytest
import torch
from PIL import Image

import pngdec_cases as cases
import pngdec_model as model
from diffuman4d_amd.host import lib as L
from diffuman4d_amd.host import ops, pngdec

pytestmark = pytest.mark.gpu


def pillow(data):
    return np.asarray(Image.open(io.BytesIO(data)))


@functools.lru_cache(maxsize=None)
def expected():
    """[(name, file, Pillow's pixels)]"""
    return [(name, data, pillow(data)) for name, data in cases.supported()]


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """The whole list in one call: (tensors as numpy, stats)."""
    stats = {}
    got = pngdec.decode_png_batch([d for _, d, _ in expected()], "cuda", stats=stats)
    return [g.cpu().numpy() for g in got], stats


def test_mixed_batch_equals_pillow_and_no_file_takes_the_pillow_route():
    got, stats = mixed_batch()
    assert stats["pillow"] == 0 and stats["device"] == len(expected())
    assert stats["bytes_uploaded"] == sum(len(cases.idat_stream(d)) for _, d, _ in expected())
    for (name, _, want), g in zip(expected(), got):
        assert g.shape == want.shape and g.dtype == np.uint8, name
        assert np.array_equal(g, want), f"{name}: {int((g != want).sum())} bytes differ"


def test_each_file_alone_and_twice():
    got, _ = mixed_batch()
    for (name, data, _), g in zip(expected(), got):
        stats = {}
        alone = pngdec.decode_png_batch([data], "cuda", stats=stats)[0].cpu().numpy()
        assert stats["pillow"] == 0, name
        assert np.array_equal(alone, g), f"{name}: alone differs from the batch"
    again = pngdec.decode_png_batch([d for _, d, _ in expected()], "cuda")
    for (name, _, _), g, a in zip(expected(), got, again):
        assert np.array_equal(a.cpu().numpy(), g), f"{name}: the second run differs"


def test_small_workspace_chunks_the_batch():
    sub = expected()[70:95]
    got = pngdec.decode_png_batch([d for _, d, _ in sub], "cuda", workspace_bytes=1)  # one file a call
    for (name, _, want), g in zip(sub, got):
        assert np.array_equal(g.cpu().numpy(), want), name
    sub = expected()[:40]
    got = pngdec.decode_png_batch([d for _, d, _ in sub], "cuda", workspace_bytes=40000)  # a few files a call
    for (name, _, want), g in zip(sub, got):
        assert np.array_equal(g.cpu().numpy(), want), name


def test_output_at_offsets_leaves_the_bytes_around_it_untouched():
    sub = [e for e in expected() if e[0].startswith(("65x65x", "129x63x", "1x1x", "63x2x", "300x300-stored", "encoder-RGBA"))]
    assert len(sub) == 14
    plans = [pngdec.probe(d) for _, d, _ in sub]
    offsets, channels, total = [], [], 37  # odd gaps: nothing is aligned
    for p in plans:
        offsets.append(total)
        channels.append(p.channels)
        total += p.h * p.w * p.channels + 29
    buf = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")
    st = pngdec.decode_plans(plans, [d for _, d, _ in sub], buf, offsets, channels)
    assert st == [0] * len(sub)
    host = buf.cpu().numpy()
    covered = np.zeros(total, dtype=bool)
    for (name, _, want), at in zip(sub, offsets):
        assert np.array_equal(host[at:at + want.size].reshape(want.shape), want), name
        covered[at:at + want.size] = True
    assert (host[~covered] == 0xA5).all()


def test_channels_must_be_the_files():
    name, data, _ = expected()[0]
    p = pngdec.probe(data)
    buf = torch.zeros(p.h * p.w * 4, dtype=torch.uint8, device="cuda")
    with pytest.raises(L.Dm4dError, match="output channels"):
        pngdec.decode_plans([p], [data], buf, [0], [3 if p.channels != 3 else 4])


def test_unsupported_files_in_a_batch_return_pillows_pixels():
    readable = []
    for name, data in cases.unsupported():
        try:
            pillow(data)
            readable.append(data)
        except Exception:
            pass
    assert len(readable) >= 5
    files = [cases.supported()[12][1]] + readable + [cases.supported()[40][1]]
    stats = {}
    got = pngdec.decode_png_batch(files, "cuda", stats=stats)
    assert stats["pillow"] == len(readable) and stats["device"] == 2
    for data, g in zip(files, got):
        assert np.array_equal(g.cpu().numpy(), pillow(data))
    unreadable = dict(cases.unsupported())["truncated-file"]
    with pytest.raises(Exception) as dev_err:
        pngdec.decode_png_batch([unreadable], "cuda")  # Pillow cannot read it either
    with pytest.raises(type(dev_err.value)):
        pillow(unreadable)


def test_malformed_files_report_the_models_status_and_take_the_pillow_route():
    bad = cases.malformed()
    plans = [pngdec.probe(d) for _, d, _ in bad]
    assert all(p is not None for p in plans)
    offsets, total = [], 0
    for p in plans:
        offsets.append(total)
        total += p.h * p.w * p.channels
    buf = torch.zeros(total, dtype=torch.uint8, device="cuda")
    st = pngdec.decode_plans(plans, [d for _, d, _ in bad], buf, offsets, [p.channels for p in plans])
    for (name, data, bit), s in zip(bad, st):
        assert s != 0 and s & bit, f"{name}: status {s}"
        assert s == model.decode_status(data)[1], name
    good = cases.supported()[13][1]
    for name, data, _ in bad:
        try:
            want = pillow(data)
        except Exception as e:
            with pytest.raises(type(e)):
                pngdec.decode_png_batch([good, data], "cuda")
            continue
        stats = {}
        got = pngdec.decode_png_batch([data, good], "cuda", stats=stats)
        assert stats == {"device": 1, "pillow": 1, "bytes_uploaded": stats["bytes_uploaded"]}, name
        assert np.array_equal(got[0].cpu().numpy(), want) and np.array_equal(got[1].cpu().numpy(), pillow(good)), name


def test_mutated_streams_agree_with_the_model():
    muts = cases.mutations(60)
    plans = [pngdec.probe(d) for _, d in muts]
    offsets, total = [], 0
    for p in plans:
        offsets.append(total)
        total += p.h * p.w * p.channels
    buf = torch.zeros(total, dtype=torch.uint8, device="cuda")
    st = pngdec.decode_plans(plans, [d for _, d in muts], buf, offsets, [p.channels for p in plans])
    host = buf.cpu().numpy()
    for (name, data), p, at, s in zip(muts, plans, offsets, st):
        px, want = model.decode_status(data)
        assert s == want, name
        if s == 0:
            assert np.array_equal(host[at:at + px.size], px.reshape(-1)), name


def test_a_host_device_is_an_error():
    with pytest.raises(L.Dm4dError, match="HIP device"):
        pngdec.decode_png_batch([cases.supported()[0][1]], "cpu")


def test_pack_masks_u8_equals_the_bool_packer():
    rng = np.random.default_rng(3)
    for w in (1, 31, 32, 33, 65):
        x = rng.integers(0, 256, (3, 5, w), dtype=np.uint8)
        x[0, 0, :min(w, 4)] = [127, 128, 0, 255][:min(w, 4)]
        xd = torch.from_numpy(x).cuda()
        want = ops.vhull_pack_masks(xd >= 128).cpu().numpy()
        assert np.array_equal(ops.vhull_pack_masks_u8(xd, 128).cpu().numpy(), want), w
        assert np.array_equal(ops.vhull_pack_masks_u8(xd, 1).cpu().numpy(), ops.vhull_pack_masks(xd).cpu().numpy()), w
