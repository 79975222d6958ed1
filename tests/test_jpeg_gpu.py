"""GPU: result JPEGs encoded on the device (csrc/jpeg.hip through diffuman4d_amd/host/jpeg.py) against Pillow's files AND the numpy
model's (tests/jpeg_model.py), byte for byte: mixed-size batches, every image alone (batch invariance), two runs (repeatability), the
crop restore, and the packaged route ``pack_results_on_device(device_jpeg=True)`` -> ``write_package`` against the existing one."""
import functools
import io

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_model
from diffuman4d_amd.host import imgwrite, jpeg, results
from diffuman4d_amd.host import lib as L

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (8, 24), (24, 8), (17, 33), (37, 53), (40, 72), (64, 48), (16, 16)]  # (h, w)


def _noise(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _smooth_plus_noise(h, w):
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 100 * np.sin(x / 37.0) * np.cos(y / 53.0), 128 + 90 * np.cos((x + y) / 71.0), 255.0 * y / h], axis=-1)
    return np.clip(base + np.random.default_rng(5).normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def cases(quality):
    """[(name, uint8 [h, w, 3])] of one batch (one quality per call of the encoder)."""
    out = [(f"noise_{h}x{w}", _noise(100 + k, h, w)) for k, (h, w) in enumerate(SIZES)]
    out.append(("white_17x33", np.full((17, 33, 3), 255, dtype=np.uint8)))
    if quality == 100:
        y, x = np.mgrid[0:48, 0:64]
        out.append(("pixel_checkerboard_48x64", np.repeat((((x + y) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)))
        out.append(("block_checkerboard_48x64", np.repeat(((((x >> 3) + (y >> 3)) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)))
    else:
        out.append(("smooth_plus_noise_320x576", _smooth_plus_noise(320, 576)))
        out.append(("noise_16x16400", _noise(200, 16, 16400)))  # 1025 MCUs: the scan of their bit lengths takes a second round of 1024
    for _, a in out:
        a.setflags(write=False)
    return tuple(out)


def pillow_bytes(a, quality):
    f = io.BytesIO()
    Image.fromarray(np.asarray(a)).save(f, "JPEG", quality=quality)
    return f.getvalue()


@functools.lru_cache(maxsize=None)
def expected(quality):
    """Pillow's files, the model's files and the model's counters of a batch; computed once."""
    counters = {}
    pil = tuple(pillow_bytes(a, quality) for _, a in cases(quality))
    model = tuple(jpeg_model.encode(a, quality, counters) for _, a in cases(quality))
    return pil, model, counters


@functools.lru_cache(maxsize=None)
def device_batch(quality):
    dev = torch.device("cuda:0")
    return tuple(jpeg.encode_jpeg_batch([torch.from_numpy(a.copy()).to(dev) for _, a in cases(quality)], quality=quality))


def first_difference(a, b):
    n = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    return f"lengths {len(a)} / {len(b)}, first difference at byte {n}"


def test_the_set_exercises_what_it_claims():
    """The model's counters over both batches (a failure here is a bug of the test's inputs, not of the encoder)."""
    c100, c90 = expected(100)[2], expected(90)[2]
    assert c100["zrl"] + c90["zrl"] >= 1 and c100["stuffed"] >= 1
    assert c100["max_ac_category"] == 10  # the pixel checkerboard
    assert c100["max_dc_category"] == 11
    assert c100["dummy_cols"] >= 1 and c100["dummy_rows"] >= 1 and c100["dummy_blocks"] >= 1
    assert c90["dummy_blocks"] >= 1
    assert any(h % 16 == 8 for h, _ in SIZES)
    assert (37, 53) in SIZES  # dummy blocks in both directions: 7 x 5 luma blocks


@pytest.mark.parametrize("quality", [100, 90])
def test_mixed_batch_equals_pillow_and_model(hip_device, quality):
    pil, model, _ = expected(quality)
    got = device_batch(quality)
    assert len(got) == len(pil)
    for (name, _), g, p, m in zip(cases(quality), got, pil, model):
        assert m == p, f"{name} q{quality}: model != Pillow ({first_difference(m, p)})"
        assert g == p, f"{name} q{quality}: device != Pillow ({first_difference(g, p)})"


@pytest.mark.parametrize("quality", [100, 90])
def test_batch_invariance_and_repeatability(hip_device, quality):
    got = device_batch(quality)
    imgs = [torch.from_numpy(a.copy()).to(hip_device) for _, a in cases(quality)]
    again = jpeg.encode_jpeg_batch(imgs, quality=quality)
    assert list(again) == list(got), "two runs of the same batch differ"
    for (name, _), img, g in zip(cases(quality), imgs, got):
        alone = jpeg.encode_jpeg_batch([img], quality=quality)
        assert alone[0] == g, f"{name} q{quality}: alone != in the batch ({first_difference(alone[0], g)})"


def test_chunked_batch_equals_one_chunk(hip_device):
    """A workspace budget that forces several chunks (one image each at the smallest budget) changes no byte."""
    imgs = [torch.from_numpy(a.copy()).to(hip_device) for _, a in cases(90)]
    assert list(jpeg.encode_jpeg_batch(imgs, quality=90, workspace_bytes=1)) == list(device_batch(90))


def test_a_batch_longer_than_one_scan_round(hip_device):
    """1025 images: the one-block scan of the files' lengths (their places in the blob) carries over from its first 1024 to the last."""
    batch = np.random.default_rng(300).integers(0, 256, (1025, 8, 8, 3), dtype=np.uint8)
    got = jpeg.encode_jpeg_batch(list(torch.from_numpy(batch).to(hip_device)), quality=90)
    assert len(got) == 1025
    for k, g in enumerate(got):
        p = pillow_bytes(batch[k], 90)
        assert g == p, f"image {k} of 1025: device != Pillow ({first_difference(g, p)})"


CROPS = [(-5, 7, 50, 30),              # clipped at a negative row offset, up-scaled
         (3, -4, 20, 16, 40, 44),      # negative column offset, down-scaled, 6-tuple canvas
         (10, 12, 90, 80, 64, 48),     # larger than the frame
         (2, 3, 33, 24)]               # cw equal to the image width


def test_restore_and_encode_equals_the_host_route(hip_device):
    srcs = [_noise(7, 40, 24), _smooth_plus_noise(48, 40), _noise(9, 37, 53), _noise(10, 33, 24)]
    want = []
    for a, crop in zip(srcs, CROPS):
        f = io.BytesIO()
        imgwrite.restore_cropped_image(Image.fromarray(a), crop).save(f, "JPEG", quality=90)
        want.append(f.getvalue())
        canvas = jpeg_model.restore(a, crop)
        assert np.array_equal(canvas, np.asarray(imgwrite.restore_cropped_image(Image.fromarray(a), crop)))
    got = jpeg.encode_jpeg_batch([torch.from_numpy(a).to(hip_device) for a in srcs], quality=90, crops=CROPS)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"crop {CROPS[k]}: device != restore_cropped_image + save ({first_difference(g, w)})"
    # a batch that mixes restored and in-place images
    mixed = jpeg.encode_jpeg_batch([torch.from_numpy(a).to(hip_device) for a in srcs], quality=90, crops=[CROPS[0], None, CROPS[2], None])
    assert mixed[0] == want[0] and mixed[2] == want[2]
    assert mixed[1] == pillow_bytes(srcs[1], 90) and mixed[3] == pillow_bytes(srcs[3], 90)


def _sample(n, h, w, crops):
    g = torch.Generator().manual_seed(3)
    return {"input_indices": torch.tensor([0, 2]), "target_indices": torch.tensor([1, 3, 4][: n - 2]),
            "pixel_values": torch.rand(n, 3, h, w, generator=g) * 2 - 1, "skeletons": None, "domain": "spatial", "alt": 0,
            "domain_label": "000000", "labels": [(k, f"{k:02d}", "000000") for k in range(n)], "crops": crops,
            "fully_denoised": torch.tensor([True] * (n - 1) + [False])}


def test_packaged_route_writes_the_files_of_the_existing_route(hip_device, tmp_path):
    n, h, w = 5, 40, 24
    crops = [None, (-3, 2, 50, 30), (4, -6, 30, 40, 56, 36), (0, 0, 40, 24), (1, 1, 8, 8)]
    sample = _sample(n, h, w, crops)
    images = torch.rand(n, 3, h, w, generator=torch.Generator().manual_seed(4)).to(hip_device)
    a_dir, b_dir = tmp_path / "host", tmp_path / "device"
    pkg_a = results.pack_results_on_device(sample, images, output_dir=str(a_dir), device=hip_device)
    pkg_b = results.pack_results_on_device(sample, images, output_dir=str(b_dir), device=hip_device, device_jpeg=True)
    assert "images" in pkg_a and "jpegs" not in pkg_a
    assert "jpegs" in pkg_b and "images" not in pkg_b
    assert np.array_equal(pkg_a["grid"][1], pkg_b["grid"][1])
    assert imgwrite.write_package(pkg_a) == imgwrite.write_package(pkg_b) == n - 1  # the last target row is still noisy
    files_a = sorted(p.relative_to(a_dir) for p in a_dir.rglob("*.jpg"))
    files_b = sorted(p.relative_to(b_dir) for p in b_dir.rglob("*.jpg"))
    assert files_a == files_b and len(files_a) == n - 1
    for rel in files_a:
        assert (a_dir / rel).read_bytes() == (b_dir / rel).read_bytes(), f"{rel}: the two routes wrote different bytes"


def test_host_tensors_and_bad_arguments_raise(hip_device):
    a = torch.zeros(8, 8, 3, dtype=torch.uint8)
    with pytest.raises(L.Dm4dError, match="HIP device"):
        jpeg.encode_jpeg_batch([a])
    with pytest.raises(ValueError):
        jpeg.encode_jpeg_batch([a.to(hip_device)], quality=0)
    with pytest.raises(ValueError):
        jpeg.encode_jpeg_batch([a.to(hip_device)], quality=101)
    with pytest.raises(L.Dm4dError):
        jpeg.encode_jpeg_batch([a.to(hip_device).float()])
