"""CPU: the definition the device JPEG route is held to.  The numpy model (tests/jpeg_model.py) equals Pillow byte for byte, the
header builder equals the header of Pillow's file, the numpy crop-restore model equals ``imgwrite.restore_cropped_image``, and the
host-side wiring of ``device_jpeg`` (write_package's "jpegs" key, the image_ext check) behaves as documented."""
import io
import os

import numpy as np
import pytest
from PIL import Image

import jpeg_model
from diffuman4d_amd.host import imgwrite, jpeg

SHAPES = [(1, 1), (8, 24), (24, 8), (17, 33), (37, 53), (40, 72), (64, 48), (16, 16), (48, 64)]  # (h, w)
QUALITIES = [30, 75, 90, 100]


def pillow_bytes(a, quality):
    f = io.BytesIO()
    Image.fromarray(a).save(f, "JPEG", quality=quality)
    return f.getvalue()


def contents(h, w, seed):
    y, x = np.mgrid[0:h, 0:w]
    grad = np.stack([(3 * y + 2 * x) % 256, 255 - (5 * x + y) % 256, (x * y) % 256], axis=-1).astype(np.uint8)
    checker = np.repeat((((x + y) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)
    return {"noise": np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8), "gradient": grad,
            "white": np.full((h, w, 3), 255, dtype=np.uint8), "checkerboard": checker}


@pytest.mark.parametrize("quality", QUALITIES)
def test_model_equals_pillow(quality):
    for k, (h, w) in enumerate(SHAPES):
        for name, a in contents(h, w, k).items():
            assert jpeg_model.encode(a, quality) == pillow_bytes(a, quality), f"{name} {h}x{w} q{quality}"


@pytest.mark.parametrize("quality", [1, 30, 49, 50, 75, 90, 100])
def test_header_equals_pillows(quality):
    for h, w in [(1, 1), (37, 53), (320, 576), (2048, 2448)]:
        head = jpeg.jpeg_header(h, w, quality)
        ref = pillow_bytes(np.zeros((h, w, 3), dtype=np.uint8), quality)
        assert ref[:len(head)] == head, f"{h}x{w} q{quality}"
        assert head[-14:-12] == b"\xff\xda" and ref[-2:] == b"\xff\xd9"


def test_quality_and_size_are_checked():
    for q in (0, 101, -1, 2.5, True):
        with pytest.raises(ValueError):
            jpeg.quant_tables(q)
    for h, w in [(0, 1), (1, 0), (65536, 1), (1, 65536)]:
        with pytest.raises(ValueError):
            jpeg.jpeg_header(h, w, 90)
    assert jpeg.quant_tables(100) == ((1,) * 64, (1,) * 64)
    assert max(jpeg.quant_tables(1)[0]) == 255  # force_baseline


def test_counters_see_the_rare_paths():
    c = {}
    y, x = np.mgrid[0:48, 0:64]
    jpeg_model.encode(np.repeat((((x + y) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2), 100, c)
    assert c["stuffed"] == 228 and c["max_ac_category"] == 10 and c["zrl"] == 0  # every odd-odd coefficient is set: no long runs
    c = {}
    a = np.full((16, 16, 3), 128, dtype=np.uint8)
    a[::2, ::2] = 160  # a weak pattern at q30: few coefficients survive, far apart in the scan
    jpeg_model.encode(np.tile(a, (2, 2, 1)), 30, c)
    zrl_weak = c["zrl"]
    c = {}
    jpeg_model.encode(np.random.default_rng(0).integers(120, 136, (32, 32, 3), dtype=np.uint8), 90, c)
    assert zrl_weak + c["zrl"] >= 1
    c = {}
    jpeg_model.encode(np.repeat(((((x >> 3) + (y >> 3)) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2), 100, c)
    assert c["max_dc_category"] == 11
    c = {}
    jpeg_model.encode(np.zeros((37, 53, 3), dtype=np.uint8), 90, c)
    assert c["dummy_cols"] == 1 and c["dummy_rows"] == 1 and c["dummy_blocks"] == 2 * 3 + 2 * 4 - 1  # 3 x 4 MCUs over 5 x 7 blocks


CROPS = [(-5, 7, 50, 30), (3, -4, 20, 16), (10, 12, 90, 80), (-20, -30, 100, 120), (3, -4, 20, 16, 40, 44), (10, 12, 90, 80, 64, 48),
         (2, 3, 40, 24), (0, 0, 13, 24), (5, 5, 7, 9, 30, 20), (100, 100, 8, 8), None]


def test_restore_model_equals_restore_cropped_image():
    """Negative ct / cl, larger than the frame, 6-tuples, cw equal to the image width, up- and down-scaling, fully outside."""
    a = np.random.default_rng(1).integers(0, 256, (40, 24, 3), dtype=np.uint8)
    for crop in CROPS:
        want = np.asarray(imgwrite.restore_cropped_image(Image.fromarray(a), crop))
        got = jpeg_model.restore(a, crop)
        assert got.shape == want.shape and np.array_equal(got, want), f"crop {crop}"
        if crop is not None:
            assert jpeg.canvas_size(40, 24, crop) == want.shape[:2]
    with pytest.raises(ValueError):
        jpeg_model.restore(a, (1, 2, 3))


def test_write_package_writes_jpegs_verbatim(tmp_path):
    one, two, three = b"\xff\xd8one\xff\xd9", b"\xff\xd8two\xff\xd9", b"not even a jpeg"
    paths = [str(tmp_path / "images" / "00" / "000000.jpg"), str(tmp_path / "images" / "01" / "000000.jpg"),
             str(tmp_path / "images" / "01" / "000001.jpg")]
    os.makedirs(os.path.dirname(paths[1]))
    with open(paths[1], "wb") as f:
        f.write(b"already here")
    pkg = {"grid": None, "jpegs": list(zip(paths, (one, two, three))), "crops": [], "quality": 90}
    assert imgwrite.write_package(pkg) == 2
    assert open(paths[0], "rb").read() == one and open(paths[1], "rb").read() == b"already here" and open(paths[2], "rb").read() == three
    assert imgwrite.write_package(pkg) == 0  # everything exists now
    # the existing keys are untouched by the new one
    arr = np.random.default_rng(2).integers(0, 256, (8, 8, 3), dtype=np.uint8)
    both = {"grid": None, "images": [(str(tmp_path / "a.jpg"), arr, None)], "jpegs": [(str(tmp_path / "b.jpg"), one)], "crops": [], "quality": 90}
    assert imgwrite.write_package(both) == 2
    assert open(tmp_path / "a.jpg", "rb").read() == pillow_bytes(arr, 90)


def test_device_jpeg_refuses_other_extensions():
    import torch
    from diffuman4d_amd.host import results
    with pytest.raises(ValueError, match="image_ext"):
        results.pack_results_on_device({}, torch.zeros(1, 3, 8, 8), image_ext=".png", device_jpeg=True)


def test_sampler_device_jpeg_needs_device_results():
    from diffuman4d_amd.host.sampler import SlidingIterativeSampler
    with pytest.raises(ValueError, match="device_results"):
        SlidingIterativeSampler(None, [], device_jpeg=True)


def test_a_host_tensor_raises():
    import torch
    from diffuman4d_amd.host import lib as L
    with pytest.raises(L.Dm4dError, match="HIP device"):
        jpeg.encode_jpeg_batch([torch.zeros(8, 8, 3, dtype=torch.uint8)])
