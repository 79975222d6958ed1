"""GPU: the nerfstudio export end to end with ``matting_model=lambda x: x[:, :1]``, through the Pillow route and through the device PNG
route: every ``fmasks/*.png`` and ``images_alpha/*.png`` decodes to the same mode, size and pixels in both, the device route's files
are the model's bytes (tests/png_model.py) for those inputs, and a source image whose stored mode is not RGB (a greyscale JPEG) takes
the ``putalpha`` fallback for its RGBA file and still matches.  A palette-mode source goes the same way, and there both routes end in
the same error: ``putalpha`` makes it mode PA, which Pillow cannot write as PNG."""
import shutil
from pathlib import Path

import numpy as np
import pytest
from PIL import Image

import png_model as M
from diffuman4d_amd.host import nerfstudio

pytestmark = pytest.mark.gpu
SCENE = Path(__file__).resolve().parent / "golden" / "capture_scene" / "ring8"
SIZES = {"00/000000": (40, 24), "00/000001": (33, 47), "03/000000": (64, 64), "03/000001": (17, 16)}


@pytest.fixture(scope="module")
def exports(tmp_path_factory):
    root = tmp_path_factory.mktemp("nerfstudio")
    data = root / "data"
    data.mkdir()
    shutil.copy(SCENE / "transforms.json", data / "transforms.json")
    (data / "sparse_pcd.ply").write_bytes(b"ply\nformat ascii 1.0\nelement vertex 0\nend_header\n")
    rng = np.random.default_rng(21)
    out = {}
    for route in ("host", "device"):
        res = root / route
        for k, (name, (h, w)) in enumerate(SIZES.items()):
            y, x = np.mgrid[0:h, 0:w]
            img = np.stack([(x * 255 // max(w - 1, 1)), (y * 255 // max(h - 1, 1)), np.full((h, w), 40 * k)], axis=-1).astype(np.uint8)
            path = res / "images" / f"{name}.jpg"
            path.parent.mkdir(parents=True, exist_ok=True)
            if route == "host":
                Image.fromarray(img).save(path, quality=90)
            else:
                shutil.copy(root / "host" / "images" / f"{name}.jpg", path)
        grey = res / "images" / "06" / "000000.jpg"
        grey.parent.mkdir(parents=True, exist_ok=True)
        if route == "host":
            Image.fromarray(rng.integers(0, 256, (19, 23), dtype=np.uint8)).save(grey, quality=90)  # a greyscale JPEG: stored mode L
        else:
            shutil.copy(root / "host" / "images" / "06" / "000000.jpg", grey)
        counts = nerfstudio.diffuman4d_to_nerfstudio(str(data), str(res), ["00", "03"], matting_model=lambda x: x[:, :1],
                                                     device_png=route == "device", gpu_ids=[0])
        assert counts == {"images": 5, "written": 5, "skipped": 0}
        out[route] = res
    return out


def names(res, sub):
    return sorted(str(p.relative_to(res / sub)) for p in (res / sub).rglob("*.png"))


def test_both_routes_decode_to_the_same_pixels(exports):
    host, dev = exports["host"], exports["device"]
    for sub in ("fmasks", "images_alpha"):
        assert names(host, sub) == names(dev, sub) == sorted(f"{n}.png" for n in list(SIZES) + ["06/000000"])
        for n in names(host, sub):
            a, b = Image.open(host / sub / n), Image.open(dev / sub / n)
            a.load(), b.load()
            assert a.mode == b.mode and a.size == b.size and np.array_equal(np.asarray(a), np.asarray(b)), (sub, n)
    assert Image.open(dev / "images_alpha" / "06" / "000000.png").mode == "LA"  # the fallback's putalpha on the greyscale image
    for res in (host, dev):
        assert (res / "transforms.json").exists() and (res / "transforms_input.json").exists() and (res / "sparse_pcd.ply").exists()
        assert not list(res.rglob("*.tmp*"))


def test_device_route_files_are_the_models_bytes(exports):
    host, dev = exports["host"], exports["device"]
    for n in list(SIZES) + ["06/000000"]:
        mask = np.asarray(Image.open(host / "fmasks" / f"{n}.png"))
        assert mask.ndim == 2 and (dev / "fmasks" / f"{n}.png").read_bytes() == M.encode(mask), n
    for n, (h, w) in SIZES.items():
        src = Image.open(dev / "images" / f"{n}.jpg")
        assert src.mode == "RGB" and src.size == (w, h)
        mask = np.asarray(Image.open(host / "fmasks" / f"{n}.png"))
        assert (dev / "images_alpha" / f"{n}.png").read_bytes() == M.encode(np.dstack([np.asarray(src), mask])), n
        assert (host / "images_alpha" / f"{n}.png").read_bytes() != (dev / "images_alpha" / f"{n}.png").read_bytes()  # Pillow's own deflate


def test_a_palette_source_ends_the_same_way_in_both_routes(tmp_path):
    """A palette image under the results' extension (Pillow opens by content): its stored mode is P, so the device route leaves its
    RGBA file to ``putalpha`` as well -- which makes it mode PA, and Pillow refuses to write that as PNG, in either route."""
    from diffuman4d_amd.host import matting
    pal = tmp_path / "images" / "00" / "000000.jpg"
    pal.parent.mkdir(parents=True)
    Image.fromarray(np.random.default_rng(4).integers(0, 256, (21, 30), dtype=np.uint8)).convert("P").save(pal, format="PNG")
    masks = {}
    for device_png in (False, True):
        out = tmp_path / str(device_png)
        with pytest.raises(OSError, match="cannot write mode PA as PNG"):
            matting.remove_background(str(tmp_path / "images"), str(out / "fmasks"), str(out / "images_alpha"), image_ext=".jpg",
                                      matting_model=lambda x: x[:, :1], device_png=device_png, gpu_ids=[0])
        masks[device_png] = Image.open(out / "fmasks" / "00" / "000000.png")
        assert not (out / "images_alpha" / "00" / "000000.png").exists()
    assert np.array_equal(np.asarray(masks[False]), np.asarray(masks[True]))
    assert (tmp_path / "True" / "fmasks" / "00" / "000000.png").read_bytes() == M.encode(np.asarray(masks[False]))
