"""GPU: the two stages that can take their JPEG files through the device decoder write exactly what they write without it.
``remove_background(device_decode=True)`` (a stand-in network, with and without ``device_png``) and
``evaluate_results(device_decode=True)`` over a handful of 40 x 72 pairs with JPEG predictions."""
import json

import numpy as np
import pytest
from PIL import Image

import jpegdec_cases as cases
from diffuman4d_amd.host import jpegdec, matting, metrics

pytestmark = pytest.mark.gpu


def _tree(root):
    return {str(p.relative_to(root)): p.read_bytes() for p in sorted(root.rglob("*")) if p.is_file()}


@pytest.fixture(scope="module")
def jpeg_dir(tmp_path_factory):
    """images/{camera}/{frame}.jpg: colour files of three samplings and odd sizes, a grayscale file, a progressive file (Pillow's
    route in both runs) and a file whose scan the decoder refuses by status."""
    root = tmp_path_factory.mktemp("jpegdec_wiring") / "images"
    files = [cases.save(cases.content("smooth", 37, 53, 1), "420", 90, False), cases.save(cases.content("noise", 40, 72, 2), "422", 90, True),
             cases.save(cases.content("smooth", 17, 33, 3), "444", 100, False), cases.save(cases.content("smooth", 24, 31, 4), "gray", 90, False),
             dict(cases.unsupported())["progressive"], dict(cases.malformed())["flipped"]]
    for k, data in enumerate(files):
        path = root / f"{k % 2:02d}" / f"{k // 2:06d}.jpg"
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_bytes(data)
    return root


@pytest.mark.parametrize("device_png", [False, True])
def test_remove_background_writes_the_same_files(jpeg_dir, tmp_path, device_png):
    seen = []
    real = jpegdec.decode_plans

    def spy(plans, *a, **kw):
        st = real(plans, *a, **kw)
        seen.append(st)
        return st
    out = {}
    for device_decode in (False, True):
        dst = tmp_path / str(device_decode)
        jpegdec.decode_plans = spy
        try:
            res = matting.remove_background(str(jpeg_dir), str(dst / "fmasks"), str(dst / "images_alpha"), image_ext=".jpg", batch_size=4,
                                            matting_model=lambda x: x[:, :1], image_size=(64, 48), device_png=device_png, gpu_ids=[0],
                                            device_decode=device_decode)
        finally:
            jpegdec.decode_plans = real
        assert res["written"] == 6
        if not device_decode:
            assert seen == []
        out[device_decode] = _tree(dst)
    assert len(out[False]) == 12 and out[True] == out[False]
    # the device decoded five files in two batches, and refused exactly the flipped one
    assert sorted(s for st in seen for s in st).count(0) == 4 and sum(len(st) for st in seen) == 5


def test_evaluate_results_writes_the_same_metrics(tmp_path):
    rng = np.random.default_rng(0)
    for cam in ("00", "01"):
        for frame in range(3):
            gt = cases.content("smooth", 40, 72, 10 * frame + int(cam))
            pred = np.clip(gt.astype(np.int16) + rng.integers(-12, 13, gt.shape), 0, 255).astype(np.uint8)
            mask = np.zeros((40, 72), dtype=np.uint8)
            mask[4:36, 10:60] = 255
            for sub, a, ext, kw in (("pred", pred, ".jpg", dict(quality=90)), ("gt", gt, ".jpg", dict(quality=95, subsampling=0)),
                                    ("fmasks", mask, ".png", {})):
                path = tmp_path / sub / cam / f"{frame:06d}{ext}"
                path.parent.mkdir(parents=True, exist_ok=True)
                Image.fromarray(a).save(path, **kw)
    texts = {}
    for device_decode in (False, True):
        out = tmp_path / f"metrics_{device_decode}.json"
        res = metrics.evaluate_results(str(tmp_path / "pred"), str(tmp_path / "gt"), str(tmp_path / "fmasks"), ".jpg", ".jpg", ".png",
                                       out_metrics_path=str(out), background_color="white", gpu_ids=[0], canvas_size=72, batch_size=4,
                                       device_decode=device_decode)
        assert len(res["values"]) == 6
        texts[device_decode] = out.read_text()
    assert texts[True] == texts[False] and json.loads(texts[True])["mean"]["psnr"] > 10


def test_evaluator_keeps_its_checks(tmp_path):
    """A grayscale prediction raises the mode error from the file's header, a size mismatch the reference's shape error."""
    gray, rgb, other = tmp_path / "g.jpg", tmp_path / "c.jpg", tmp_path / "o.jpg"
    gray.write_bytes(cases.save(cases.content("smooth", 40, 72, 1), "gray", 90, False))
    rgb.write_bytes(cases.save(cases.content("smooth", 40, 72, 1), "420", 90, False))
    other.write_bytes(cases.save(cases.content("smooth", 40, 64, 1), "420", 90, False))
    for device_decode in (False, True):
        ev = metrics.ImageEvaluator("cuda", device_decode=device_decode)
        with pytest.raises(ValueError, match="image mode 'L', expected 'RGB'"):
            ev(str(gray), str(rgb), crop_with_fmask=False)
        with pytest.raises(ValueError, match="same shape"):
            ev(str(other), str(rgb), crop_with_fmask=False)
        assert ev(str(rgb), str(rgb), crop_with_fmask=False, canvas_size=72)[1] == pytest.approx(1.0)
    with pytest.raises(metrics.Dm4dError, match="HIP device"):
        metrics.ImageEvaluator("cpu", device_decode=True)
