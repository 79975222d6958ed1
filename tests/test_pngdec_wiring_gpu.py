"""GPU: the two stages that can take their PNG files through the device decoder write exactly what they write without it:
``carve_scene(device_decode=True)`` on a tiny synthetic scene (4 views of 65 x 97 masks, 2 frames, one mask stored as mode ``1`` so
it takes the Pillow route) and ``evaluate_results(device_decode=True)`` with PNG masks and PNG predictions."""
import json

import numpy as np
import pytest
from PIL import Image

from diffuman4d_amd.host import metrics, pngdec, vhull

pytestmark = pytest.mark.gpu

H, W, FOCAL, DIST = 65, 97, 100.0, 3.0


def _tree(root):
    return {str(p.relative_to(root)): p.read_bytes() for p in sorted(root.rglob("*")) if p.is_file()}


def _camera(angle: float) -> list:
    """camera-to-world of an OpenGL camera (x right, y up, z backwards) on a circle around the origin, looking at it"""
    pos = np.array([DIST * np.cos(angle), DIST * np.sin(angle), 0.4])
    z = pos / np.linalg.norm(pos)
    x = np.cross([0.0, 0.0, 1.0], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, y, z, pos
    return m.tolist()


def _mask(radius: float) -> np.ndarray:
    """a disc around the principal point with a soft edge: values on both sides of the threshold 128"""
    y, x = np.mgrid[0:H, 0:W]
    r = np.hypot(x - W / 2, y - H / 2)
    return np.clip((radius - r) * 40.0 + 128.0, 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    root = tmp_path_factory.mktemp("pngdec_wiring")
    frames = []
    for cam in range(4):
        frames.append({"camera_label": f"{cam:02d}", "fl_x": FOCAL, "fl_y": FOCAL, "cx": W / 2, "cy": H / 2, "w": W, "h": H,
                       "transform_matrix": _camera(0.3 + 1.5 * cam)})
        for frame in range(2):
            path = root / "fmasks" / f"{cam:02d}" / f"{frame:06d}.png"
            path.parent.mkdir(parents=True, exist_ok=True)
            m = _mask(14.0 + 3 * frame + cam)
            if (cam, frame) == (3, 0):
                Image.fromarray(m >= 128).save(path)  # mode "1": not of the device's set
                assert Image.open(path).mode == "1" and pngdec.probe(path.read_bytes()) is None
            else:
                Image.fromarray(m).save(path)
                assert pngdec.probe(path.read_bytes()) is not None
    (root / "transforms.json").write_text(json.dumps({"frames": frames}))
    return root


KW = dict(bounds=(-1.0, 1.0, -1.0, 1.0, -1.0, 1.0), voxel_size=0.05)


def test_carve_scene_writes_the_same_files(scene, tmp_path):
    seen = []
    real = pngdec.decode_plans

    def spy(plans, *a, **kw):
        st = real(plans, *a, **kw)
        seen.append(st)
        return st
    out = {}
    for device_decode in (False, True):
        dst = tmp_path / str(device_decode)
        pngdec.decode_plans = spy
        try:
            res = vhull.carve_scene(str(scene / "fmasks"), str(scene / "transforms.json"), str(dst / "surfs"),
                                    sparse_pcd_path=str(dst / "sparse_pcd.ply"), device_decode=device_decode, **KW)
        finally:
            pngdec.decode_plans = real
        if not device_decode:
            assert seen == []
        assert set(res["frames"]) == {"000000", "000001"} and min(res["frames"].values()) > 50
        out[device_decode] = _tree(dst)
    assert sorted(out[False]) == ["sparse_pcd.ply", "surfs/000000.ply", "surfs/000001.ply", "surfs_bounds.json"]
    assert out[True] == out[False]
    assert seen == [[0, 0, 0], [0, 0, 0, 0]]  # one call a frame; the mode-1 file never reached the decoder


def test_carve_scene_keeps_its_mode_error(scene, tmp_path):
    bad = tmp_path / "fmasks"
    for src in sorted((scene / "fmasks").rglob("*.png")):
        dst = bad / src.relative_to(scene / "fmasks")
        dst.parent.mkdir(parents=True, exist_ok=True)
        dst.write_bytes(src.read_bytes())
    Image.fromarray(np.zeros((H, W, 3), dtype=np.uint8)).save(bad / "01" / "000000.png")
    texts = []
    for device_decode in (False, True):
        with pytest.raises(ValueError) as e:
            vhull.carve_scene(str(bad), str(scene / "transforms.json"), str(tmp_path / f"surfs{device_decode}"), device_decode=device_decode, **KW)
        texts.append(str(e.value))
    assert texts[0] == texts[1] and "image mode 'RGB', expected 'L' or '1'" in texts[0]


def test_evaluate_results_writes_the_same_metrics(tmp_path):
    rng = np.random.default_rng(0)
    y, x = np.mgrid[0:40, 0:72]
    for cam in ("00", "01"):
        for frame in range(3):
            gt = np.stack([(x * 3 + y * 2 + 30 * frame) & 255, (x + y * 5 + 17 * int(cam)) & 255, (x * y // 5) & 255], axis=-1).astype(np.uint8)
            pred = np.clip(gt.astype(np.int16) + rng.integers(-12, 13, gt.shape), 0, 255).astype(np.uint8)
            mask = np.zeros((40, 72), dtype=np.uint8)
            mask[4:36, 10:60] = 255
            mask[4:36, 9] = 130
            for sub, a, ext, kw in (("pred", pred, ".png", {}), ("gt", gt, ".jpg", dict(quality=95, subsampling=0)), ("fmasks", mask, ".png", {})):
                path = tmp_path / sub / cam / f"{frame:06d}{ext}"
                path.parent.mkdir(parents=True, exist_ok=True)
                Image.fromarray(a).save(path, **kw)
    seen = []
    real = pngdec.decode_plans

    def spy(plans, *a, **kw):
        st = real(plans, *a, **kw)
        seen.append(([p.channels for p in plans], st))
        return st
    texts = {}
    for device_decode in (False, True):
        out = tmp_path / f"metrics_{device_decode}.json"
        pngdec.decode_plans = spy
        try:
            res = metrics.evaluate_results(str(tmp_path / "pred"), str(tmp_path / "gt"), str(tmp_path / "fmasks"), ".png", ".jpg", ".png",
                                           out_metrics_path=str(out), background_color="white", gpu_ids=[0], canvas_size=72, batch_size=4,
                                           device_decode=device_decode)
        finally:
            pngdec.decode_plans = real
        assert len(res["values"]) == 6
        texts[device_decode] = out.read_text()
    assert texts[True] == texts[False] and json.loads(texts[True])["mean"]["psnr"] > 10
    # two batches (4 + 2 pairs): per pair one RGB prediction and one mask, every one decoded on the device
    assert [sorted(ch) for ch, _ in seen] == [[1] * 4 + [3] * 4, [1] * 2 + [3] * 2] and all(s == 0 for _, st in seen for s in st)


def test_evaluator_keeps_its_mode_checks(tmp_path):
    rgb, rgba, gray = tmp_path / "c.png", tmp_path / "a.png", tmp_path / "g.png"
    a = np.random.default_rng(1).integers(0, 256, (40, 72, 4), dtype=np.uint8)
    Image.fromarray(a[..., :3]).save(rgb), Image.fromarray(a).save(rgba), Image.fromarray(a[..., 0]).save(gray)
    for device_decode in (False, True):
        ev = metrics.ImageEvaluator("cuda", device_decode=device_decode)
        with pytest.raises(ValueError, match="image mode 'RGBA', expected 'RGB'"):
            ev(str(rgba), str(rgb), crop_with_fmask=False)
        with pytest.raises(ValueError, match="image mode 'RGB', expected 'L'"):
            ev(str(rgb), str(rgb), pred_fmask=str(rgb), canvas_size=72)
        assert ev(str(rgb), str(rgb), pred_fmask=str(gray), gt_fmask=str(gray), crop_with_fmask=False, canvas_size=72)[1] == pytest.approx(1.0)
