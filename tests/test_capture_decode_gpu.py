"""GPU: SpaTemDataset(device_decode=True) against the flag-off call on the scenes of tests/kp2d_scene.py with JPEG images (4:2:0 and
4:4:4) and PNG masks and skeletons: every entry of the get_item dict equal, every JPEG and PNG file decoded on the device; WebP images,
a progressive JPEG and an interlaced PNG keep the Pillow route inside the same call; every error of _load_frame comes with the same
class and text, the first bad frame's in label order."""
import shutil
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

import kp2d_scene as ks
import pngdec_cases as pc
from diffuman4d_amd.host import capture, ops, skeleton, triang

pytestmark = pytest.mark.gpu

PALETTE = skeleton.load_palette(ks.PALETTE_PATH)
OUT = 64
FLAVOURS = {"jpg420": (".jpg", {"quality": 92}), "jpg444": (".jpg", {"quality": 92, "subsampling": 0}), "webp": (".webp", {"lossless": True})}

# as tests/test_capture_kp2d_gpu.py: the device entries, whatever another test module left installed in capture.ops
GENUINE = {name: getattr(ops, name) for name in ("capture_crop_resize", "skeleton_draw", "skeleton_box_mask", "capture_plane_stats",
                                                 "capture_fill_rects")}
assert all(f.__module__ == ops.__name__ for f in GENUINE.values())


@pytest.fixture(autouse=True)
def genuine_ops(monkeypatch):
    for name, f in GENUINE.items():
        monkeypatch.setattr(ops, name, f)


@pytest.fixture(scope="module")
def scenes(hip_device, tmp_path_factory):
    """One scene per size of kp2d_scene.SIZES, as tests/test_capture_kp2d_gpu.py builds them, with the images re-saved per flavour."""
    roots = []
    for hw in ks.SIZES:
        root = tmp_path_factory.mktemp(f"decode_{hw[0]}x{hw[1]}")
        d = ks.write_cameras_and_detections(root, hw)
        triang.triangulate_skeleton(str(d / "transforms.json"), str(d / "poses_sapiens"), str(d / "poses_3d"),
                                    out_kp2d_proj_dir=str(d / "poses_2d"), spa_labels_proj=list(range(8)))
        ks.write_images_and_masks(d, hw)
        ks.write_skeleton_pngs(d, hw, PALETTE, skeleton.draw_plans)
        for name, (ext, kw) in FLAVOURS.items():
            for p in sorted((d / "images").rglob("*.png")):
                q = d / name / p.parent.name / (p.stem + ext)
                q.parent.mkdir(parents=True, exist_ok=True)
                Image.open(p).save(q, **kw)
        roots.append(root)
    return roots


def dataset(root, flavour="jpg420", **kw):
    pats = {"image_path_pat": "{data_dir}/{scene_label}/" + flavour + "/{spa_label}/{tem_label}" + FLAVOURS[flavour][0],
            "skeleton_path_pat": ks.patterns()["skeleton_path_pat"]}
    return capture.SpaTemDataset(data_dir=str(root), scene_label=ks.SCENE, height=OUT, width=OUT, decode_threads=4, **{**pats, **kw})


def same(a, b):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert a[k].device == b[k].device and torch.equal(a[k], b[k]), (k, int((a[k] != b[k]).sum()))
        else:
            assert a[k] == b[k], k


def file_counts(labels, has_gt_target, source):
    """(image files, PNG files) a task reads."""
    full = sum(1 for _, spa, _ in labels if has_gt_target or spa in ks.INPUTS)
    return full, full + (len(labels) if source == "files" else 0)


@pytest.mark.parametrize("source", ["files", "kp2d"])
@pytest.mark.parametrize("has_gt_target", [True, False])
@pytest.mark.parametrize("task", ["spatial", "temporal"])
@pytest.mark.parametrize("size,flavour", [(0, "jpg420"), (0, "jpg444"), (1, "jpg420"), (1, "jpg444")])
def test_flag_on_equals_flag_off(scenes, size, flavour, task, has_gt_target, source):
    spa, tem = ks.TASKS[task]
    kw = dict(has_gt_target=has_gt_target, **({"skeleton_source": "kp2d", "palette": PALETTE} if source == "kp2d" else {}))
    off, on = dataset(scenes[size], flavour, **kw), dataset(scenes[size], flavour, device_decode=True, **kw)
    want, got = off.get_item(ks.SCENE, spa, tem, ks.INPUTS), on.get_item(ks.SCENE, spa, tem, ks.INPUTS)
    same(got, want)
    assert got["pixel_values"].is_cuda and got["skeletons"].max() > -1.0
    images, pngs = file_counts(want["labels"], has_gt_target, source)
    assert on.decode_stats["device"] == images + pngs and on.decode_stats["pillow"] == 0 and on.decode_stats["bytes_uploaded"] > 0
    assert off.decode_stats == {"device": 0, "pillow": 0, "bytes_uploaded": 0}
    same(on.get_item(ks.SCENE, spa, tem, ks.INPUTS), want)  # a second call: the same again, and the counts add up
    assert on.decode_stats["device"] == 2 * (images + pngs)


@pytest.mark.parametrize("has_gt_target", [True, False])
def test_webp_images_keep_the_pillow_route(scenes, has_gt_target):
    spa, tem = ks.TASKS["spatial"]
    want = dataset(scenes[0], "webp", has_gt_target=has_gt_target).get_item(ks.SCENE, spa, tem, ks.INPUTS)
    on = dataset(scenes[0], "webp", has_gt_target=has_gt_target, device_decode=True)
    same(on.get_item(ks.SCENE, spa, tem, ks.INPUTS), want)
    images, pngs = file_counts(want["labels"], has_gt_target, "files")
    h, w = ks.SIZES[0]
    assert on.decode_stats["pillow"] == images and on.decode_stats["device"] == pngs and on.decode_stats["bytes_uploaded"] > images * h * w * 3


def interlaced_png(mask: np.ndarray) -> bytes:
    """An Adam7 file of a mode-L plane, every row with filter 0 (Pillow writes no interlaced files)."""
    raw = b""
    for x0, y0, dx, dy in ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)):
        sub = mask[y0::dy, x0::dx]
        if sub.size:
            raw += b"".join(b"\0" + np.ascontiguousarray(row).tobytes() for row in sub)
    h, w = mask.shape
    return pc.SIGNATURE + pc.ihdr(h, w, 1, interlace=1) + pc.chunk(b"IDAT", zlib.compress(raw)) + pc.chunk(b"IEND", b"")


@pytest.fixture()
def scene(scenes, tmp_path):
    """A copy of the first scene that a test may damage."""
    shutil.copytree(scenes[0] / ks.SCENE, tmp_path / ks.SCENE)
    return tmp_path


def test_files_the_probes_refuse(scene):
    d = scene / ks.SCENE
    Image.open(d / "images" / "01" / "000000.png").save(d / "jpg420" / "01" / "000000.jpg", quality=92, progressive=True)
    mask = np.asarray(Image.open(d / "fmasks" / "05" / "000000.png"))
    (d / "fmasks" / "05" / "000000.png").write_bytes(interlaced_png(mask))
    assert np.array_equal(np.asarray(Image.open(d / "fmasks" / "05" / "000000.png")), mask)
    spa, tem = ks.TASKS["spatial"]
    for kw in ({}, {"skeleton_source": "kp2d", "palette": PALETTE}):
        want = dataset(scene, **kw).get_item(ks.SCENE, spa, tem, ks.INPUTS)
        on = dataset(scene, device_decode=True, **kw)
        same(on.get_item(ks.SCENE, spa, tem, ks.INPUTS), want)
        images, pngs = file_counts(want["labels"], True, "kp2d" if kw else "files")
        assert on.decode_stats["pillow"] == 2 and on.decode_stats["device"] == images + pngs - 2


def both(root, cls, spa=None, **kw):
    """The error of the flag-off call and of the flag-on call: the same class and text -> the text."""
    spa_, tem = ks.TASKS["spatial"]
    texts = []
    for flag in (False, True):
        with pytest.raises(cls) as e:
            dataset(root, device_decode=flag, **kw).get_item(ks.SCENE, spa or spa_, tem, ks.INPUTS)
        assert type(e.value) is cls
        texts.append(str(e.value))
    assert texts[0] == texts[1], texts
    return texts[0]


KP2D = {"skeleton_source": "kp2d", "palette": PALETTE}


def save(path, array, **kw):
    Image.fromarray(array).save(path, **kw)


def test_the_errors_of_load_frame_are_the_same(scene):
    d = scene / ks.SCENE
    h, w = ks.SIZES[0]
    spare = scene / "spare"
    shutil.copytree(d, spare / ks.SCENE)

    def fresh():
        shutil.rmtree(d)
        shutil.copytree(spare / ks.SCENE, d)
    # a gray JPEG as image: mode 'L'
    save(d / "jpg420" / "03" / "000000.jpg", np.zeros((h, w), np.uint8) + 90, quality=92)
    for kw in ({}, KP2D):
        assert "image mode 'L', expected 'RGB'" in both(scene, ValueError, **kw)
    # an RGBA PNG as image
    fresh()
    pats = {"image_path_pat": ks.patterns()["image_path_pat"]}
    save(d / "images" / "03" / "000000.png", np.full((h, w, 4), 200, np.uint8))
    assert "image mode 'RGBA', expected 'RGB'" in both(scene, ValueError, **pats)
    # an RGB PNG as mask
    fresh()
    save(d / "fmasks" / "03" / "000000.png", np.full((h, w, 3), 200, np.uint8))
    assert "image mode 'RGB', expected 'L'" in both(scene, ValueError)
    # an empty mask
    fresh()
    save(d / "fmasks" / "04" / "000000.png", np.zeros((h, w), np.uint8))
    for kw in ({}, KP2D):
        assert both(scene, ValueError, **kw).startswith("foreground mask is empty: ") and "jpg420/04/000000.jpg" in both(scene, ValueError, **kw)
    # an empty skeleton that serves as image
    fresh()
    save(d / "skeletons" / "06" / "000000.png", np.zeros((h, w, 3), np.uint8))
    assert both(scene, ValueError, has_gt_target=False).startswith("skeleton is empty, no mask can be made from it: ")
    # sizes that differ
    fresh()
    m = np.zeros((h, w + 1), np.uint8)
    m[20:200, 30:200] = 255
    save(d / "fmasks" / "02" / "000000.png", m)
    for kw in ({}, KP2D):
        assert both(scene, AssertionError, **kw) == f"Error: image size: ({w}, {h}) != fmask size: ({w + 1}, {h}) != skeleton size: ({w}, {h})"
    # an input camera's mask below 2 %, and one exactly in the band of the limit (the host decides, the same way)
    fresh()
    m = np.zeros((h, w), np.uint8)
    m[100:110, 100:110] = 255
    save(d / "fmasks" / "05" / "000000.png", m)
    for kw in ({}, KP2D):
        assert both(scene, AssertionError, **kw) == "Error: foreground mask < 2%. Please check the data."
    m[:] = 0
    m.reshape(-1)[: h * w // 50] = 255  # 1632 of 81 600 pixels: exactly 2 %
    save(d / "fmasks" / "05" / "000000.png", m)
    assert capture._sum_mean_at_most(int(m.sum(dtype=np.int64)), m.size, 0.02) is None
    if capture._mask_mean_at_most(m, 0.02):
        assert both(scene, AssertionError) == "Error: foreground mask < 2%. Please check the data."
    else:
        spa, tem = ks.TASKS["spatial"]
        same(dataset(scene, device_decode=True).get_item(ks.SCENE, spa, tem, ks.INPUTS), dataset(scene).get_item(ks.SCENE, spa, tem, ks.INPUTS))
    # a target's mask below 2 % is no error (only inputs are checked): both modes agree on that too
    fresh()
    m[:] = 0
    m[100:110, 100:110] = 255
    save(d / "fmasks" / "06" / "000000.png", m)
    spa, tem = ks.TASKS["spatial"]
    same(dataset(scene, device_decode=True).get_item(ks.SCENE, spa, tem, ks.INPUTS), dataset(scene).get_item(ks.SCENE, spa, tem, ks.INPUTS))


def test_of_two_bad_frames_the_earlier_one_is_raised(scene):
    d = scene / ks.SCENE
    h, w = ks.SIZES[0]
    gray, empty = np.zeros((h, w), np.uint8) + 90, np.zeros((h, w), np.uint8)
    # camera 02's mask is empty (known after the device's statistics), camera 04's image cannot be read as RGB (known at once)
    save(d / "fmasks" / "02" / "000000.png", empty)
    save(d / "jpg420" / "04" / "000000.jpg", gray, quality=92)
    for kw in ({}, KP2D):
        assert both(scene, ValueError, **kw).startswith("foreground mask is empty: ")
    # the other way round
    shutil.copyfile(d / "fmasks" / "03" / "000000.png", d / "fmasks" / "02" / "000000.png")
    save(d / "jpg420" / "01" / "000000.jpg", gray, quality=92)
    save(d / "fmasks" / "04" / "000000.png", empty)
    for kw in ({}, KP2D):
        assert "jpg420/01/000000.jpg: image mode 'L'" in both(scene, ValueError, **kw)
    # two errors that both wait for the statistics: input camera 01 below 2 %, camera 04 still empty
    Image.open(d / "images" / "01" / "000000.png").save(d / "jpg420" / "01" / "000000.jpg", quality=92)
    m = empty.copy()
    m[100:110, 100:110] = 255
    save(d / "fmasks" / "01" / "000000.png", m)
    assert both(scene, AssertionError) == "Error: foreground mask < 2%. Please check the data."
