"""GPU: the pose stage with device_decode: pose_inputs, fmask_boxes and predict_keypoints give the same tensors, boxes and JSON files
whether Pillow or the device decodes the JPEG / PNG inputs; WebP images, mode-1 masks and progressive JPEG files keep the Pillow route
inside the same call."""
import numpy as np
import pytest
import torch
from PIL import Image

from diffuman4d_amd.host import codec, pose

pytestmark = pytest.mark.gpu

SHAPE = (32, 24)
SIZES = [(37, 50), (64, 64), (33, 47), (40, 40), (21, 30)]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """images/{cam}/{k}.jpg|.webp and fmasks/{cam}/{k}.png: baseline 4:2:0 and 4:4:4 JPEG, a grayscale JPEG, a progressive JPEG, a WebP;
    masks of mode L and one of mode 1."""
    root = tmp_path_factory.mktemp("pose_decode")
    rng = np.random.default_rng(9)
    images, masks = [], []
    for k, (h, w) in enumerate(SIZES):
        yy, xx = np.mgrid[:h, :w]
        img = np.stack([(xx * 5 + 3 * k) % 256, (yy * 7) % 256, (xx + yy) * 2 % 256], -1).astype(np.uint8)
        img = (img // 2 + rng.integers(0, 128, img.shape)).astype(np.uint8)
        m = (((xx - w / 2) / (0.3 * w)) ** 2 + ((yy - h / 2) / (0.4 * h)) ** 2 < 1)
        soft = np.where(m, 255, (xx * 3) % 120).astype(np.uint8)
        ip = root / "images" / "00" / f"{k:06d}{'.webp' if k == 4 else '.jpg'}"
        mp = root / "fmasks" / "00" / f"{k:06d}.png"
        ip.parent.mkdir(parents=True, exist_ok=True)
        mp.parent.mkdir(parents=True, exist_ok=True)
        im = Image.fromarray(img)
        if k == 0:
            im.save(ip, quality=90)
        elif k == 1:
            im.save(ip, quality=85, subsampling=0)
        elif k == 2:
            im.convert("L").save(ip, quality=90)
        elif k == 3:
            im.save(ip, quality=90, progressive=True)
        else:
            im.save(ip, lossless=True)
        (Image.fromarray(m).convert("1") if k == 3 else Image.fromarray(soft)).save(mp)
        images.append(str(ip)), masks.append(str(mp))
    return root, images, masks


def counting(monkeypatch):
    """How many files each decode_staged call of the pose stage took."""
    taken = []
    real = codec.decode_staged
    monkeypatch.setattr(pose, "decode_staged", lambda entries, *a, **k: taken.append(len(entries)) or real(entries, *a, **k))
    return taken


def test_pose_inputs_and_fmask_boxes(hip_device, files, monkeypatch):
    _, images, masks = files
    taken = counting(monkeypatch)
    want = pose.pose_inputs(images, masks, None, SHAPE, hip_device, bbox_source="fmask")
    assert taken == []
    got = pose.pose_inputs(images, masks, None, SHAPE, hip_device, bbox_source="fmask", device_decode=True)
    assert taken == [3 + 4]  # three JPEG images (not the progressive one, not the WebP) and the four mode-L masks
    assert torch.equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    boxes = pose.fmask_boxes(masks, hip_device)
    assert np.array_equal(pose.fmask_boxes(masks, hip_device, device_decode=True), boxes) and taken == [7, 4]
    assert (boxes[:, 2] > boxes[:, 0]).all()
    # no masks, caller's boxes, one image alone
    a = pose.pose_inputs(images[:2], None, [[2.5, 3.0, 30.0, 33.0], None], SHAPE, hip_device)
    b = pose.pose_inputs(images[:2], None, [[2.5, 3.0, 30.0, 33.0], None], SHAPE, hip_device, device_decode=True)
    assert torch.equal(a[0], b[0]) and taken[-1] == 2
    # only files the device does not take: nothing is handed to it
    c = pose.pose_inputs(images[3:], masks[3:4] + [None], None, SHAPE, hip_device, device_decode=True)
    assert torch.equal(c[0], pose.pose_inputs(images[3:], masks[3:4] + [None], None, SHAPE, hip_device)[0]) and taken[-1] == 2


def test_the_errors_are_the_same(hip_device, files, tmp_path):
    _, images, masks = files
    Image.fromarray(np.zeros((37, 50, 3), np.uint8)).save(tmp_path / "rgb_mask.png")
    for bad in ([str(tmp_path / "rgb_mask.png")], [masks[1]]):  # a mask's mode; a mask's size
        texts = []
        for flag in (False, True):
            with pytest.raises(ValueError) as e:
                pose.pose_inputs(images[:1], bad, None, SHAPE, hip_device, device_decode=flag)
            texts.append(str(e.value))
        assert texts[0] == texts[1]


def test_predict_keypoints_writes_the_same_files(hip_device, files, tmp_path):
    root, images, _ = files

    def net(x):  # a stand-in pose network: 5 maps of the input's quarter size, a function of the input
        pooled = torch.nn.functional.avg_pool2d(x.mean(dim=1, keepdim=True), 4)
        return torch.cat([pooled * s + 0.1 * k for k, s in enumerate((1.0, -1.0, 0.5, 2.0, -0.3))], dim=1)
    out = {}
    for flag in (False, True):
        dst = tmp_path / f"kp_{flag}"
        res = pose.predict_keypoints(str(root / "images"), str(dst), str(root / "fmasks"), pose_model=net, shape=SHAPE, batch_size=2,
                                     gpu_ids=[hip_device.index or 0], num_workers=2, bbox_source="fmask", device_decode=flag)
        assert res == {"images": len(images), "written": len(images), "skipped": 0}
        out[flag] = {p.relative_to(dst).as_posix(): p.read_bytes() for p in sorted(dst.rglob("*.json"))}
    assert len(out[True]) == len(images) and out[True] == out[False]
