"""GPU: the two dm4d_detect_* kernels and the detector route of predict_keypoints against tests/detect_model.py.  Everything is compared
bit for bit: the detector's input, the kept boxes, scores, anchor indices and counts, and the keypoints in the JSON files.

An image that mmcv's keep-ratio rule does not fit into a canvas (263 x 301 into 96 x 64: the rule looks at the longer and the shorter
side, not at width and height) is refused with a ValueError before any launch; that is asserted where such a pair comes up."""
import functools
import json

import numpy as np
import pytest
import torch
from PIL import Image

import detect_model as M
from test_pose_gpu import stub_model

pytestmark = pytest.mark.gpu

SIZES = [(37, 23), (64, 48), (301, 263), (263, 301)]  # (h, w)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# -- network input ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sources():
    rng = np.random.default_rng(17)
    images, masks = [], []
    for h, w in SIZES:
        yy, xx = np.mgrid[:h, :w]
        base = np.stack([xx * 255.0 / (w - 1), yy * 255.0 / (h - 1), (xx + yy) * 255.0 / (h + w - 2)], -1)
        images.append(np.clip(base + rng.normal(0, 20, (h, w, 3)), 0, 255).astype(np.uint8))
        m = rng.integers(0, 256, (h, w), dtype=np.uint8)
        m[: h // 3] = 255
        m[-(h // 4):] = 0
        masks.append(m)
    return images, masks


@functools.lru_cache(maxsize=None)
def input_reference(k, shape, masked):
    images, masks = sources()
    return M.detector_input(images[k], masks[k] if masked else None, shape)


@pytest.mark.parametrize("shape", [(64, 64), (96, 64)])
@pytest.mark.parametrize("masked", [True, False])
def test_input_is_bit_equal_to_the_model_alone_and_in_a_batch(hip_device, shape, masked):
    from diffuman4d_amd.host import detect
    images, masks = sources()
    fit = [k for k, (h, w) in enumerate(SIZES) if M.fits(h, w, shape)]
    assert fit == ([0, 1, 2, 3] if shape == (64, 64) else [0, 1, 2])
    for k in set(range(4)) - set(fit):
        with pytest.raises(ValueError, match="does not fit"):
            detect.detector_inputs([images[k]], None, shape, hip_device)
    x, meta = detect.detector_inputs([images[k] for k in fit], [masks[k] for k in fit] if masked else None, shape, hip_device)
    assert x.shape == (len(fit), 3) + shape and x.dtype == torch.float32 and x.device == hip_device
    got = x.cpu().numpy()
    for r, k in enumerate(fit):
        ref = input_reference(k, shape, masked)
        assert np.array_equal(bits(got[r]), bits(ref)), f"image {k}: {np.count_nonzero(bits(got[r]) != bits(ref))} values differ"
        assert meta["resized"][r].tolist() == list(M.rescaled_size(*SIZES[k], shape)) and tuple(meta["inv_scale"][r]) == M.inv_scale(*SIZES[k], shape)
        alone, _ = detect.detector_inputs([images[k]], [masks[k]] if masked else None, shape, hip_device)
        assert np.array_equal(bits(alone.cpu().numpy()[0]), bits(got[r]))
    # an image without a mask beside one with a mask, in another order
    mixed, _ = detect.detector_inputs([images[2], images[0]], [None, masks[0]], shape, hip_device)
    assert np.array_equal(bits(mixed.cpu().numpy()[0]), bits(input_reference(2, shape, False)))
    assert np.array_equal(bits(mixed.cpu().numpy()[1]), bits(input_reference(0, shape, True)))


def test_input_at_the_default_canvas_and_with_other_statistics(hip_device):
    from diffuman4d_amd.host import detect
    images, masks = sources()
    x, meta = detect.detector_inputs([images[2]], [masks[2]], device=hip_device)
    assert x.shape == (1, 3, 640, 640) and meta["resized"].tolist() == [[559, 640]]
    assert np.array_equal(bits(x.cpu().numpy()[0]), bits(input_reference(2, (640, 640), True)))
    kw = dict(mean=(1.5, 100.25, 127.0), std=(3.0, 60.5, 0.7), pad_value=7)
    for order in ("rgb", "bgr"):
        y, _ = detect.detector_inputs([images[0]], None, (64, 64), hip_device, channel_order=order, **kw)
        assert np.array_equal(bits(y.cpu().numpy()[0]), bits(M.detector_input(images[0], None, (64, 64), channel_order=order, **kw)))


def test_input_from_files_with_and_without_device_decode(hip_device, tmp_path):
    """JPEG images and PNG masks: the tensor is the same whether Pillow or the device decodes them, and it is the model's of Pillow's pixels."""
    from diffuman4d_amd.host import detect
    images, masks = sources()
    ipaths, mpaths = [], []
    for k in (1, 2, 3):
        ipaths.append(str(tmp_path / f"{k}.jpg")), mpaths.append(str(tmp_path / f"{k}.png"))
        Image.fromarray(images[k]).save(ipaths[-1], quality=90)
        Image.fromarray(masks[k]).save(mpaths[-1])
    a, _ = detect.detector_inputs(ipaths, mpaths, (64, 64), hip_device)
    b, _ = detect.detector_inputs(ipaths, mpaths, (64, 64), hip_device, device_decode=True)
    assert torch.equal(a, b)
    for r, (ip, mp) in enumerate(zip(ipaths, mpaths)):
        ref = M.detector_input(np.asarray(Image.open(ip).convert("RGB")), np.asarray(Image.open(mp)), (64, 64))
        assert np.array_equal(bits(a.cpu().numpy()[r]), bits(ref))


# -- selection -------------------------------------------------------------------------------------------------------------------------
def dense(A, C, seed, share=0.3, levels=None):
    """Clustered boxes [A, 4] in a 640 x 640 canvas and scores [A, C] of which about `share` lie above 0.3; levels: that many distinct
    score values only (ties)."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(60, 580, (max(A // 40, 1), 2))
    c = centres[rng.integers(0, len(centres), A)] + rng.normal(0, 15, (A, 2))
    wh = rng.uniform(20, 160, (A, 2))
    boxes = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)
    s = rng.random((A, C))
    scores = np.where(s < share, 0.3 + 0.7 * rng.random((A, C)), 0.3 * rng.random((A, C)))
    if levels:
        scores = np.round(scores * levels) / levels
    return boxes, scores.astype(np.float32)


INV = (np.float32(1.0 / (640 / 2448)), np.float32(1.0 / (535 / 2048)))


def run(hip_device, boxes, scores, inv, cat=0, score_thr=0.3, nms_thr=0.3, keep=100):
    """boxes [n, A, 4], scores [n, A, C], inv [n, 2] numpy -> (counts, out, idx) numpy."""
    from diffuman4d_amd.host import ops
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(hip_device)
    counts, out, idx = ops.detect_select(t(boxes), t(scores), t(inv), cat, score_thr, nms_thr, keep)
    torch.cuda.synchronize()
    return counts.cpu().numpy(), out.cpu().numpy(), idx.cpu().numpy()


def same(got, want, what=""):
    counts, out, idx = got
    assert counts.tolist() == want[0], (what, counts.tolist(), want[0])
    assert np.array_equal(idx, want[2]), what
    assert np.array_equal(bits(out), bits(want[1])), what


@pytest.mark.parametrize("A", [1, 63, 64, 65, 1000, 8400])
@pytest.mark.parametrize("C,cat", [(1, 0), (3, 0), (3, 2)])
def test_select_is_bit_equal_to_the_model(hip_device, A, C, cat):
    boxes, scores = dense(A, C, A * 10 + C + cat)
    if A == 1:
        scores[0, cat] = 0.7
    want = M.select(boxes, scores, INV, cat)
    got = run(hip_device, boxes[None], scores[None], np.array([INV]), cat)
    same([g[0] for g in got], want)
    assert want[0][2] > 0 and (A < 1000 or want[0][0] < min(want[0][2], 100))  # something passes; in the large cases the NMS removes something


def test_select_edges_of_threshold_and_cap(hip_device):
    boxes, scores = dense(1000, 1, 5)
    below = np.minimum(scores, np.float32(0.3))  # all at or below the threshold: it is strict
    same([g[0] for g in run(hip_device, boxes[None], below[None], np.array([INV]))], M.select(boxes, below, INV))
    assert M.select(boxes, below, INV)[0] == [0, 0, 0]
    k = np.arange(1000)
    apart = np.stack([(k % 40) * 15.0, (k // 40) * 15.0, (k % 40) * 15.0 + 5, (k // 40) * 15.0 + 5], 1).astype(np.float32)  # nothing overlaps
    rng = np.random.default_rng(6)
    for above in (100, 101):  # exactly max_per_img candidates, and one more
        s = (0.29 * rng.random(1000)).astype(np.float32)
        s[rng.permutation(1000)[:above]] = (0.31 + 0.6 * rng.random(above)).astype(np.float32)
        want = M.select(apart, s[:, None], INV)
        assert want[0] == [100, 0, above]
        same([g[0] for g in run(hip_device, apart[None], s[None, :, None], np.array([INV]))], want, above)
    for keep in (1, 2, 37, 256):
        same([g[0] for g in run(hip_device, boxes[None], scores[None], np.array([INV]), keep=keep)], M.select(boxes, scores, INV, max_per_img=keep), keep)
    for thr in (0.0, 0.1, 0.7, 1.0):
        same([g[0] for g in run(hip_device, boxes[None], scores[None], np.array([INV]), nms_thr=thr)], M.select(boxes, scores, INV, nms_thr=thr), thr)


@pytest.mark.parametrize("levels", [None, 7, 1])
def test_select_with_5000_candidates_and_repeated_scores(hip_device, levels):
    """More candidates than places: the radix select; with few distinct scores (levels = 1: one) it has to go down to the index bits."""
    boxes, scores = dense(8400, 1, 9, share=0.7, levels=None if levels == 1 else levels)
    if levels == 1:
        scores[:] = np.where(scores > 0.3, np.float32(0.75), np.float32(0.25))
    want = M.select(boxes, scores, INV)
    assert want[0][2] >= 5000
    same([g[0] for g in run(hip_device, boxes[None], scores[None], np.array([INV]))], want)
    if levels == 1:  # the first 100 anchors above the threshold are the ones that reach the NMS
        assert want[2][0] == np.nonzero(scores[:, 0] > 0.3)[0][0]


def test_select_drops_and_counts_what_cannot_be_a_box(hip_device):
    boxes, scores = dense(1000, 1, 12, share=0.2)
    hot = np.nonzero(scores[:, 0] > 0.3)[0]
    scores[hot[0::9], 0] = np.nan
    scores[hot[1::9], 0] = np.inf  # passes, and sorts first
    boxes[hot[2::9], 2] = boxes[hot[2::9], 0]          # x2 == x1
    boxes[hot[3::9], 3] = boxes[hot[3::9], 1] - 1      # y2 < y1
    boxes[hot[4::9], 0] = np.nan
    boxes[hot[5::9], 3] = np.inf
    boxes[hot[6::9], 2] = 3e38                         # finite until it is scaled
    scores[hot[7::9], 0] = -0.0
    want = M.select(boxes, scores, INV)
    assert want[0][1] == sum(len(hot[j::9]) for j in (2, 3, 4, 5, 6)) and want[0][2] == len(hot) - len(hot[0::9]) - len(hot[7::9])
    same([g[0] for g in run(hip_device, boxes[None], scores[None], np.array([INV]))], want)
    # a negative threshold: zeros of either sign pass and tie
    want = M.select(boxes, scores, INV, score_thr=-0.5, max_per_img=256)
    same([g[0] for g in run(hip_device, boxes[None], scores[None], np.array([INV]), score_thr=-0.5, keep=256)], want)


def test_select_does_not_depend_on_the_batch_or_the_run(hip_device):
    sets = [dense(1000, 3, 20 + k, share=0.1 + 0.15 * k) for k in range(5)]
    order = [0, 1, 2, 3, 4, 0]  # the same image at positions 0 and 5
    boxes, scores = np.stack([sets[k][0] for k in order]), np.stack([sets[k][1] for k in order])
    inv = np.array([[1.0 + 0.37 * k, 2.0 - 0.21 * k] for k in order], dtype=np.float32)
    a = run(hip_device, boxes, scores, inv, cat=1)
    b = run(hip_device, boxes, scores, inv, cat=1)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    for x in a:
        assert x[0].tobytes() == x[5].tobytes()
    for r, k in enumerate(order):
        same([g[r] for g in a], M.select(sets[k][0], sets[k][1], tuple(inv[r]), 1), r)
    alone = run(hip_device, boxes[3:4], scores[3:4], inv[3:4], cat=1)
    for x, y in zip(alone, a):
        assert x[0].tobytes() == y[3].tobytes()


def test_select_boxes_checks_and_returns_lists(hip_device):
    from diffuman4d_amd.host import detect
    images, _ = sources()
    _, meta = detect.detector_inputs(images[:2], None, (64, 64), hip_device)
    boxes, scores = dense(65, 2, 3)
    tb = torch.from_numpy(np.stack([boxes, boxes])).to(hip_device)
    ts = torch.from_numpy(np.stack([scores, np.zeros_like(scores)])).to(hip_device)
    kept, sc = detect.select_boxes(tb, ts, meta, det_cat_id=1)
    want = M.select(boxes, scores, M.inv_scale(*SIZES[0], (64, 64)), 1)
    assert len(kept) == 2 and kept[0].dtype == np.float32 and kept[0].shape == (want[0][0], 4) and kept[1].shape == (0, 4) and sc[1].shape == (0,)
    assert np.array_equal(bits(kept[0]), bits(want[1][:want[0][0], :4])) and np.array_equal(bits(sc[0]), bits(want[1][:want[0][0], 4]))
    with pytest.raises(ValueError, match=r"boxes: expected \[2, A, 4\]"):
        detect.select_boxes(tb[:1], ts[:1], meta)
    with pytest.raises(ValueError, match="scores: expected"):
        detect.select_boxes(tb, ts[:, :10], meta)


# -- end to end ------------------------------------------------------------------------------------------------------------------------
DET_SHAPE = (64, 64)
POSE_SHAPE = (64, 48)
E2E_SIZES = [(80, 60), (64, 48), (50, 70), (33, 47), (90, 41), (64, 64)]


def planted():
    """The stand-in detector's output for a batch of three, by position: no box above the threshold; two that overlap (one stays); five
    of which three stay.  [3, 12, 4] canvas pixels and [3, 12, 2] scores; the persons are class 1."""
    boxes = np.tile(np.array([[2, 2, 6, 6]], dtype=np.float32), (3, 12, 1))
    scores = np.zeros((3, 12, 2), dtype=np.float32)
    scores[:, :, 0] = 0.9  # another class: never looked at
    scores[0, :, 1] = 0.2
    boxes[1, 4], boxes[1, 9] = [5, 8, 30, 40], [6, 9, 31, 42]
    scores[1, 4, 1], scores[1, 9, 1] = 0.6, 0.8
    boxes[2, [1, 3, 5, 7, 11]] = [[3, 4, 20, 30], [4, 4, 21, 31], [25, 10, 40, 38], [10, 20, 30.5, 36.25], [26, 11, 40, 37]]
    scores[2, [1, 3, 5, 7, 11], 1] = [0.5, 0.7, 0.9, 0.31, 0.85]
    return boxes, scores


def stand_in_detector(x):
    """Ignores the values of its input, checks its form, returns the planted output for as many images as it was given."""
    assert isinstance(x, torch.Tensor) and x.device.type == "cuda" and x.dtype == torch.float32 and x.shape[1:] == (3,) + DET_SHAPE and x.shape[0] <= 3
    boxes, scores = planted()
    return torch.from_numpy(boxes[: x.shape[0]]).to(x.device), torch.from_numpy(scores[: x.shape[0]]).to(x.device)


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """Six images (lossless WebP) with masks (PNG) in two camera folders; sorted paths = the order of E2E_SIZES."""
    root = tmp_path_factory.mktemp("detect_e2e")
    rng = np.random.default_rng(23)
    images, masks = [], []
    for k, (h, w) in enumerate(E2E_SIZES):
        ys, xs = np.mgrid[0:h, 0:w]
        blob = 200 * np.exp(-((xs - 0.4 * w) ** 2 + (ys - 0.55 * h) ** 2) / (2 * 6.0 ** 2))
        a = np.clip(blob[..., None] + rng.integers(0, 8, (h, w, 3)), 0, 255).astype(np.uint8)
        m = np.zeros((h, w), dtype=np.uint8)
        m[h // 5: h - 3, w // 6: w - w // 4] = 255
        m[:2] = 90
        images.append(a), masks.append(m)
        for d, arr in (("images", a), ("fmasks", m)):
            path = root / d / f"{k // 3:02d}" / (f"{k:06d}" + (".png" if d == "fmasks" else ".webp"))
            path.parent.mkdir(parents=True, exist_ok=True)
            Image.fromarray(arr).save(path, lossless=True) if d == "images" else Image.fromarray(arr).save(path)
    return root, images, masks


def files_of(root):
    return {p.relative_to(root).as_posix(): p.read_bytes() for p in sorted(root.rglob("*.json"))}


def test_predict_keypoints_with_a_detector(hip_device, scene, tmp_path):
    from diffuman4d_amd.host import pose
    root, images, masks = scene
    g = hip_device.index or 0

    def predict(out, **kw):
        return pose.predict_keypoints(str(root / "images"), str(tmp_path / out), str(root / "fmasks"), pose_model=stub_model, shape=POSE_SHAPE,
                                      batch_size=3, num_workers=2, **kw)
    assert predict("det", gpu_ids=[g], bbox_source="detector", person_detector=stand_in_detector, det_shape=DET_SHAPE, det_cat_id=1) == \
        {"images": 6, "written": 6, "skipped": 0}
    assert predict("whole", gpu_ids=[g]) == {"images": 6, "written": 6, "skipped": 0}
    det, whole = files_of(tmp_path / "det"), files_of(tmp_path / "whole")
    paths, _ = pose.list_inputs(str(root / "images"), None)
    boxes, scores = planted()
    for k, p in enumerate(paths):
        name = pose.output_path("", p).lstrip("/")
        info = json.loads(det[name])["instance_info"]
        counts, out, _ = M.select(boxes[k % 3], scores[k % 3], M.inv_scale(*E2E_SIZES[k], DET_SHAPE), 1)
        assert counts[0] == [0, 1, 3][k % 3] and len(info) == max(counts[0], 1)
        if counts[0] == 0:
            assert det[name] == whole[name]  # no kept box: the whole image, as the whole-image route writes it
            continue
        x, centers, scales = pose.pose_inputs([images[k]], [masks[k]], [list(out[:counts[0], :4])], POSE_SHAPE, hip_device)
        kp, sc = pose.decode_heatmaps(stub_model(x), POSE_SHAPE[::-1], centers, scales)
        assert [i["keypoints"] for i in info] == kp.tolist() and [i["keypoint_scores"] for i in info] == sc.tolist()
    # two workers: the same files
    assert predict("det2", gpu_ids=[g, g], bbox_source="detector", person_detector=stand_in_detector, det_shape=DET_SHAPE, det_cat_id=1)["written"] == 6
    assert files_of(tmp_path / "det2") == det
    # a second pass writes nothing
    assert predict("det2", gpu_ids=[g], bbox_source="detector", person_detector=stand_in_detector, det_shape=DET_SHAPE, det_cat_id=1) == \
        {"images": 6, "written": 0, "skipped": 6}


@pytest.mark.parametrize("source", ["image", "fmask"])
def test_the_other_box_sources_write_what_they_wrote(hip_device, scene, tmp_path, source):
    """bbox_source "image" and "fmask" go the way they went before the detector route: the files are those of pose_inputs called
    directly, byte for byte."""
    from diffuman4d_amd.host import pose
    root, images, masks = scene
    res = pose.predict_keypoints(str(root / "images"), str(tmp_path / "got"), str(root / "fmasks"), pose_model=stub_model, shape=POSE_SHAPE,
                                 batch_size=4, gpu_ids=[hip_device.index or 0], num_workers=2, bbox_source=source)
    assert res == {"images": 6, "written": 6, "skipped": 0}
    paths, _ = pose.list_inputs(str(root / "images"), None)
    for k, p in enumerate(paths):
        x, centers, scales = pose.pose_inputs([images[k]], [masks[k]], None, POSE_SHAPE, hip_device, bbox_source=source)
        kp, sc = pose.decode_heatmaps(stub_model(x), POSE_SHAPE[::-1], centers, scales)
        pose.write_instances(pose.output_path(str(tmp_path / "want"), p), kp, sc)
    assert files_of(tmp_path / "got") == files_of(tmp_path / "want") and len(files_of(tmp_path / "got")) == 6
