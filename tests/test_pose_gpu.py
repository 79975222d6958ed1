"""GPU: the three dm4d_pose_* kernels and predict_keypoints against tests/pose_model.py.  The network input is compared bit for bit; the
decode's scores bit for bit and its locations against the float64 model, within 4 x the distance between the float32 and float64 models
on the same cases (with a floor of 2^-20 max(Hh, Wh) for cases on which the two agree exactly).  On an MI355X the device's distance to
the float64 model was at most 1.81e-6 heatmap pixel on the maps up to 64 x 48, the float32 model's 1.81e-6; on the wide maps (12 x 400,
14 x 1024) 2.29e-5, the float32 model's 2.29e-5 (profiles/pose_parity.log)."""
import functools
import json
import os
import threading

import numpy as np
import pytest
import torch
from PIL import Image

import pose_cases
import pose_model as M

pytestmark = pytest.mark.gpu

SHAPES = [(32, 24), (40, 28)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# -- network input ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sources():
    """Three images of different sizes (h, w) with their masks: all 0, all 255, a ramp."""
    rng = np.random.default_rng(7)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in [(7, 9), (37, 50), (64, 64)]]
    masks = [np.zeros((7, 9), dtype=np.uint8), np.full((37, 50), 255, dtype=np.uint8),
             np.tile(np.linspace(0, 255, 64).astype(np.uint8), (64, 1))]
    return images, masks


# per image: the boxes of its rows (None = the whole image)
BOXES = [
    [None, [3.2, 2.1, 4.9, 4.4]],                                         # equal to the image; strong enlargement
    [[4.3, 2.7, 41.6, 30.2], [-30.0, -20.0, 80.0, 57.0], [25.0, -18.5, 75.0, 18.5]],   # fractional corners; larger than the image; half outside
    [[-64.0, -64.0, 128.0, 128.0], [10.0, 12.0, 30.5, 40.25]],            # strong reduction (zero rim); a second box on one image
]


@functools.lru_cache(maxsize=None)
def input_reference(shape, masked):
    images, masks = sources()
    rows = []
    for k, image in enumerate(images):
        for box in BOXES[k]:
            rows.append(M.pose_input(image, masks[k] if masked else None, box, shape))
    return rows


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("masked", [True, False])
def test_input_is_bit_equal_to_the_model_alone_and_in_a_batch(hip_device, shape, masked):
    from diffuman4d_amd.host import pose
    images, masks = sources()
    want = input_reference(shape, masked)
    x, centers, scales = pose.pose_inputs(images, masks if masked else None, BOXES, shape, hip_device)
    assert x.shape == (len(want), 3) + shape and x.dtype == torch.float32
    got = x.cpu().numpy()
    for r, (ref, c, s) in enumerate(want):
        assert np.array_equal(bits(got[r]), bits(ref)), f"row {r}: {np.count_nonzero(bits(got[r]) != bits(ref))} values differ"
        assert np.array_equal(centers[r], c) and np.array_equal(scales[r], s)
    r0 = 0
    for k in range(3):  # each image alone: the same bits as in the mixed batch
        alone, _, _ = pose.pose_inputs([images[k]], [masks[k]] if masked else None, [BOXES[k]], shape, hip_device)
        assert np.array_equal(bits(alone.cpu().numpy()), bits(got[r0: r0 + len(BOXES[k])]))
        r0 += len(BOXES[k])


def test_input_from_files_and_mixed_masks(hip_device, tmp_path):
    """PNG / WebP-lossless files decode to the arrays they were made from; an image without a mask may sit beside one with a mask; a
    mode-1 mask is its L conversion."""
    from diffuman4d_amd.host import pose
    images, masks = sources()
    paths = []
    for k, a in enumerate(images):
        paths.append(str(tmp_path / f"{k}.png"))
        Image.fromarray(a).save(paths[-1])
    one = Image.fromarray(masks[2] >= 128)
    x, _, _ = pose.pose_inputs(paths, [None, Image.fromarray(masks[1]), one], None, (32, 24), hip_device)
    got = x.cpu().numpy()
    refs = [M.pose_input(images[0], None, None, (32, 24)), M.pose_input(images[1], masks[1], None, (32, 24)),
            M.pose_input(images[2], np.asarray(one.convert("L")), None, (32, 24))]
    for r, (ref, _, _) in enumerate(refs):
        assert np.array_equal(bits(got[r]), bits(ref))


# -- mask box --------------------------------------------------------------------------------------------------------------------------
def test_mask_box(hip_device):
    from diffuman4d_amd.host import pose
    masks = [np.zeros((7, 9), dtype=np.uint8), np.full((37, 50), 255, dtype=np.uint8)]
    for y, x in [(0, 0), (0, 49), (36, 0), (36, 49)]:  # a single pixel in each corner
        m = np.zeros((37, 50), dtype=np.uint8)
        m[y, x] = 128
        masks.append(m)
    m = np.full((64, 64), 127, dtype=np.uint8)  # 127 next to 128
    m[20, 33], m[41, 7] = 128, 255
    masks.append(m)
    rng = np.random.default_rng(3)
    big = np.zeros((301, 203), dtype=np.uint8)  # more than one 16-byte vector per thread, a head and a tail
    big[40:250, 31:170] = rng.integers(0, 256, (210, 139), dtype=np.uint8)
    big[40, 31], big[249, 169] = 200, 200
    masks.append(big)
    got = pose.fmask_boxes(masks, hip_device)
    assert got.dtype == np.int32 and got.tolist() == [M.mask_box(m) for m in masks]
    assert got[0].tolist() == [0, 0, 9, 7] and got[1].tolist() == [0, 0, 50, 37] and got[6].tolist() == [7, 20, 34, 42]
    assert np.array_equal(pose.fmask_boxes(masks[::-1], hip_device), got[::-1])
    x, c, s = pose.pose_inputs([np.zeros((64, 64, 3), dtype=np.uint8)], [m], None, (32, 24), hip_device, bbox_source="fmask")
    cm, sm = M.center_scale([7, 20, 34, 42], (32, 24))
    assert np.array_equal(c[0], cm) and np.array_equal(s[0], sm)


# -- decode ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def decode_reference(Hh, Wh, rows):
    maps = pose_cases.row_maps(Hh, Wh) if rows else pose_cases.case_maps(Hh, Wh)[1]
    l64, s64, conds = M.udp_decode(maps, np.float64, details=True)
    l32, _ = M.udp_decode(maps, np.float32)
    return maps, l64, s64, conds, float(np.abs(l32.astype(np.float64) - l64).max())


# 12 x 400 and 14 x 1024: maps so wide that the LDS holds fewer than 32 rows of them (one band of 12 rows; three bands of 5, 5 and 4 rows,
# fewer than the 8 outputs a thread takes per pass), the second at the widest map the entry point accepts
@pytest.mark.parametrize("Hh,Wh,rows", [(8, 6, False), (23, 17, False), (64, 48, False), (64, 48, True), (12, 400, True), (14, 1024, False),
                                        (14, 1024, True)])
def test_decode(hip_device, Hh, Wh, rows):
    from diffuman4d_amd.host import ops
    maps, l64, s64, conds, model_gap = decode_reference(Hh, Wh, rows)
    K = len(maps)
    assert conds.max() < 100  # every case, none left out
    assert not rows or K == Hh  # a peak in every row
    tol = max(4 * model_gap, 2.0 ** -20 * max(Hh, Wh))
    heat = torch.from_numpy(maps).to(hip_device)
    locs1, scores1 = ops.pose_udp_decode(heat[None].contiguous())
    locs3, scores3 = ops.pose_udp_decode(torch.stack([heat, heat.flip(0), heat]).contiguous())
    torch.cuda.synchronize()
    locs, scores = locs1.cpu().numpy()[0], scores1.cpu().numpy()[0]
    dist = np.abs(locs.astype(np.float64) - l64).max()
    print(f"decode {Hh} x {Wh} K {K}: device-fp64 model {dist:.3e}, fp32-fp64 model {model_gap:.3e}, tolerance {tol:.3e}, max cond {conds.max():.3f}")
    assert np.array_equal(bits(scores), bits(s64))
    assert dist <= tol
    assert np.array_equal(bits(locs3.cpu().numpy()[0]), bits(locs)) and np.array_equal(bits(locs3.cpu().numpy()[2]), bits(locs))
    assert np.array_equal(bits(locs3.cpu().numpy()[1]), bits(locs[::-1])) and np.array_equal(bits(scores3.cpu().numpy()[1]), bits(scores[::-1]))
    if not rows:
        names = pose_cases.case_maps(Hh, Wh)[0]
        at = dict(zip(names, locs))
        for k in ("constant_high", "constant_low"):
            assert at[k].tolist() == [0, 0]           # the step is exactly 0
        for k in ("zero", "negative"):
            assert at[k].tolist() == [-1, -1]         # not refined
        assert at["tie"][0] < Wh / 2 and at["tie"][1] < Hh / 2  # the first maximum wins


def test_decode_heatmaps_maps_to_image_pixels(hip_device):
    from diffuman4d_amd.host import pose
    names, maps = pose_cases.case_maps(23, 17)
    l64 = decode_reference(23, 17, False)[1]
    centers, scales = np.array([[30.5, 41.25], [10.0, 12.0]]), np.array([[51.0, 69.0], [17.0, 23.0]])
    heat = torch.from_numpy(np.stack([maps, maps])).to(hip_device)
    kp, sc = pose.decode_heatmaps(heat, (68, 92), centers, scales)
    assert kp.shape == (2, len(maps), 2) and kp.dtype == np.float64 and sc.dtype == np.float32
    tol = max(4 * decode_reference(23, 17, False)[4], 2.0 ** -20 * 23)
    for r in range(2):
        want = M.to_image(l64, (17, 23), (68, 92), centers[r], scales[r])
        assert np.abs(kp[r] - want).max() <= tol * (scales[r] / [16, 22]).max()


# -- end to end ------------------------------------------------------------------------------------------------------------------------
def stub_model(x):
    """4 x 4 average pool of the green plane, shifted positive."""
    return torch.nn.functional.avg_pool2d(x[:, 1:2], 4) + 3.0


def test_predict_keypoints_end_to_end(hip_device, tmp_path):
    from diffuman4d_amd.host import pose
    rng = np.random.default_rng(11)
    shape, images, masks = (64, 48), [], []
    for k, (h, w, cx, cy) in enumerate([(80, 60, 22.0, 51.0), (64, 48, 30.5, 20.25), (50, 70, 40.0, 12.0)]):
        ys, xs = np.mgrid[0:h, 0:w]
        blob = 200 * np.exp(-((xs - cx) ** 2 + (ys - cy) ** 2) / (2 * 6.0 ** 2))
        a = np.clip(blob[..., None] + rng.integers(0, 8, (h, w, 3)), 0, 255).astype(np.uint8)
        m = np.full((h, w), 255, dtype=np.uint8)
        m[:3] = 90
        images.append(a), masks.append(m)
        for d, arr in (("images", a), ("fmasks", m)):
            path = tmp_path / d / f"{k % 2:02d}" / (f"{k:06d}" + (".png" if d == "fmasks" else ".webp"))
            path.parent.mkdir(parents=True, exist_ok=True)
            Image.fromarray(arr).save(path, lossless=True) if d == "images" else Image.fromarray(arr).save(path)
    out = str(tmp_path / "poses_sapiens")
    res = pose.predict_keypoints(str(tmp_path / "images"), out, str(tmp_path / "fmasks"), pose_model=stub_model, shape=shape, batch_size=2,
                                 gpu_ids=[hip_device.index or 0], num_workers=2)
    assert res == {"images": 3, "written": 3, "skipped": 0}
    order = [0, 2, 1]  # sorted paths: 00/000000, 00/000002, 01/000001
    paths, _ = pose.list_inputs(str(tmp_path / "images"), None)
    stamps = {}
    for p, k in zip(paths, order):
        x, center, scale = M.pose_input(images[k], masks[k], None, shape)
        heat = stub_model(torch.from_numpy(x)[None]).numpy()[0]
        l64, s64 = M.udp_decode(heat, np.float64)
        l32, _ = M.udp_decode(heat, np.float32)
        tol = max(4 * np.abs(l32 - l64).max(), 2.0 ** -20 * 16) * (scale / [11, 15]).max()
        want = M.to_image(l64, (12, 16), (48, 64), center, scale)
        path = pose.output_path(out, p)
        info = json.load(open(path))["instance_info"]
        assert len(info) == 1 and np.abs(np.array(info[0]["keypoints"]) - want).max() <= tol
        assert np.allclose(np.array(info[0]["keypoint_scores"]), s64, rtol=1e-6, atol=0)  # the stub's own sums differ by ulps between CPU and device
        assert np.abs(np.array(info[0]["keypoints"])[0] - [[22.0, 51.0], [30.5, 20.25], [40.0, 12.0]][k]).max() < 6.0  # the blob itself, to the stub's coarseness
        stamps[path] = os.stat(path).st_mtime_ns
    res = pose.predict_keypoints(str(tmp_path / "images"), out, str(tmp_path / "fmasks"), pose_model=stub_model, shape=shape,
                                 gpu_ids=[hip_device.index or 0])
    assert res == {"images": 3, "written": 0, "skipped": 3}
    assert all(os.stat(p).st_mtime_ns == t for p, t in stamps.items())


def test_predict_keypoints_with_two_workers_equals_one(hip_device, tmp_path):
    """The stage driver (host/staging.py run_stage) with two worker threads on one device, one image per batch: the same files byte for
    byte as with one worker; skip_exists then writes nothing; a batch that fails in one worker reaches the caller and leaves no thread."""
    from diffuman4d_amd.host import pose, staging
    rng = np.random.default_rng(5)
    for k, (h, w) in enumerate([(5, 7), (16, 16), (33, 20)]):
        path = tmp_path / "images" / "00" / f"{k:06d}.webp"
        path.parent.mkdir(parents=True, exist_ok=True)
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(path, lossless=True)
    g = hip_device.index or 0

    def run(out, gpu_ids, skip_exists):
        return pose.predict_keypoints(str(tmp_path / "images"), str(tmp_path / out), pose_model=stub_model, shape=(64, 48), batch_size=1,
                                      gpu_ids=gpu_ids, num_workers=2, skip_exists=skip_exists)
    assert run("one", [g], False) == {"images": 3, "written": 3, "skipped": 0}
    assert run("two", [g, g], False) == {"images": 3, "written": 3, "skipped": 0}
    files = sorted(p.relative_to(tmp_path / "one") for p in (tmp_path / "one").rglob("*") if p.is_file())
    assert len(files) == 3 and files == sorted(p.relative_to(tmp_path / "two") for p in (tmp_path / "two").rglob("*") if p.is_file())
    for f in files:
        assert (tmp_path / "one" / f).read_bytes() == (tmp_path / "two" / f).read_bytes(), f
    assert run("two", [g, g], True) == {"images": 3, "written": 0, "skipped": 3}

    seen = []

    def process_batch(model, batch, dev, pool):
        seen.append((batch, dev, torch.cuda.current_stream(dev) != torch.cuda.default_stream(dev), torch.is_grad_enabled()))
        if batch == [1]:
            raise RuntimeError("batch 1 fails")
        return [pool.submit(len, batch)]
    with pytest.raises(RuntimeError, match="batch 1 fails"):
        staging.run_stage("a_stage", [g, g], 2, "dm4d-test-stage", [[0], [1], [2]], lambda dev: None, process_batch)
    assert sorted(s[0] for s in seen) == [[0], [1], [2]] and all(s[1:] == (torch.device("cuda", g), True, False) for s in seen)
    assert not [t.name for t in threading.enumerate() if t.name.startswith("dm4d-test-stage")]
