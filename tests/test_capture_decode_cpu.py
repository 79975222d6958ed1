"""CPU: the host side of SpaTemDataset(device_decode=True).  The numpy model of the two device steps (tests/capture_stats_model.py)
gives what capture.py takes from pixels on the host route -- mask_bbox, crop_box, skeleton_mask_rect, skeleton_mask, the 2 % decision;
the flag is validated and forwarded; files are probed, not decoded, with _open's mode errors; the checks run in label order on
stubbed statistics; and the whole route runs against the flag-off call with the device entries replaced by their models."""
import numpy as np
import pytest
import torch
from PIL import Image

import capture_model as cm
import capture_stats_model as sm
import kp2d_scene as ks
from diffuman4d_amd.host import capture, codec, skeleton
from diffuman4d_amd.host import lib as L


def random_planes(rng, channels, count=40):
    out = []
    for _ in range(count):
        h, w = (int(v) for v in rng.integers(1, 90, 2))
        p = np.zeros((h, w, 3) if channels == 3 else (h, w), np.uint8)
        for _ in range(int(rng.integers(0, 3))):
            y, x = int(rng.integers(h)), int(rng.integers(w))
            p[y: y + int(rng.integers(1, 30)), x: x + int(rng.integers(1, 30))] = rng.integers(0, 256, p[y: y + 1, x: x + 1].shape)
        out.append(p)
    return out


def test_the_model_gives_mask_bbox_and_crop_box():
    planes = [p for p in sm.edge_planes() if p.ndim == 2] + random_planes(np.random.default_rng(1), 1)
    empties = 0
    for p in planes:
        fc, fr, lc, lr, total = sm.plane_stats(p)
        assert total == int(p.astype(np.int64).sum())
        if lc < 0:
            empties += 1
            assert (fc, fr) == (p.shape[1], p.shape[0]) and capture.mask_bbox(p != 0) is None
            with pytest.raises(ValueError, match="foreground mask is empty"):
                capture.crop_box(p)
            continue
        box = (fc - 1, fr - 1, lc + 1, lr + 1)
        assert capture.mask_bbox(p != 0) == box
        assert capture.crop_box(p) == capture._crop_from_bbox(box, *p.shape)
    assert 2 <= empties < len(planes) // 2


def test_the_model_gives_skeleton_mask():
    rgb = [p for p in sm.edge_planes() if p.ndim == 3] + random_planes(np.random.default_rng(2), 3)
    rgb.append(np.zeros((100, 120, 3), np.uint8))
    rgb[-1][2, 1, 0] = rgb[-1][98, 118, 1] = 1  # the padded box is clamped at all four borders
    filled = 0
    for p in rgb:
        h, w = p.shape[:2]
        st = sm.plane_stats(p)
        if st[2] < 0:
            with pytest.raises(ValueError, match="skeleton is empty"):
                capture.skeleton_mask(p)
            continue
        rect = capture.skeleton_mask_rect(st[:4], h, w)
        want = capture.skeleton_mask(p)
        assert np.array_equal(sm.fill_rect(h, w, rect), want)
        c0, r0, c1, r1 = rect
        assert capture.crop_box(want) == capture._crop_from_bbox((c0 - 1, r0 - 1, c1, r1), h, w)
        filled += 1
    assert filled > 20 and sm.fill_rect(100, 120, capture.skeleton_mask_rect(sm.plane_stats(rgb[-1])[:4], 100, 120)).all()


def test_fill_rect_and_pack_planes():
    assert not sm.fill_rect(5, 7, (3, 1, 3, 4)).any() and not sm.fill_rect(5, 7, (0, 2, 7, 2)).any()
    assert sm.fill_rect(1, 1, (0, 0, 1, 1)).tolist() == [[255]]
    blob, desc = sm.pack_planes([np.full((3, 5), 1, np.uint8), np.full((2, 2, 3), 2, np.uint8)], guard=3)
    assert desc[:, :4].tolist() == [[16, 3, 5, 1], [48, 2, 2, 3]] and blob.size == 63
    assert (blob[:16] == 0xA5).all() and (blob[16:31] == 1).all() and (blob[31:48] == 0xA5).all() and (blob[48:60] == 2).all()


def test_the_two_percent_decision_from_the_sum():
    rng = np.random.default_rng(3)
    decided = undecided = 0
    for _ in range(300):
        h, w = (int(v) for v in rng.integers(20, 80, 2))
        m = np.zeros((h, w), np.uint8)
        k = int(rng.integers(0, h * w // 12))
        m.reshape(-1)[rng.permutation(h * w)[:k]] = rng.integers(1, 256, k) if rng.integers(2) else 255
        got = capture._sum_mean_at_most(sm.plane_stats(m)[4], m.size, 0.02)
        exact = m.astype(np.float64).sum() / (255.0 * m.size)
        if abs(exact - 0.02) > 1e-4:
            assert got is capture._mask_mean_at_most(m, 0.02) is bool(exact <= 0.02)
            decided += 1
        else:
            assert got is None
            undecided += 1
    assert decided > 200
    m = np.zeros((100, 100), np.uint8)  # exactly 2 %: inside the band, the float32 mean decides
    m.reshape(-1)[:200] = 255
    assert capture._sum_mean_at_most(200 * 255, 10000, 0.02) is None and isinstance(capture._mask_mean_at_most(m, 0.02), bool)
    assert capture._sum_mean_at_most(0, 10000, 0.02) is True and capture._sum_mean_at_most(255 * 10000, 10000, 0.02) is False


# -- the flag -----------------------------------------------------------------------------------------------------------------------
def test_the_flag_needs_a_hip_device(tmp_path):
    with pytest.raises(L.Dm4dError, match=r"SpaTemDataset\(device_decode=True\).*not a HIP device"):
        capture.SpaTemDataset(str(tmp_path), device="cpu", device_decode=True)
    import inspect
    names = list(inspect.signature(capture.SpaTemDataset.__init__).parameters)
    assert names[-2:] == ["palette", "device_decode"]
    assert inspect.signature(capture.SpaTemDataset.__init__).parameters["device_decode"].default is False


def test_the_data_config_forwards_the_flag(monkeypatch):
    from diffuman4d_amd.host import config
    assert config.NATIVE_DATASET_KEYS["device_decode"] is False
    seen = []
    monkeypatch.setattr(capture._l, "hip_device", lambda device, what: seen.append((device, what)))
    base = ["exp=demo_3d", f"data.data_dir={ks.GOLDEN / 'triang_scene'}", f"data.scene_label={ks.SCENE}", "data.height=64", "data.width=64"]
    cfg = config.compose(base + ["data.device_decode=true"])
    assert cfg["data"]["device_decode"] is True
    ds = config.instantiate(cfg["data"])
    assert type(ds) is capture.SpaTemDataset and ds.device_decode is True and seen == [("cuda", "SpaTemDataset(device_decode=True)")]
    assert ds.decode_stats == {"device": 0, "pillow": 0, "bytes_uploaded": 0}
    off = capture.SpaTemDataset(str(ks.GOLDEN / "triang_scene"), scene_label=ks.SCENE)
    assert off.device_decode is False and len(seen) == 1


def test_the_pose_stage_and_the_tools_take_the_flag(monkeypatch, tmp_path):
    import importlib.util
    import inspect
    from pathlib import Path
    from diffuman4d_amd.host import pose
    for fn in (pose.pose_inputs, pose.fmask_boxes, pose.predict_keypoints):
        p = inspect.signature(fn).parameters["device_decode"]
        assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
    tools = Path(__file__).resolve().parent.parent / "tools"
    spec = importlib.util.spec_from_file_location("preprocess_tool", tools / "preprocess.py")
    preprocess = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(preprocess)
    calls = []
    monkeypatch.setitem(preprocess.STAGES, "predict_keypoints", lambda *a, **kw: calls.append(kw) or {})
    preprocess.run(str(tmp_path), ["predict_keypoints"], sapiens_ckpt_path="ckpt")
    preprocess.run(str(tmp_path), ["predict_keypoints"], sapiens_ckpt_path="ckpt", device_decode=True)
    assert calls == [{}, {"device_decode": True}]
    spec = importlib.util.spec_from_file_location("predict_keypoints_tool", tools / "predict_keypoints.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    seen = []
    monkeypatch.setattr(pose, "predict_keypoints", lambda *a, **kw: seen.append(kw) or {})
    argv = ["--images_dir", "i", "--out_kp2d_dir", "o", "--sapiens_ckpt_path", "c"]
    assert tool.main(argv) == 0 and tool.main(argv + ["--device_decode"]) == 0
    assert "device_decode" not in seen[0] and seen[1]["device_decode"] is True


# -- files are probed, not decoded --------------------------------------------------------------------------------------------------
def test_read_probes_files_and_keeps_opens_errors(tmp_path):
    rng = np.random.default_rng(4)
    rgb = rng.integers(0, 256, (24, 40, 3), dtype=np.uint8)
    Image.fromarray(rgb).save(tmp_path / "a.jpg")
    Image.fromarray(rgb).save(tmp_path / "p.jpg", progressive=True)
    Image.fromarray(rgb).save(tmp_path / "a.png")
    Image.fromarray(rgb[..., 0]).save(tmp_path / "g.jpg")
    Image.fromarray(rgb[..., 0]).save(tmp_path / "m.png")
    Image.fromarray(np.dstack([rgb, rgb[..., :1]])).save(tmp_path / "rgba.png")
    Image.fromarray(rgb).save(tmp_path / "a.webp", lossless=True)
    for name, mode in (("a.jpg", "RGB"), ("a.png", "RGB"), ("m.png", "L"), ("g.jpg", "L")):
        f = capture._read(str(tmp_path / name), mode)
        assert isinstance(f, codec.StagedFile) and (f.h, f.w, f.mode) == (24, 40, mode) and capture._hw(f) == (24, 40)
        assert f.nbytes == 24 * 40 * (3 if mode == "RGB" else 1) and f.path == str(tmp_path / name)
    for name in ("p.jpg", "a.webp"):  # the probes refuse them: Pillow's pixels, as ever
        a = capture._read(str(tmp_path / name), "RGB")
        assert isinstance(a, np.ndarray) and np.array_equal(a, capture._open(str(tmp_path / name), "RGB")) and capture._hw(a) == (24, 40)
    for name, mode in (("g.jpg", "RGB"), ("rgba.png", "RGB"), ("a.png", "L"), ("a.webp", "L")):
        with pytest.raises(ValueError) as want:
            capture._open(str(tmp_path / name), mode)
        with pytest.raises(ValueError) as got:
            capture._read(str(tmp_path / name), mode)
        assert str(got.value) == str(want.value) and "no conversion is made" in str(got.value)
    with pytest.raises(FileNotFoundError) as want:
        capture._open(str(tmp_path / "absent.png"), "L")
    with pytest.raises(FileNotFoundError) as got:
        capture._read(str(tmp_path / "absent.png"), "L")
    assert str(got.value) == str(want.value)


# -- the checks, in label order, on stubbed statistics ----------------------------------------------------------------------------------
def frame(h=50, w=40, target=False, check=True, mask=None):
    img = np.zeros((h, w, 3), np.uint8)
    return {"img": None if target else img, "mask": None if target else (np.zeros((h, w), np.uint8) if mask is None else mask),
            "skel": img, "plan": None, "crop": None, "check": check and not target, "hw": (h, w), "path": "skel.png", "img_path": "img.png"}


GOOD = [10, 5, 29, 44, 255 * 20 * 40]   # 40 % of a 50 x 40 mask
EMPTY = [40, 50, -1, -1, 0]


def test_settle_frame_gives_the_host_routes_crop_and_errors():
    m = np.zeros((50, 40), np.uint8)
    m[5:45, 10:30] = 255
    fr = frame(mask=m)
    capture._settle_frame(fr, sm.plane_stats(m))
    assert sm.plane_stats(m) == GOOD and fr["crop"] == capture.crop_box(m)
    s = np.zeros((50, 40, 3), np.uint8)
    s[20:30, 15:22, 1] = 200
    fr = frame(target=True)
    capture._settle_frame(fr, sm.plane_stats(s))
    assert fr["crop"] == capture.crop_box(capture.skeleton_mask(s)) and np.array_equal(sm.fill_rect(50, 40, fr["rect"]), capture.skeleton_mask(s))
    with pytest.raises(ValueError, match="^foreground mask is empty: img.png$"):
        capture._settle_frame(frame(), EMPTY)
    with pytest.raises(ValueError, match="^skeleton is empty, no mask can be made from it: skel.png$"):
        capture._settle_frame(frame(target=True), EMPTY)
    fr = frame()
    fr["hw"] = (50, 39)
    with pytest.raises(AssertionError, match=r"^Error: image size: \(40, 50\) != fmask size: \(40, 50\) != skeleton size: \(39, 50\)$"):
        capture._settle_frame(fr, GOOD)
    small = [0, 0, 3, 3, 255 * 16]  # 0.8 %
    with pytest.raises(AssertionError, match="^Error: foreground mask < 2%. Please check the data.$"):
        capture._settle_frame(frame(), small)
    capture._settle_frame(frame(check=False), small)  # a frame that is no input is not checked
    # the empty check comes before the size check, the size check before the 2 % check
    fr = frame()
    fr["hw"] = (50, 39)
    with pytest.raises(ValueError, match="foreground mask is empty"):
        capture._settle_frame(fr, EMPTY)
    with pytest.raises(AssertionError, match="image size"):
        capture._settle_frame(fr, small)


def test_the_band_of_the_two_percent_check_decodes_the_mask_on_the_host(monkeypatch):
    m = np.zeros((100, 100), np.uint8)
    m.reshape(-1)[:200] = 255  # exactly 2 %
    asked = []
    real = capture._mask_mean_at_most
    monkeypatch.setattr(capture, "_mask_mean_at_most", lambda mask, limit: asked.append(mask) or real(mask, limit))
    fr = frame(100, 100, mask=m)
    try:
        capture._settle_frame(fr, sm.plane_stats(m))
        raised = False
    except AssertionError:
        raised = True
    assert len(asked) == 1 and asked[0] is m and raised is real(m, 0.02)
    capture._settle_frame(frame(), GOOD)  # far from the limit: the sum decides
    assert len(asked) == 1


def test_the_first_bad_frame_in_label_order_is_raised():
    rows = {0: GOOD, 1: EMPTY, 2: [0, 0, 3, 3, 255 * 16], 3: GOOD}
    frames = [frame(), frame(), frame(), frame()]
    with pytest.raises(ValueError, match="foreground mask is empty"):
        capture._settle_frames(frames, rows)
    assert frames[0]["crop"] is not None and frames[2]["crop"] is None  # the walk stopped at frame 1
    with pytest.raises(AssertionError, match="foreground mask < 2%"):
        capture._settle_frames([frame(), frame(), frame()], {0: GOOD, 1: rows[2], 2: EMPTY})
    # a frame whose files could not be read waits for its turn: an earlier frame's error wins, a later frame's does not
    unread = ValueError("x.jpg: image mode 'L', expected 'RGB' (no conversion is made: it would change values)")
    with pytest.raises(ValueError, match="foreground mask is empty"):
        capture._settle_frames([frame(), frame(), unread], {0: GOOD, 1: EMPTY})
    with pytest.raises(ValueError, match="image mode 'L'"):
        capture._settle_frames([frame(), unread, frame()], {0: GOOD, 2: EMPTY})
    done = [frame(), frame(target=True)]
    capture._settle_frames(done, {0: GOOD, 1: [15, 20, 21, 29, 0]})
    assert all(fr["crop"] is not None for fr in done)


# -- the whole route, the device entries replaced by their models -------------------------------------------------------------------
PALETTE = skeleton.load_palette(ks.PALETTE_PATH)
HW = ks.SIZES[0]
KP2D = {"skeleton_source": "kp2d", "palette": PALETTE}


@pytest.fixture(scope="module")
def scene_root(tmp_path_factory):
    root = tmp_path_factory.mktemp("decode_cpu")
    scene = ks.write_cameras_and_detections(root, HW)
    ks.detections_as_poses_2d(scene)
    ks.write_images_and_masks(scene, HW)
    ks.write_skeleton_pngs(scene, HW, PALETTE, ks.model_draw)
    for p in sorted((scene / "images").rglob("*.png")):
        q = scene / "jpg" / p.parent.name / (p.stem + ".jpg")
        q.parent.mkdir(parents=True, exist_ok=True)
        Image.open(p).save(q, quality=92)
    return root


@pytest.fixture
def standins(monkeypatch):
    """The device entries as numpy models over the same staging buffer -> the log of what they were asked."""
    log = {"stats": [], "rects": [], "decoded": [], "refuse": set()}

    def crop_resize(blob, blob_host, n_frames, desc_off, tab_off, tab_len, H, W, meta=None):
        if meta is None:
            return cm.standin_crop_resize(blob, blob_host, n_frames, desc_off, tab_off, tab_len, H, W)
        both = torch.cat([blob, blob_host])
        return cm.standin_crop_resize(both, both, n_frames, blob.numel() + desc_off, blob.numel() + tab_off, tab_len, H, W)

    def rows(meta_host, n, desc_off, fields=8):
        return meta_host.numpy()[desc_off: desc_off + n * fields * 8].view(np.int64).reshape(n, fields)

    def plane_stats(blob, meta, meta_host, n, desc_off):
        out = []
        for off, h, w, ch in rows(meta_host, n, desc_off)[:, :4].tolist():
            assert off % 16 == 0
            out.append(sm.plane_stats(blob.numpy()[off: off + h * w * ch].reshape((h, w) if ch == 1 else (h, w, ch))))
        log["stats"].append(n)
        return torch.tensor(out, dtype=torch.int64)

    def fill_rects(blob, meta, meta_host, n, desc_off):
        for off, h, w, c0, r0, c1, r1 in rows(meta_host, n, desc_off)[:, :7].tolist():
            blob.numpy()[off: off + h * w] = sm.fill_rect(h, w, (c0, r0, c1, r1)).reshape(-1)
        log["rects"].append(n)

    def decode_staged(entries, buf, fallback, stats=None):
        for off, f, ch in entries:
            refused = f.path in log["refuse"]
            px = np.asarray(fallback(f) if refused else Image.open(f.path)).reshape(-1)
            assert ch == f.plan.bytes_per_pixel and px.size == f.nbytes and off % 16 == 0
            buf.numpy()[off: off + px.size] = px
            stats["pillow" if refused else "device"] += 1
            stats["bytes_uploaded"] += f.plan.payload_len + (px.size if refused else 0)
            log["decoded"].append(f.path)

    monkeypatch.setattr(capture.ops, "capture_crop_resize", crop_resize)
    monkeypatch.setattr(capture.ops, "skeleton_draw", ks.standin_skeleton_draw)
    monkeypatch.setattr(capture.ops, "skeleton_box_mask", ks.standin_box_mask)
    monkeypatch.setattr(capture.ops, "capture_plane_stats", plane_stats)
    monkeypatch.setattr(capture.ops, "capture_fill_rects", fill_rects)
    monkeypatch.setattr(capture, "decode_staged", decode_staged)
    monkeypatch.setattr(capture._l, "hip_device", lambda device, what: None)
    return log


def dataset(root, images="jpg", **kw):
    ext = ".jpg" if images == "jpg" else ".png"
    pats = {"image_path_pat": "{data_dir}/{scene_label}/" + images + "/{spa_label}/{tem_label}" + ext,
            "skeleton_path_pat": ks.patterns()["skeleton_path_pat"]}
    return capture.SpaTemDataset(data_dir=str(root), scene_label=ks.SCENE, device="cpu", decode_threads=4, height=64, width=64, **{**pats, **kw})


def same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]) if isinstance(a[k], torch.Tensor) else a[k] == b[k], k


@pytest.mark.parametrize("source", [{}, KP2D])
@pytest.mark.parametrize("has_gt_target", [True, False])
@pytest.mark.parametrize("task", ["spatial", "temporal"])
def test_the_route_on_stand_ins_equals_the_flag_off_call(scene_root, standins, task, has_gt_target, source):
    spa, tem = ks.TASKS[task]
    want = dataset(scene_root, has_gt_target=has_gt_target, **source).get_item(ks.SCENE, spa, tem, ks.INPUTS)
    on = dataset(scene_root, has_gt_target=has_gt_target, device_decode=True, **source)
    same(on.get_item(ks.SCENE, spa, tem, ks.INPUTS), want)
    full = sum(1 for _, s, _ in want["labels"] if has_gt_target or s in ks.INPUTS)
    targets = len(want["labels"]) - full
    files = 2 * full + (0 if source else len(want["labels"]))
    assert on.decode_stats["device"] == files == len(standins["decoded"]) and on.decode_stats["pillow"] == 0
    assert standins["stats"] == ([full + (0 if source else targets)] if full or not source else [])  # one launch over masks and target maps
    assert standins["rects"] == ([targets] if targets and not source else [])                          # one launch, the files route only


def test_refused_and_unprobed_files_on_stand_ins(scene_root, standins):
    spa, tem = ks.TASKS["spatial"]
    want = dataset(scene_root, images="images").get_item(ks.SCENE, spa, tem, ks.INPUTS)  # PNG images
    scene = scene_root / ks.SCENE
    standins["refuse"] = {str(scene / "images" / "02" / "000000.png"), str(scene / "fmasks" / "05" / "000000.png")}
    on = dataset(scene_root, images="images", device_decode=True)
    same(on.get_item(ks.SCENE, spa, tem, ks.INPUTS), want)
    assert on.decode_stats["device"] == 22 and on.decode_stats["pillow"] == 2


def test_errors_in_label_order_on_stand_ins(scene_root, standins, tmp_path):
    import shutil
    shutil.copytree(scene_root / ks.SCENE, tmp_path / ks.SCENE)
    d = tmp_path / ks.SCENE
    h, w = HW
    Image.fromarray(np.zeros((h, w), np.uint8)).save(d / "fmasks" / "02" / "000000.png")
    Image.fromarray(np.zeros((h, w), np.uint8) + 90).save(d / "jpg" / "04" / "000000.jpg")
    spa, tem = ks.TASKS["spatial"]
    for source in ({}, KP2D):
        texts = []
        for flag in (False, True):
            with pytest.raises(ValueError) as e:
                dataset(tmp_path, device_decode=flag, **source).get_item(ks.SCENE, spa, tem, ks.INPUTS)
            texts.append(str(e.value))
        assert texts[0] == texts[1] and texts[0].startswith("foreground mask is empty: ")
    shutil.copyfile(d / "fmasks" / "03" / "000000.png", d / "fmasks" / "02" / "000000.png")
    for source in ({}, KP2D):
        texts = []
        for flag in (False, True):
            with pytest.raises(ValueError) as e:
                dataset(tmp_path, device_decode=flag, **source).get_item(ks.SCENE, spa, tem, ks.INPUTS)
            texts.append(str(e.value))
        assert texts[0] == texts[1] and "jpg/04/000000.jpg: image mode 'L', expected 'RGB'" in texts[0]
