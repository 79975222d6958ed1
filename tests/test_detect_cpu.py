"""CPU: tests/detect_model.py, the numpy definition of the person-box stage, against what it restates, and the host side of
diffuman4d_amd/host/detect.py against the model.

The NMS fixtures tests/golden/detect_nms_*.npz hold ``dets`` float32 [k, 5], ``thr`` and ``keep``: the indices that the reference's own
``pose_utils.py::nms`` returned for them.  They were made once by cutting that function (pure numpy) out of its module with ``ast`` and
calling it, so that nothing else of the module (it imports cv2) was needed; only the arrays are kept.  No two scores of a fixture are
equal: the reference's order among equal scores is ``argsort``'s and is not part of the definition.

The resize rule against an independent fp64 bilinear at the same sampling positions, over the image sizes and canvases below that
fit (mmcv's keep-ratio rule looks at the longer and the shorter side only, so a landscape image does not fit a portrait canvas and
the other way round: 263 x 301 into 96 x 64 and 37 x 23, 64 x 48, 301 x 263 into 64 x 96 are refused with a ValueError, which is
asserted): the largest difference measured here is 1 grey level, on 11.26 % of the 100032 bytes (0 % at scale 1, 11.99 % to 13.30 %
per case otherwise: the price of 11-bit weights and of shifts that truncate); asserted: at most 1 level, on fewer than 22.52 % of all
bytes."""
import glob
import os

import numpy as np
import pytest

import detect_model as M

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
SIZES = [(37, 23), (64, 48), (301, 263), (263, 301)]  # (h, w)
CANVASES = [(64, 64), (96, 64), (64, 96)]             # (H, W)
MEASURED_SHARE = 0.1126


def gradient_noise(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    base = np.stack([xx * 255.0 / max(w - 1, 1), yy * 255.0 / max(h - 1, 1), (xx + yy) * 255.0 / max(h + w - 2, 1)], -1)
    return np.clip(base + rng.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)


# -- NMS -------------------------------------------------------------------------------------------------------------------------------
def test_fixture_set_is_the_one_the_definition_asks_for():
    names = sorted(os.path.basename(p)[len("detect_nms_"):-4] for p in glob.glob(os.path.join(GOLDEN, "detect_nms_*.npz")))
    assert names == sorted(["empty", "one", "two_overlap", "two_apart", "n37", "n100", "nested", "identical", "disjoint", "touching", "ovr_equals_thr"])
    sizes = {n: len(np.load(os.path.join(GOLDEN, f"detect_nms_{n}.npz"))["dets"]) for n in names}
    assert (sizes["empty"], sizes["one"], sizes["two_overlap"], sizes["two_apart"], sizes["n37"], sizes["n100"]) == (0, 1, 2, 2, 37, 100)
    d = np.load(os.path.join(GOLDEN, "detect_nms_ovr_equals_thr.npz"))["dets"]
    f = np.float32
    area = lambda b: f(f(f(b[2] - b[0]) + f(1)) * f(f(b[3] - b[1]) + f(1)))
    inter = f(f(f(min(d[0][2], d[1][2]) - max(d[0][0], d[1][0])) + f(1)) * f(f(min(d[0][3], d[1][3]) - max(d[0][1], d[1][1])) + f(1)))
    assert f(inter / f(f(area(d[0]) + area(d[1])) - inter)) == f(0.3)  # the pair that sits on the threshold


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "detect_nms_*.npz"))), ids=lambda p: os.path.basename(p)[11:-4])
def test_nms_keeps_what_the_reference_kept(path):
    z = np.load(path)
    dets, thr, want = z["dets"], float(z["thr"]), z["keep"].tolist()
    assert dets.dtype == np.float32 and dets.shape[1:] == (5,) and len(set(dets[:, 4].tolist())) == len(dets)
    order = np.argsort(-dets[:, 4].astype(np.float64), kind="stable")
    got = [int(order[k]) for k in M.nms(dets[order], thr)]
    assert got == want  # equal, not close
    # the whole selection on the same boxes (identity scale, every score above the threshold, no cap in the way)
    counts, out, idx = M.select(dets[:, :4], dets[:, 4:5], (np.float32(1), np.float32(1)), 0, 0.3, thr, 128)
    assert idx[:counts[0]].tolist() == want and counts == [len(want), 0, len(dets)]
    assert np.array_equal(out[:counts[0]], dets[want].reshape(-1, 5)) and not out[counts[0]:].any() and (idx[counts[0]:] == -1).all()


# -- selection -------------------------------------------------------------------------------------------------------------------------
def apart(A):
    """A boxes of 8 x 8 pixels, 20 apart: none overlaps another."""
    k = np.arange(A)
    x, y = (k % 64) * 20.0, (k // 64) * 20.0
    return np.stack([x, y, x + 8, y + 8], 1).astype(np.float32)


ONE = (np.float32(1), np.float32(1))


@pytest.mark.parametrize("seed,A", [(0, 300), (1, 1000), (2, 1000), (3, 60)])
def test_top_k_then_threshold_equals_threshold_then_top_k(seed, A):
    """The reference keeps the best 100 of the scores above 0.05 and then asks for > 0.3; the definition asks for > 0.3 and keeps the
    best 100."""
    rng = np.random.default_rng(seed)
    s = (rng.random(A) ** (0.5 if seed == 2 else 2)).astype(np.float32)
    s = np.unique(s)[rng.permutation(len(np.unique(s)))]  # no ties: the reference's tie order is not defined
    A = len(s)
    first = [a for a in sorted(np.nonzero(s > np.float32(0.05))[0], key=lambda a: -s[a])[:100] if s[a] > np.float32(0.3)]
    counts, out, idx = M.select(apart(A), s[:, None], ONE, 0, 0.3, 0.3, 100)
    assert idx[:counts[0]].tolist() == first and counts[0] == len(first) == min(100, int((s > np.float32(0.3)).sum()))
    assert counts[2] == int((s > np.float32(0.3)).sum())


def test_ties_go_by_anchor_index_and_the_cap_holds():
    s = np.full(300, 0.5, dtype=np.float32)
    s[[7, 250]] = 0.9
    s[[3, 100]] = 0.25  # below
    counts, out, idx = M.select(apart(300), s[:, None], ONE, 0, 0.3, 0.3, 100)
    rest = [a for a in range(300) if a not in (7, 250, 3, 100)]
    assert counts == [100, 0, 298] and idx.tolist() == [7, 250] + rest[:98]
    counts, out, idx = M.select(apart(300), s[:, None], ONE, 0, 0.3, 0.3, 1)
    assert counts == [1, 0, 298] and idx.tolist() == [7]
    # the threshold is strict, in float32
    s2 = np.array([0.3, np.nextafter(np.float32(0.3), np.float32(1)), 0.29999], dtype=np.float32)
    counts, _, idx = M.select(apart(3), s2[:, None], ONE, 0, 0.3, 0.3, 100)
    assert counts == [1, 0, 1] and idx[0] == 1
    # the class column
    sc = np.zeros((3, 3), dtype=np.float32)
    sc[1, 2], sc[0, 0] = 0.8, 0.9
    assert M.select(apart(3), sc, ONE, 2)[2][:2].tolist() == [1, -1] and M.select(apart(3), sc, ONE, 0)[2][:2].tolist() == [0, -1]


def test_nan_scores_never_pass_and_bad_boxes_are_dropped_and_counted():
    boxes = apart(8)
    s = np.array([0.9, np.nan, 0.8, 0.7, 0.6, 0.5, 0.4, 0.2], dtype=np.float32)
    boxes[2] = [5, 5, 5, 9]            # x2 == x1
    boxes[3] = [5, 9, 9, 5]            # y2 < y1
    boxes[4] = [0, 0, np.inf, 4]       # not finite
    boxes[5] = [0, 0, np.nan, 4]
    boxes[6] = [0, 0, 3e38, 4]         # finite, but not after the scaling by 2
    counts, out, idx = M.select(boxes, s[:, None], (np.float32(2), np.float32(2)), 0, 0.3, 0.3, 100)
    assert counts == [1, 5, 6] and idx[:2].tolist() == [0, -1]
    assert np.array_equal(out[0], np.array([0, 0, 16, 16, 0.9], dtype=np.float32))
    counts, _, _ = M.select(boxes, np.full((8, 1), np.nan, dtype=np.float32), ONE)
    assert counts == [0, 0, 0]


def test_the_scale_is_one_float32_multiply():
    inv = M.inv_scale(2048, 2448, (640, 640))
    assert inv[0].dtype == np.float32 and inv == (np.float32(1.0 / (640 / 2448)), np.float32(1.0 / (535 / 2048)))
    b = np.array([[10.3, 20.7, 300.1, 500.9]], dtype=np.float32)
    _, out, _ = M.select(b, np.ones((1, 1), np.float32), inv)
    assert np.array_equal(out[0, :4], np.array([b[0, 0] * inv[0], b[0, 1] * inv[1], b[0, 2] * inv[0], b[0, 3] * inv[1]], dtype=np.float32))


# -- resize ----------------------------------------------------------------------------------------------------------------------------
def bilinear64(image, nw, nh):
    """An independent fp64 bilinear at (d + 0.5) * scale - 0.5, edge clamped, rounded half up."""
    h, w = image.shape[:2]
    fx = np.clip((np.arange(nw) + 0.5) * (w / nw) - 0.5, 0, w - 1)
    fy = np.clip((np.arange(nh) + 0.5) * (h / nh) - 0.5, 0, h - 1)
    x0, y0 = np.minimum(np.floor(fx).astype(int), w - 1), np.minimum(np.floor(fy).astype(int), h - 1)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    ax, ay = (fx - x0)[None, :, None], (fy - y0)[:, None, None]
    p = image.astype(np.float64)
    top = p[y0][:, x0] * (1 - ax) + p[y0][:, x1] * ax
    bot = p[y1][:, x0] * (1 - ax) + p[y1][:, x1] * ax
    return np.floor(top * (1 - ay) + bot * ay + 0.5).astype(np.int64)


def test_resize_is_the_identity_at_scale_one_and_exact_on_constants():
    img = gradient_noise(48, 64, 1)
    assert np.array_equal(M.resize(img, 64, 48), img)
    assert M.rescaled_size(48, 64, (64, 64)) == (64, 48) and np.array_equal(M.canvas_bytes(img, None, (64, 64))[:48], img)
    for v in (0, 1, 114, 127, 254, 255):
        for (h, w), (nw, nh) in (((37, 23), (40, 64)), ((301, 263), (56, 64)), ((5, 9), (64, 36))):
            assert (M.resize(np.full((h, w, 3), v, np.uint8), nw, nh) == v).all()


def test_resize_against_an_independent_bilinear():
    worst, differ, total, refused = 0, 0, 0, []
    from diffuman4d_amd.host import detect
    for (h, w) in SIZES:
        for shape in CANVASES:
            if not M.fits(h, w, shape):
                with pytest.raises(ValueError, match="does not fit"):
                    detect.detector_tables([(h, w)], shape)
                refused.append(((h, w), shape))
                continue
            nw, nh = M.rescaled_size(h, w, shape)
            img = gradient_noise(h, w, h * 1000 + w)
            d = np.abs(M.resize(img, nw, nh) - bilinear64(img, nw, nh))
            print(f"resize {w} x {h} -> {nw} x {nh} in {shape[1]} x {shape[0]}: max {d.max()}, differing {np.count_nonzero(d) / d.size:.4%}")
            worst, differ, total = max(worst, int(d.max())), differ + np.count_nonzero(d), total + d.size
    print(f"resize: max {worst}, differing {differ / total:.4%} of {total} bytes")
    assert refused == [((37, 23), (64, 96)), ((64, 48), (64, 96)), ((301, 263), (64, 96)), ((263, 301), (96, 64))]
    assert worst <= 1
    assert differ / total < 2 * MEASURED_SHARE


@pytest.mark.parametrize("size,shape,want", [((2048, 2448), (640, 640), (640, 535)), ((2448, 2048), (640, 640), (535, 640)),
                                              ((1024, 1024), (640, 640), (640, 640)), ((37, 23), (96, 64), (60, 96)),
                                              ((1, 5000), (640, 640), None), ((10, 10), (64, 96), (64, 64))])
def test_sizes_and_the_pad_region(size, shape, want):
    h, w = size
    from diffuman4d_amd.host import detect
    if want is None:  # a side that resizes to nothing
        with pytest.raises(ValueError, match="empty"):
            detect.detector_tables([size], shape)
        return
    assert M.rescaled_size(h, w, shape) == want
    tabs, nwnh, inv = detect.detector_tables([size], shape)
    assert nwnh.tolist() == [list(want)] and inv.dtype == np.float32 and tuple(inv[0]) == M.inv_scale(h, w, shape)
    if h * w <= 4096:
        img = gradient_noise(h, w, 3)
        mask = gradient_noise(h, w, 4)[..., 0]
        for m in (None, mask):
            v = M.canvas_bytes(img, m, shape)
            assert (v[want[1]:] == M.PAD_VALUE).all() and (v[:, want[0]:] == M.PAD_VALUE).all()
            x = M.detector_input(img, m, shape)
            pad = [(np.float32(114) - np.float32(M.MEAN[c])) / np.float32(M.STD[c]) for c in range(3)]
            assert x.dtype == np.float32 and x.shape == (3,) + shape and all((x[c, want[1]:] == pad[c]).all() for c in range(3))
            assert np.array_equal(M.detector_input(img, m, shape, channel_order="bgr", mean=M.MEAN[::-1], std=M.STD[::-1]), x[::-1])
        assert np.array_equal(M.canvas_bytes(img, np.full((h, w), 255, np.uint8), shape), M.canvas_bytes(img, None, shape))
        assert (M.canvas_bytes(img, np.zeros((h, w), np.uint8), shape)[:want[1], :want[0]] == 0).all()


@pytest.mark.parametrize("size", SIZES + [(2048, 2448), (5, 9), (1, 1)])
@pytest.mark.parametrize("shape", [(64, 64), (96, 64), (640, 640)])
def test_host_tables_are_the_models(size, shape):
    from diffuman4d_amd.host import detect
    if not M.fits(*size, shape):
        return
    (tab,), nwnh, _ = detect.detector_tables([size], shape)
    nw, nh = M.rescaled_size(*size, shape)
    xs, a0, a1 = M.axis(size[1], nw)
    ys, b0, b1 = M.axis(size[0], nh)
    assert tab.dtype == np.int32 and tab.size == 2 + 2 * (nw + nh) and tab[:2].tolist() == [nw, nh]
    assert np.array_equal(tab[2: 2 + nw], xs) and np.array_equal(tab[2 + nw: 2 + nw + nh], ys)
    coef = tab[2 + nw + nh:].view(np.uint32)
    assert np.array_equal(coef & 0xffff, np.concatenate([a0, b0])) and np.array_equal(coef >> 16, np.concatenate([a1, b1]))
    assert ((np.concatenate([a0, b0]) + np.concatenate([a1, b1])) == M.ONE).all()


# -- arguments -------------------------------------------------------------------------------------------------------------------------
def test_predict_keypoints_argument_errors(tmp_path):
    import torch
    from PIL import Image
    from diffuman4d_amd.host import detect, pose
    from diffuman4d_amd.host.lib import Dm4dError
    (tmp_path / "images" / "00").mkdir(parents=True)
    Image.fromarray(np.zeros((8, 6, 3), np.uint8)).save(tmp_path / "images" / "00" / "000000.jpg")
    images_dir, out = str(tmp_path / "images"), str(tmp_path / "kp")
    with pytest.raises(ValueError, match="bbox_source"):
        pose.predict_keypoints(images_dir, out, pose_model=lambda x: x, bbox_source="detector")
    with pytest.raises(ValueError, match="bbox_source"):
        pose.predict_keypoints(images_dir, out, pose_model=lambda x: x, bbox_source="boxes", person_detector=lambda x: x)
    with pytest.raises(NotImplementedError, match="mmdet") as e:
        pose.predict_keypoints(images_dir, out, pose_model=lambda x: x, detector_ckpt_path="rtmdet.pth", person_detector=lambda x: x)
    assert "person_detector" in str(e.value)
    if not torch.cuda.is_available():
        with pytest.raises(Dm4dError, match="no HIP device"):  # past every argument check
            pose.predict_keypoints(images_dir, out, pose_model=lambda x: x, bbox_source="detector", person_detector=lambda x: (x, x))
    with pytest.raises(FileNotFoundError, match="never downloaded"):
        detect.load_person_detector(str(tmp_path / "rtmdet.pt"), "cpu")
    with pytest.raises(Dm4dError, match="expected a tensor on a HIP device"):
        detect.select_boxes(torch.zeros(1, 4, 4), torch.zeros(1, 4, 1), {"sizes": [(8, 6)]})
    with pytest.raises(ValueError, match="channel_order"):
        detect.detector_inputs([np.zeros((8, 6, 3), np.uint8)], channel_order="gbr")
    with pytest.raises(ValueError, match="pad_value"):
        detect.detector_inputs([np.zeros((8, 6, 3), np.uint8)], pad_value=256)
    with pytest.raises(ValueError, match="does not fit"):  # before the device is asked for
        detect.detector_inputs([np.zeros((263, 301, 3), np.uint8)], shape=(96, 64))


def test_the_command_lines_hand_the_detector_flags_on(tmp_path, monkeypatch, capsys):
    import importlib.util
    from pathlib import Path
    from diffuman4d_amd.host import pose
    tools = Path(__file__).resolve().parent.parent / "tools"

    def load(name):
        spec = importlib.util.spec_from_file_location(name + "_tool", tools / (name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    seen = []
    monkeypatch.setattr(pose, "predict_keypoints", lambda *a, **kw: seen.append(kw) or {})
    tool = load("predict_keypoints")
    argv = ["--images_dir", "i", "--out_kp2d_dir", "o", "--sapiens_ckpt_path", "c"]
    assert tool.main(argv) == 0
    assert tool.main(argv + ["--person_detector", "det.pt", "--bbox_source", "detector", "--bbox_thr", "0.4", "--nms_thr", "0.5", "--det_shape", "320,480"]) == 0
    assert "person_detector" not in seen[0] and seen[0]["bbox_source"] == "image"
    assert {k: seen[1][k] for k in ("person_detector", "bbox_source", "bbox_thr", "nms_thr", "det_shape", "det_cat_id")} == \
        {"person_detector": "det.pt", "bbox_source": "detector", "bbox_thr": 0.4, "nms_thr": 0.5, "det_shape": (320, 480), "det_cat_id": 0}
    for bad in (["--bbox_source", "detector"], ["--person_detector", "det.pt"]):  # one without the other
        with pytest.raises(SystemExit):
            tool.main(argv + bad)
    capsys.readouterr()
    preprocess = load("preprocess")
    calls = []
    monkeypatch.setitem(preprocess.STAGES, "predict_keypoints", lambda *a, **kw: calls.append(kw) or {})
    (tmp_path / "scene").mkdir()
    base = ["--data_dir", str(tmp_path / "scene"), "--actions", "predict_keypoints", "--sapiens_ckpt_path", "c"]
    assert preprocess.main(base) == 0
    assert preprocess.main(base + ["--person_detector", "det.pt", "--bbox_source", "detector", "--nms_thr", "0.5", "--det_shape", "320,480"]) == 0
    assert calls == [{}, {"person_detector": "det.pt", "bbox_source": "detector", "nms_thr": 0.5, "det_shape": (320, 480)}]
    with pytest.raises(SystemExit):
        preprocess.main(base + ["--bbox_source", "detector"])
