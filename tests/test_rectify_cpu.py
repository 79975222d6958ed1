"""CPU: the definition of raw-capture rectification (tests/rectify_model.py) against exact identities and against its independent fp64
form, the reference's camera arithmetic, and the host stage (diffuman4d_amd/host/rectify.py) and its command line on a stand-in for
``ops.rectify`` in the manner of tests/cpu_standin_ops.py: the stand-in reads the very descriptors, tables and staged bytes the library
would be given and computes the result with the model."""
import contextlib
import importlib.util
import io
import json

import numpy as np
import pytest
import torch
from PIL import Image

import rectify_model as rm
from cpu_standin_ops import ROOT

IDENT_CCM = [[0, 1, 0]] * 3


def pinhole(h, w):
    """Focal lengths that are powers of two and a principal point on a quarter pixel: (x + 0.5 - cx) / f * f + cx - 0.5 is then x in
    fp32 exactly, which an identity needs, since the undistorted value is truncated (x - 1e-6 would sample 0.999999 of the pixel)."""
    return np.array([[64.0, 0, w / 2 + 0.25], [0, 32.0, h / 2 - 0.5], [0, 0, 1]])


def identity_case(h, w, scale, seed=3):
    K = pinhole(h, w)
    return dict(image=rm.texture(h, w, seed), K=K, D=np.zeros(5), ccm=IDENT_CCM, K_undist=K, undist_hw=(h, w),
                resized_wh=(w // scale, h // scale), cropped_ltrb=(0, 0, w // scale, h // scale))


# -- pure-numpy identities -------------------------------------------------------------------------------------------------------------
def test_identity_returns_the_input():
    """No distortion, the identity colour table, the same camera, scale 1, the full crop: pixel centres map onto pixel centres."""
    c = identity_case(37, 53, 1)
    assert np.array_equal(rm.rectify(**c), c["image"])


def test_scale_two_is_the_round_half_even_block_mean():
    c = identity_case(40, 56, 2)
    s = c["image"].astype(np.int64).reshape(20, 2, 28, 2, 3).sum(axis=(1, 3))
    q, r = s // 4, s % 4
    want = q + ((r == 3) | ((r == 2) & (q % 2 == 1)))  # .25 down, .75 up, .5 to even
    assert np.array_equal(rm.rectify(**c), want.astype(np.uint8))


def test_a_crop_is_the_slice_of_the_uncropped_result():
    c = rm.cases()[7]
    rw, rh = c["resized_wh"]
    full = rm.rectify(**dict(c, cropped_ltrb=(0, 0, rw, rh)))
    for ltrb in ((0, 0, rw, rh), (5, 7, 40, 33), (rw - 9, 0, rw, 11), (0, rh - 3, 17, rh)):
        l, t, r, b = ltrb
        assert np.array_equal(rm.rectify(**dict(c, cropped_ltrb=ltrb)), full[t:b, l:r])


def test_colour_clamps_and_permutes_the_rows():
    """Rows in B, G, R order: the first row of ccm is applied to the LAST channel of the RGB image."""
    lut = rm.colour_table([[0, 0, 7], [0, 1, 0], [0, 2, 1]])
    b = np.arange(256, dtype=np.float32)
    assert np.array_equal(lut[0], np.minimum(2 * b + 1, 255)) and np.array_equal(lut[1], b) and np.array_equal(lut[2], np.full(256, 7, np.float32))
    lut = rm.colour_table([[0.01, 0, 0], [0, -1, 100], [0, 3, -300]])
    assert lut.min() == 0 and lut.max() == 255
    assert np.array_equal(lut[0], np.clip(3 * b - 300, 0, 255)) and np.array_equal(lut[1], np.clip(100 - b, 0, 255))
    assert lut[2][0] == 0 and lut[2][200] == 255 and lut[2][100] == np.float32(100.0)
    c = identity_case(16, 24, 1)
    out = rm.rectify(**dict(c, ccm=[[0, 0, 300], [0, 1, 0], [0, 0, -5]]))
    assert (out[..., 0] == 0).all() and np.array_equal(out[..., 1], c["image"][..., 1]) and (out[..., 2] == 255).all()


# -- the model against its fp64 form ---------------------------------------------------------------------------------------------------
MEASURED_SHARE = 6.02e-4


def test_model_against_reference64():
    """The 12 seeded cases of rectify_model.cases(): the fp32 definition and the independent fp64 form differ by at most one grey level (a
    one-level flip at the truncation to uint8 moves a rounded mean by at most one), and in few bytes.  Measured on the CPU: 75 of
    124,641 bytes differ, a share of 6.02e-4 (the largest single case 1.6e-2: case 5, whose vertical scale 2.0 puts means on .5 ties);
    asserted below twice that, the margin for seed-to-seed spread.  Several cases hold black (outside) pixels."""
    total = differ = black = 0
    for k, c in enumerate(rm.cases()):
        a, b = rm.rectify(**c), rm.reference64(**c)
        l, t, r, bt = c["cropped_ltrb"]
        assert a.shape == b.shape == (bt - t, r - l, 3)
        d = np.abs(a.astype(np.int32) - b.astype(np.int32))
        assert d.max() <= 1, (k, int(d.max()))
        assert a.std() > 20, k  # a texture, not a flat image
        total, differ, black = total + d.size, differ + int((d > 0).sum()), black + int((a == 0).all(axis=-1).sum())
    print(f"model vs reference64: {differ} of {total} bytes differ, share {differ / total:.3e}; black pixels {black}")
    assert differ / total < 2 * MEASURED_SHARE
    assert black > 1000


def test_cases_cover_what_they_claim():
    cs = rm.cases()
    assert len(cs) == 12
    sizes = {c["image"].shape[:2] for c in cs}
    assert (48, 64) in sizes and (263, 301) in sizes
    assert any(c["D"][0] < 0 for c in cs) and any(c["D"][0] > 0 for c in cs) and all(np.all(c["D"][1:] != 0) for c in cs)
    assert any(c["undist_hw"][1] / c["resized_wh"][0] != c["undist_hw"][0] / c["resized_wh"][1] for c in cs)
    touch = set()
    for c in cs:
        l, t, r, b = c["cropped_ltrb"]
        rw, rh = c["resized_wh"]
        touch |= {n for n, hit in (("l", l == 0), ("t", t == 0), ("r", r == rw), ("b", b == rh)) if hit}
        touch |= {"inner"} if (l > 0 and t > 0 and r < rw and b < rh) else set()
    assert touch == {"l", "t", "r", "b", "inner"}


def test_area_taps_refuse_other_scales():
    for n_in, n_out in ((10, 11), (81, 10), (10, 0)):
        with pytest.raises(ValueError, match="scale is outside"):
            rm.area_taps(n_in, n_out)
    first, count, wts = rm.area_taps(7, 3)
    assert list(first) == [0, 2, 4] and list(count) == [3, 3, 3] and wts.dtype == np.float32
    assert np.allclose(wts.sum(axis=1), 1, atol=1e-6)


# -- the reference's camera arithmetic -------------------------------------------------------------------------------------------------
def cam5():
    return {"K": np.array([[2496.0, 0, 1224.0], [0, 2496.0, 1024.0], [0, 0, 1]]), "H": 2048, "W": 2448}


def cam12():
    return {"K": np.array([[3648.0, 0, 2048.0], [0, 3648.0, 1500.0], [0, 0, 1]]), "H": 3000, "W": 4096}


def test_calc_unified_cameras_against_hand_computed_values():
    from diffuman4d_amd.host.rectify import calc_unified_cameras
    cams = {f"{k:02d}": cam5() if k < 48 else cam12() for k in range(60)}
    out = calc_unified_cameras(cams)
    # 5 MP: f = 2496 * 1024 / 1920 = 1331.2, scale 8 / 15: 2448 -> 1305.6 -> 1306, 2048 -> 1092.27 -> 1092; c = (652.8, 546.13)
    a = out["00"]
    assert a["resized_wh"] == (1306, 1092) and a["cropped_ltrb"] == (141, 34, 1165, 1058) and (a["H"], a["W"]) == (1024, 1024)
    assert abs(a["K"][0, 0] - 1331.2) < 1e-9 and abs(a["K"][1, 1] - 1331.2) < 1e-9 and a["K"][0, 2] == 512 and a["K"][1, 2] == 512
    # 12 MP: f = 3648 * 1024 / 1920 = 1945.6, target int(2880 * 1024 / 1920) = 1536: 4096 -> 2184.53 -> 2185, 3000 -> 1600; c = (1092.27, 800)
    b = out["48"]
    assert b["resized_wh"] == (2185, 1600) and b["cropped_ltrb"] == (324, 32, 1860, 1568) and (b["H"], b["W"]) == (1536, 1536)
    assert abs(b["K"][0, 0] - 1945.6) < 1e-9 and b["K"][0, 2] == 768 and b["K"][1, 2] == 768
    assert cams["00"]["K"][0, 0] == 2496.0 and "resized_wh" not in cams["00"]  # a deep copy
    half = calc_unified_cameras({"00": cam5()}, image_size=512)["00"]
    assert half["resized_wh"] == (653, 546) and half["cropped_ltrb"] == (70, 17, 582, 529)


def test_calc_unified_cameras_refusals():
    from diffuman4d_amd.host.rectify import calc_unified_cameras
    cams = {f"{k:02d}": cam5() if k < 48 else cam12() for k in range(61)}
    with pytest.raises(ValueError, match="Unknown camera id: 60"):
        calc_unified_cameras(cams)
    off = cam5()
    off["K"][0, 2] = 100.0  # the crop about the principal point leaves the resized image
    with pytest.raises(AssertionError):
        calc_unified_cameras({"00": off})


# -- the host stage on a stand-in ------------------------------------------------------------------------------------------------------
class Standin:
    """``ops.rectify`` on the CPU: descriptors, tables, colour tables and staged bytes as the library takes them -> the model's result."""

    def __init__(self):
        self.calls = []

    def __call__(self, blob, meta, meta_host, n, desc_off, tab_off, tab_len, lut, out_bytes):
        from diffuman4d_amd.host import lib as L
        m = meta_host.numpy()
        desc = m[desc_off: desc_off + n * L.RECTIFY_FIELDS * 8].view(np.int64).reshape(n, L.RECTIFY_FIELDS)
        tab = m[tab_off: tab_off + tab_len * 4].view(np.int32)
        assert np.array_equal(meta.numpy(), m) and tuple(lut.shape) == (n, 3, 256) and lut.dtype == torch.float32
        out = np.zeros(out_bytes, dtype=np.uint8)
        for k, d in enumerate(desc):
            src, h, w, uh, uw, rh, rw, top, left, ch, cw, htab, hk, vtab, vk, cam, dst = (int(v) for v in d[:17])
            assert src % 16 == 0 and dst % 16 == 0 and not d[17:].any()
            for off, kk, n_in, n_out in ((htab, hk, uw, rw), (vtab, vk, uh, rh)):  # the host's tables are the model's
                first, count, wts = rm.area_taps(n_in, n_out)
                assert kk == wts.shape[1]
                assert np.array_equal(tab[off: off + 2 * n_out].reshape(n_out, 2), np.stack([first, count], axis=1))
                assert np.array_equal(tab[off + 2 * n_out: off + (2 + kk) * n_out].view(np.float32).reshape(n_out, kk), wts)
            image = blob.numpy()[src: src + h * w * 3].reshape(h, w, 3)
            und = rm.undistort_f32(image, lut[k].numpy(), tab[cam: cam + 16].view(np.float32), (uh, uw))
            out[dst: dst + ch * cw * 3] = rm.area_resize(und, (rw, rh))[top: top + ch, left: left + cw].reshape(-1)
        self.calls.append(n)
        return torch.from_numpy(out)


@pytest.fixture
def on_cpu(monkeypatch):
    from diffuman4d_amd.host import lib as L, ops
    standin = Standin()
    standin.devices = []
    monkeypatch.setattr(L, "hip_device", lambda device, what: standin.devices.append(device) or torch.device("cpu"))
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "stream", lambda s: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "Stream", lambda device=None: None)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: type("S", (), {"synchronize": lambda self: None, "cuda_stream": 0})())
    monkeypatch.setattr(ops, "rectify", standin)
    return standin


def camera_entry(c):
    h, w = c["image"].shape[:2]
    return {"K": c["K"].tolist(), "D": c["D"].tolist(), "ccm": c["ccm"].tolist(), "K_undist": c["K_undist"].tolist(), "H_undist": c["undist_hw"][0],
            "W_undist": c["undist_hw"][1], "H": h, "W": w, "resized_wh": list(c["resized_wh"]), "cropped_ltrb": list(c["cropped_ltrb"])}


def encoded(a, fmt, **kw):
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, format=fmt, **kw)
    return buf.getvalue()


def test_extract_images_on_the_standin(on_cpu, tmp_path):
    from diffuman4d_amd.host import rectify
    cs = rm.cases()
    cam_a, cam_b = cs[2], cs[4]
    cameras = {"00": camera_entry(cam_a), "07": camera_entry(cam_b)}
    cams_json = tmp_path / "cams.json"
    cams_json.write_text(json.dumps(cameras))
    png = tmp_path / "raw.png"
    png.write_bytes(encoded(cam_a["image"], "PNG"))
    jpg = encoded(cam_b["image"], "JPEG", quality=92)
    arr = rm.texture(*cam_b["image"].shape[:2], 77)
    frames = [("00", "000000", str(png)), ("07", "000000", jpg), ("07", "000001", arr), ("00", "000001", png.read_bytes())]
    out_dir = tmp_path / "images"
    res = rectify.extract_images(iter(frames), str(cams_json), str(out_dir), ".png", 85, True, 3, batch_size=3, gpu_ids=[0])
    up = sum((c["image"].shape[0] * c["image"].shape[1] * 3 + 15) // 16 * 16 for c in (cam_a, cam_b, cam_b, cam_a))  # every source as pixels
    assert res == {"frames": 4, "written": 4, "skipped": 0, "device_decoded": 0, "pillow_decoded": 3, "bytes_uploaded": up}
    assert on_cpu.calls == [3, 1]
    assert sorted(str(p.relative_to(out_dir)) for p in out_dir.rglob("*")) == ["00", "00/000000.png", "00/000001.png", "07", "07/000000.png", "07/000001.png"]

    def want(c, image):
        return rm.rectify(**dict(c, image=image))
    jpg_pixels = np.asarray(Image.open(io.BytesIO(jpg)).convert("RGB"))
    for name, ref in (("00/000000", want(cam_a, cam_a["image"])), ("07/000000", want(cam_b, jpg_pixels)), ("07/000001", want(cam_b, arr)),
                      ("00/000001", want(cam_a, cam_a["image"]))):
        assert np.array_equal(np.asarray(Image.open(out_dir / f"{name}.png")), ref), name

    # skip_exists: a truncated file is removed and written again, the others are kept
    victim = out_dir / "07" / "000001.png"
    good = victim.read_bytes()
    victim.write_bytes(good[: len(good) // 2])
    stamp = (out_dir / "00" / "000000.png").stat().st_mtime_ns
    on_cpu.calls.clear()
    res = rectify.extract_images(frames, cameras, str(out_dir), ".png", batch_size=8, gpu_ids=[0], num_workers=2)
    assert res == {"frames": 4, "written": 1, "skipped": 3, "device_decoded": 0, "pillow_decoded": 0, "bytes_uploaded": (arr.nbytes + 15) // 16 * 16} and on_cpu.calls == [1]
    assert victim.read_bytes() == good and (out_dir / "00" / "000000.png").stat().st_mtime_ns == stamp
    # skip_exists off: everything again
    res = rectify.extract_images(frames, cameras, str(out_dir), ".png", 85, False, batch_size=8, gpu_ids=[0])
    assert res["written"] == 4 and res["skipped"] == 0
    # a frame size that is not the camera's, a camera that is not named
    with pytest.raises(ValueError, match="not the camera's frame size"):
        rectify.extract_images([("00", "000009", arr)], cameras, str(out_dir), ".png", gpu_ids=[0])
    with pytest.raises(ValueError, match="is not in cameras"):
        rectify.extract_images([("03", "000000", arr)], cameras, str(out_dir), ".png", gpu_ids=[0])


def test_frames_are_consumed_lazily_and_skipped_sources_are_never_read(on_cpu, tmp_path, monkeypatch):
    """`frames` is taken a window at a time (here one batch of two), and a callable source is called by the loader only for a frame
    that is not skipped."""
    from diffuman4d_amd.host import rectify
    monkeypatch.setattr(rectify, "WINDOW_BATCHES", 1)
    c = rm.cases()[0]
    cameras = {"00": camera_entry(c)}
    taken, read = [], []

    def source(k):
        def get():
            read.append(k)
            return encoded(c["image"], "PNG") if k % 2 else c["image"]
        return get

    def frames():
        for k in range(5):
            taken.append((k, len(on_cpu.calls)))  # how many device calls had been made when frame k was asked for
            yield "00", f"{k:06d}", source(k)
    out_dir = tmp_path / "images"
    res = rectify.extract_images(frames(), cameras, str(out_dir), ".png", batch_size=2, gpu_ids=[0], num_workers=2)
    assert res["frames"] == 5 and res["written"] == 5 and res["pillow_decoded"] == 2 and sorted(read) == [0, 1, 2, 3, 4]
    assert taken == [(0, 0), (1, 0), (2, 1), (3, 1), (4, 2)] and on_cpu.calls == [2, 2, 1]
    want = rm.rectify(**c)
    assert all(np.array_equal(np.asarray(Image.open(out_dir / "00" / f"{k:06d}.png")), want) for k in range(5))
    (out_dir / "00" / "000003.png").unlink()
    read.clear()
    res = rectify.extract_images(frames(), cameras, str(out_dir), ".png", batch_size=2, gpu_ids=[0], num_workers=2)
    assert res["skipped"] == 4 and res["written"] == 1 and read == [3]


def test_the_hosts_colour_table_is_the_models():
    from diffuman4d_amd.host import rectify
    rng = np.random.default_rng(5)
    for ccm in [IDENT_CCM, [[0.01, 0, 0], [0, -1, 100], [0, 3, -300]]] + [c["ccm"] for c in rm.cases()[:3]] + \
            [rng.normal(0, 1, (3, 3)) * [1e-3, 1, 20] for _ in range(20)]:
        assert np.array_equal(rectify.colour_table(ccm), rm.colour_table(ccm))


def test_scales_outside_one_to_eight_raise_before_any_device_call(on_cpu, tmp_path):
    from diffuman4d_amd.host import rectify
    c = rm.cases()[0]
    h, w = c["undist_hw"]
    for resized in ((w + 1, h), (w, h + 1), (w // 9, h), (w, h // 9)):
        cams = {"00": dict(camera_entry(c), resized_wh=list(resized), cropped_ltrb=[0, 0, 1, 1])}
        with pytest.raises(ValueError, match="scale is outside 1..8"):
            rectify.extract_images([("00", "000000", c["image"])], cams, str(tmp_path / "o"), ".png", gpu_ids=[0])
        with pytest.raises(ValueError, match="scale is outside 1..8"):
            rectify.calib_undist_image(c["image"], c["K"], c["D"], c["ccm"], resized, (0, 0, 1, 1), undist_K=c["K_undist"], undist_hw=(h, w))
    assert on_cpu.calls == [] and on_cpu.devices == [] and not (tmp_path / "o").exists()
    with pytest.raises(ValueError, match="leaves the resized image"):
        rectify.Rectification(c["K"], c["D"], c["ccm"], (w, h), (0, 0, w + 1, h), c["K_undist"], (h, w))


def test_calib_undist_image_and_rectify_batch_on_the_standin(on_cpu):
    from diffuman4d_amd.host import rectify
    c = rm.cases()[3]
    got = rectify.calib_undist_image(c["image"], c["K"], c["D"], c["ccm"], c["resized_wh"], c["cropped_ltrb"], undist_K=c["K_undist"],
                                     undist_hw=c["undist_hw"])
    assert got.dtype == np.uint8 and np.array_equal(got, rm.rectify(**c))
    # a memory budget of one image per call: the same results from more calls
    cs = rm.cases()[:3]
    rects = [rectify.Rectification(c["K"], c["D"], c["ccm"], c["resized_wh"], c["cropped_ltrb"], c["K_undist"], c["undist_hw"]) for c in cs]
    on_cpu.calls.clear()
    outs = rectify.rectify_batch([c["image"] for c in cs], rects, "cuda", stage_bytes=1)
    assert on_cpu.calls == [1, 1, 1] and all(np.array_equal(o.numpy(), rm.rectify(**c)) for o, c in zip(outs, cs))


def test_load_cameras_derives_resize_and_crop_as_the_reference_does():
    from diffuman4d_amd.host import rectify
    cam = {"K": cam5()["K"].tolist(), "D": [0.1, 0, 0, 0, 0], "ccm": IDENT_CCM, "K_undist": cam5()["K"].tolist(), "H_undist": 2048, "W_undist": 2448,
           "H": 2048, "W": 2448}
    r = rectify.load_cameras({"00": cam})["00"]
    assert (r.rw, r.rh, r.left, r.top, r.cw, r.ch) == (1306, 1092, 141, 34, 1024, 1024) and r.source_hw == (2048, 2448)
    with pytest.raises(ValueError, match="missing ccm"):
        rectify.load_cameras({"00": {k: v for k, v in cam.items() if k != "ccm"}})


def test_smc_frames_needs_h5py(tmp_path, monkeypatch):
    import sys
    from diffuman4d_amd.host import rectify
    monkeypatch.setitem(sys.modules, "h5py", None)  # the import fails, wherever the test runs
    with pytest.raises(ImportError, match="h5py"):
        rectify.SmcFrames(str(tmp_path / "scene.smc"))


# -- the command line ------------------------------------------------------------------------------------------------------------------
def test_tool_help_and_argument_errors(tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("extract_images_tool", ROOT / "tools" / "extract_images.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with pytest.raises(SystemExit) as e:
        tool.main(["--help"])
    assert e.value.code == 0 and "--cameras_json" in capsys.readouterr().out
    cams = tmp_path / "c.json"
    cams.write_text("{}")
    raw = tmp_path / "raw"
    raw.mkdir()
    bad = ([], ["--raw_images_dir", str(raw), "--out_images_dir", "o"], ["--smc", "a.smc", "--raw_images_dir", str(raw), "--cameras_json", str(cams), "--out_images_dir", "o"],
           ["--raw_images_dir", str(raw), "--cameras_json", str(tmp_path / "none.json"), "--out_images_dir", "o"],
           ["--raw_images_dir", str(tmp_path / "none"), "--cameras_json", str(cams), "--out_images_dir", "o"],
           ["--raw_images_dir", str(raw), "--cameras_json", str(cams), "--out_images_dir", "o", "--batch_size", "0"],
           ["--raw_images_dir", str(raw), "--cameras_json", str(cams), "--out_images_dir", "o", "--gpu_ids", "x"])
    for argv in bad:
        with pytest.raises(SystemExit) as e:
            tool.main(argv)
        assert e.value.code == 2, argv
    (raw / "00").mkdir()
    (raw / "00" / "000003.jpg").write_bytes(b"x")
    (raw / "01").mkdir()
    (raw / "01" / "000000.png").write_bytes(b"x")
    assert tool.raw_frames(str(raw)) == [("00", "000003", str(raw / "00" / "000003.jpg")), ("01", "000000", str(raw / "01" / "000000.png"))]
