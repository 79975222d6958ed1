"""GPU: dm4d_rectify_u8 (csrc/rectify.hip) through diffuman4d_amd/host/rectify.py against the numpy definition tests/rectify_model.py,
byte for byte; batch invariance and repeatability; every kind of tile of the kernel's 32 x 8 tile shape and both store paths; and the
stage end to end with the sources decoded by Pillow and on the device."""
import io
import json

import numpy as np
import pytest
import torch
from PIL import Image

import rectify_model as rm

pytestmark = pytest.mark.gpu

TILE_W, TILE_H = 32, 8  # kTileW, kTileH of csrc/rectify.hip


def rect_of(c):
    from diffuman4d_amd.host import rectify
    return rectify.Rectification(c["K"], c["D"], c["ccm"], c["resized_wh"], c["cropped_ltrb"], c["K_undist"], c["undist_hw"])


def run(cases, dev):
    from diffuman4d_amd.host import rectify
    return [t.cpu().numpy() for t in rectify.rectify_batch([c["image"] for c in cases], [rect_of(c) for c in cases], dev)]


@pytest.fixture(scope="module")
def cases():
    return rm.cases()


@pytest.fixture(scope="module")
def want(cases):
    return [rm.rectify(**c) for c in cases]


def test_mixed_batch_equals_the_model(hip_device, cases, want):
    got = run(cases, hip_device)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == np.uint8, k
        assert np.array_equal(g, w), (k, int(np.abs(g.astype(int) - w.astype(int)).max()), float((g != w).mean()))


def test_batch_invariance_and_repeatability(hip_device, cases, want):
    batch = run(cases, hip_device)
    again = run(cases, hip_device)
    rev = run(cases[::-1], hip_device)[::-1]
    for k, c in enumerate(cases):
        alone = run([c], hip_device)[0]
        assert np.array_equal(batch[k], again[k]) and np.array_equal(batch[k], rev[k]) and np.array_equal(batch[k], alone), k


def test_every_kind_of_tile_and_both_store_paths(hip_device, cases):
    """301 x 263 -> 150 x 131: five tile columns and seventeen tile rows, neither size a multiple of the tile (interior, edge and corner
    tiles; rows of 450 bytes leave through byte stores).  -> 144 x 131: rows of 432 bytes leave through 16-byte stores, the last tile of
    a row is half a tile wide.  A crop of 48 x 21 at (7, 5): 16-byte stores of a crop that starts inside the resized image."""
    base = cases[7]
    assert base["image"].shape[:2] == (263, 301)
    big = dict(base, resized_wh=(150, 131), cropped_ltrb=(0, 0, 150, 131))
    vec = dict(base, resized_wh=(144, 131), cropped_ltrb=(0, 0, 144, 131))
    crop = dict(base, resized_wh=(150, 131), cropped_ltrb=(7, 5, 55, 26))
    assert 150 // TILE_W >= 3 and 131 // TILE_H >= 3 and 150 % TILE_W and 131 % TILE_H and 144 % 16 == 0 and 144 % TILE_W
    for k, (g, c) in enumerate(zip(run([big, vec, crop], hip_device), (big, vec, crop))):
        assert np.array_equal(g, rm.rectify(**c)), k


def test_the_largest_scale_and_the_largest_patch(hip_device):
    """Scale 8 and just below it on both axes: windows of 8 and 9 taps, and a full tile's patch of 256 x 64 and 257 x 65 undistorted
    pixels, the most LDS a workgroup asks for (about 50 of the 64 KB)."""
    exact = rm.make_case(30, 70, 260, 1.0, 1.0, -0.1, "full", uh=72, uw=264)
    exact.update(resized_wh=(33, 9), cropped_ltrb=(0, 0, 33, 9))
    below = rm.make_case(31, 70, 260, 1.0, 1.0, 0.1, "full", uh=71, uw=263)
    below.update(resized_wh=(33, 9), cropped_ltrb=(0, 0, 33, 9))
    for k, (g, c) in enumerate(zip(run([exact, below], hip_device), (exact, below))):
        assert np.array_equal(g, rm.rectify(**c)), k


def test_every_sample_outside_the_source_is_black(hip_device, cases):
    base = cases[2]
    away = base["K_undist"].copy()
    away[0, 2] = -1.0e5
    w = rm.rectify(**dict(base, K_undist=away))
    assert not w.any() and np.array_equal(run([dict(base, K_undist=away)], hip_device)[0], w)
    # coefficients that overflow to inf and NaN in fp32 everywhere but at the principal point, which lies on a pixel centre (r2 = 0)
    wild = dict(base, D=np.array([3.0e38, 3.0e38, 1.0, 1.0, 3.0e38]))
    w = rm.rectify(**wild)
    assert np.count_nonzero(w.any(axis=-1)) <= 4 and np.array_equal(run([wild], hip_device)[0], w)


def test_identities_on_the_device(hip_device):
    K = np.array([[64.0, 0, 28.25], [0, 32.0, 19.5], [0, 0, 1]])  # exact in fp32: see tests/test_rectify_cpu.py::pinhole
    img = rm.texture(40, 56, 3)
    same = dict(image=img, K=K, D=np.zeros(5), ccm=[[0, 1, 0]] * 3, K_undist=K, undist_hw=(40, 56), resized_wh=(56, 40), cropped_ltrb=(0, 0, 56, 40))
    half = dict(same, resized_wh=(28, 20), cropped_ltrb=(0, 0, 28, 20))
    g_same, g_half = run([same, half], hip_device)
    assert np.array_equal(g_same, img)
    s = img.astype(np.int64).reshape(20, 2, 28, 2, 3).sum(axis=(1, 3))
    q, r = s // 4, s % 4
    assert np.array_equal(g_half, (q + ((r == 3) | ((r == 2) & (q % 2 == 1)))).astype(np.uint8))


def test_calib_undist_image_takes_the_references_arguments(hip_device, cases, want):
    from diffuman4d_amd.host import rectify
    c = cases[5]
    got = rectify.calib_undist_image(c["image"], c["K"], c["D"], c["ccm"], c["resized_wh"], c["cropped_ltrb"], undist_K=c["K_undist"],
                                     undist_hw=c["undist_hw"], device=hip_device)
    assert isinstance(got, np.ndarray) and np.array_equal(got, want[5])


def encoded(a, **kw):
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, format="JPEG", **kw)
    return buf.getvalue()


def test_extract_images_end_to_end_with_and_without_device_decode(hip_device, tmp_path):
    """2 cameras x 3 frames of 96 x 80 baseline JPEG sources (paths and bytes), one progressive JPEG, which the device decoder does not
    take, and one array source, written as .png: the files hold the model applied to Pillow's decode, and are the same files with the
    sources decoded on the device."""
    from diffuman4d_amd.host import rectify
    cams = {"00": rm.make_case(40, 80, 96, 1.37, 1.83, -0.2, "inner"), "01": rm.make_case(41, 80, 96, 2.0, 1.0, 0.15, "full", 6.0)}
    cameras = {}
    for label, c in cams.items():
        cameras[label] = {"K": c["K"].tolist(), "D": c["D"].tolist(), "ccm": c["ccm"].tolist(), "K_undist": c["K_undist"].tolist(), "H_undist": 80,
                          "W_undist": 96, "H": 80, "W": 96, "resized_wh": list(c["resized_wh"]), "cropped_ltrb": list(c["cropped_ltrb"])}
    cams_json = tmp_path / "cams.json"
    cams_json.write_text(json.dumps(cameras))
    frames, pixels = [], {}
    for ci, label in enumerate(cams):
        for fr in range(3):
            data = encoded(rm.texture(80, 96, 50 + 10 * ci + fr), quality=90)
            src = data
            if fr != 1:
                path = tmp_path / f"raw_{label}_{fr}.jpg"
                path.write_bytes(data)
                src = str(path)
            frames.append((label, f"{fr:06d}", src))
            pixels[(label, f"{fr:06d}")] = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    prog = encoded(rm.texture(80, 96, 90), quality=90, progressive=True)
    frames.append(("00", "000003", prog))
    pixels[("00", "000003")] = np.asarray(Image.open(io.BytesIO(prog)).convert("RGB"))
    arr = rm.texture(80, 96, 91)
    frames.append(("01", "000003", arr))
    pixels[("01", "000003")] = arr
    g = hip_device.index or 0
    off = rectify.extract_images(frames, str(cams_json), str(tmp_path / "off"), ".png", batch_size=3, gpu_ids=[g], num_workers=4)
    on = rectify.extract_images(frames, cameras, str(tmp_path / "on"), ".png", batch_size=3, gpu_ids=[g], num_workers=4, device_decode=True)
    from diffuman4d_amd.host import codec, jpegdec
    plane = 80 * 96 * 3
    assert off == {"frames": 8, "written": 8, "skipped": 0, "device_decoded": 0, "pillow_decoded": 7, "bytes_uploaded": 8 * plane}
    files = sum(jpegdec.probe(codec.read_file(s)).payload_len for _, _, s in frames[:6])  # the six baseline files go up as file bytes
    assert on == {"frames": 8, "written": 8, "skipped": 0, "device_decoded": 6, "pillow_decoded": 1, "bytes_uploaded": files + 2 * plane}
    assert files < 6 * plane
    for (label, fr), px in pixels.items():
        a = (tmp_path / "off" / label / f"{fr}.png").read_bytes()
        assert a == (tmp_path / "on" / label / f"{fr}.png").read_bytes(), (label, fr)
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(a))), rm.rectify(**dict(cams[label], image=px))), (label, fr)
    again = rectify.extract_images(frames, cameras, str(tmp_path / "on"), ".png", batch_size=8, gpu_ids=[g], device_decode=True)
    assert again["written"] == 0 and again["skipped"] == 8


def test_the_wrapper_refuses_what_it_cannot_take(hip_device):
    from diffuman4d_amd.host import lib as L, ops, rectify
    with pytest.raises(L.Dm4dError, match="HIP device"):
        rectify.rectify_batch([rm.texture(8, 8, 0)], [rect_of(rm.cases()[0])], "cpu")
    blob = torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(L.Dm4dError, match="HIP device"):
        ops.rectify(blob, blob, blob, 1, 0, 0, 1, torch.zeros(1, 3, 256), 16)
