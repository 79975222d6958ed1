"""CPU: the captured-scene dataset (diffuman4d_amd/host/capture.py) against Pillow and against the reference's own SpaTemDataset
(its results on tests/golden/capture_scene, recorded by tests/golden/make_golden_capture.py in capture_reference.pt).  The device
resize is replaced here by tests/capture_model.py, which reads the same staging buffer the kernel reads."""
import hashlib
import json
import shutil
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image

import capture_model as cm
from diffuman4d_amd.host import capture, lib as L
from diffuman4d_amd.host.dataset import plucker_maps

GOLDEN = Path(__file__).resolve().parent / "golden"
SCENE_DIR = GOLDEN / "capture_scene"
REF = torch.load(GOLDEN / "capture_reference.pt", weights_only=False)
SCENE = REF["scene"]


def digest(t) -> str:
    a = t.detach().cpu().contiguous().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
    return hashlib.sha256(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


@pytest.fixture
def standin(monkeypatch):
    monkeypatch.setattr(capture.ops, "capture_crop_resize", cm.standin_crop_resize)


def dataset(data_dir=SCENE_DIR, **kw):
    return capture.SpaTemDataset(data_dir=str(data_dir), scene_label=SCENE, device="cpu", decode_threads=4, **kw)


# -- 1. the host coefficient tables + the two-pass model are Pillow, byte for byte -----------------------------------------------
def pillow_cases():
    rng = np.random.default_rng(1234)
    cases = []
    for n in range(52):
        mode = "RGB" if n % 2 == 0 else "L"
        h, w = (int(v) for v in rng.integers(8, 120, 2))
        ch, cw = (int(v) for v in rng.integers(20, 160, 2))
        H, W = (int(v) for v in rng.integers(8, 200, 2))
        top, left = int(rng.integers(0, max(1, h - ch + 1))), int(rng.integers(0, max(1, w - cw + 1)))
        edge = n % 6  # boxes past each edge
        if edge == 1:
            left = -int(rng.integers(1, 30))
        elif edge == 2:
            top = -int(rng.integers(1, 30))
        elif edge == 3:
            left = w - cw + int(rng.integers(1, 30))
        elif edge == 4:
            top = h - ch + int(rng.integers(1, 30))
        if n % 7 == 0:
            H = ch  # vertical pass skipped
        if n % 9 == 0:
            W = cw  # horizontal pass skipped
        if n % 13 == 0:
            ch, cw = 1, 1  # 1-pixel crop
        if n == 26:
            H, W = ch, cw  # no resize at all
        cases.append((mode, h, w, top, left, ch, cw, H, W, n))
    return cases


@pytest.mark.parametrize("mode,h,w,top,left,ch,cw,H,W,seed", pillow_cases())
def test_model_equals_pillow_crop_resize(mode, h, w, top, left, ch, cw, H, W, seed):
    a = np.random.default_rng(seed).integers(0, 256, (h, w, 3) if mode == "RGB" else (h, w), dtype=np.uint8)
    ref = np.asarray(Image.fromarray(a).crop((left, top, left + cw, top + ch)).resize((W, H), Image.BICUBIC))
    assert np.array_equal(cm.crop_resize(a, top, left, ch, cw, H, W), ref)


def test_tables_sum_sequentially_and_identity_is_exact():
    b, k = capture.bicubic_table(37, 37)
    assert (k.max(axis=1) == 1 << 22).all() and (k.sum(axis=1) == 1 << 22).all()  # an identity pass keeps every byte
    b, k = capture.bicubic_table(1400, 1024)
    assert b.shape == (1024, 2) and k.shape[1] == 2 * int(np.ceil(2 * 1400 / 1024)) + 1
    assert (b[:, 0] >= 0).all() and (b.sum(axis=1) <= 1400).all()


# -- 2. host bookkeeping -------------------------------------------------------------------------------------------------------
def test_cameras_equal_the_reference():
    cams = capture.read_cameras(str(SCENE_DIR / SCENE / "transforms.json"))
    assert sorted(cams) == sorted(REF["cameras"])
    for lab, c in REF["cameras"].items():
        assert torch.equal(cams[lab]["K"], c["K"]) and cams[lab]["K"].dtype == c["K"].dtype
        assert torch.equal(cams[lab]["pose"], c["pose"])


@pytest.mark.parametrize("name", sorted(REF["queries"]))
def test_get_item_equals_the_reference(name, standin, monkeypatch):
    q = REF["queries"][name]
    masks = []
    inner = capture.skeleton_mask
    monkeypatch.setattr(capture, "skeleton_mask", lambda s, p="": masks.append(inner(s, p)) or masks[-1])
    s = dataset(**q["kw"]).get_item(SCENE, q["spa"], q["tem"], REF["inputs"])
    # bookkeeping
    assert s["domain"] == q["domain"] and s["labels"] == q["labels"]
    assert torch.equal(s["Ks"], q["Ks"]) and torch.equal(s["poses"], q["poses"])
    assert s["hws"] == q["hws"] and s["crops"] == q["crops"]
    assert tuple(s["cond_masks"].shape) == q["cond_masks_shape"] and torch.equal(s["cond_masks"][:, 0, 0, 0], q["cond_masks"])
    assert sorted(digest(m) for m in masks) == sorted(q["skeleton_masks"])  # has_gt_target=False masks (frames load in parallel)
    # tensors (the stand-in computes what the kernel computes)
    for k in ("pixel_values", "skeletons"):
        assert tuple(s[k].shape) == q[k + "_shape"], k
        assert torch.equal(s[k][:, :, ::16, ::16], q[k + "_thumb"]), k
        assert digest(s[k]) == q[k + "_sha256"], k
    # Pluecker maps: dataset.plucker_maps on these cameras, which tests/test_plucker.py pins to the reference's ray_utils to 1e-6
    pl = s["plucker_embeds"]
    assert tuple(pl.shape) == q["plucker_embeds_shape"] and torch.equal(pl, plucker_maps(q["kw"]["height"], q["kw"]["width"], s["Ks"], s["poses"]))
    assert float((pl[:, :, ::16, ::16] - q["plucker_embeds_thumb"]).abs().max()) <= 1e-6
    for k in ("pixel_values", "skeletons"):
        assert s[k].min() >= -1.0 and s[k].max() <= 1.0


def test_plucker_cameras_mode_returns_none(standin):
    q = REF["queries"]["temporal_down"]
    s = dataset(plucker="cameras", **q["kw"]).get_item(SCENE, q["spa"], q["tem"], REF["inputs"])
    assert s["plucker_embeds"] is None and digest(s["pixel_values"]) == q["pixel_values_sha256"]


def test_nearest_input_camera_integer_form():
    ds = dataset(height=64, width=64)
    q = REF["queries"]["temporal_down"]
    assert f"{ds.nearest_input_camera(int(q['spa'][0]), [int(c) for c in REF['inputs']]):02d}" == q["labels"][0][1]


def test_the_real_ops_call_refuses_host_tensors():
    q = REF["queries"]["spatial_down"]
    with pytest.raises(L.Dm4dError, match="HIP device"):
        dataset(**q["kw"]).get_item(SCENE, q["spa"], q["tem"], REF["inputs"])


# -- 3. error cases ------------------------------------------------------------------------------------------------------------
@pytest.fixture
def scene_copy(tmp_path):
    shutil.copytree(SCENE_DIR, tmp_path / "scene")
    return tmp_path / "scene"


SPA = ["00", "01", "02", "03"]


def test_missing_file(scene_copy, standin):
    (scene_copy / SCENE / "images" / "02" / "000001.webp").unlink()
    with pytest.raises(FileNotFoundError):
        dataset(scene_copy, height=64, width=64).get_item(SCENE, SPA, ["000001"], REF["inputs"])


def test_bad_mode_is_refused_not_converted(scene_copy, standin):
    p = scene_copy / SCENE / "fmasks" / "02" / "000001.png"
    Image.open(p).convert("1").save(p)
    with pytest.raises(ValueError, match=r"000001\.png.*mode '1'"):
        dataset(scene_copy, height=64, width=64).get_item(SCENE, SPA, ["000001"], REF["inputs"])
    p = scene_copy / SCENE / "images" / "03" / "000001.webp"
    Image.open(p).convert("RGBA").save(p, format="PNG")  # Pillow opens by content, not by name
    with pytest.raises(ValueError, match="mode 'RGBA'"):
        dataset(scene_copy, height=64, width=64).get_item(SCENE, ["03", "01"], ["000001"], REF["inputs"])


def test_sizes_that_differ(scene_copy, standin):
    p = scene_copy / SCENE / "skeletons" / "02" / "000001.webp"
    Image.open(p).resize((150, 200)).save(p, lossless=True)
    with pytest.raises(AssertionError, match=r"image size: \(160, 200\) != fmask size: \(160, 200\) != skeleton size: \(150, 200\)"):
        dataset(scene_copy, height=64, width=64).get_item(SCENE, SPA, ["000001"], REF["inputs"])


def test_input_mask_below_two_percent(scene_copy, standin):
    p = scene_copy / SCENE / "fmasks" / "01" / "000001.png"
    m = np.zeros((200, 160), np.uint8)
    m[50:60, 50:60] = 255  # 100 px of 32000: 0.3 %
    Image.fromarray(m).save(p)
    with pytest.raises(AssertionError, match="foreground mask < 2%"):
        dataset(scene_copy, height=64, width=64).get_item(SCENE, SPA, ["000001"], REF["inputs"])
    # the same mask on a target camera is accepted (the check is for input cameras only)
    dataset(scene_copy, height=64, width=64).get_item(SCENE, SPA, ["000001"], ["05"])


def test_easyvolcap_cameras_are_named_not_parsed(tmp_path):
    (tmp_path / "cams").mkdir()
    with pytest.raises(NotImplementedError, match="EasyVolcap"):
        capture.SpaTemDataset(data_dir=str(tmp_path), camera_path_pat="{data_dir}/cams", scene_label="s")
    with pytest.raises(NotImplementedError, match="EasyVolcap"):
        capture.read_cameras(str(tmp_path / "intri.yml"))


def test_global_intrinsics_fallback_and_norm():
    tfs = json.loads((SCENE_DIR / SCENE / "transforms.json").read_text())
    cams = capture.read_cameras(str(SCENE_DIR / SCENE / "transforms.json"))
    odd = cams["01"]["K"]
    assert float(odd[0, 0]) == tfs["fl_x"] and float(odd[1, 2]) == tfs["cy"]
    pos = torch.stack([c["pose"][:3, 3] for c in cams.values()])
    ext = pos.max(0).values - pos.min(0).values
    assert abs(float(torch.linalg.norm(ext)) - 1.0) < 1e-6  # the bounding box of the positions has unit diagonal


# -- 4. the CLI resolves the dataset without the reference checkout ---------------------------------------------------------------
def test_config_resolves_to_the_native_dataset():
    from diffuman4d_amd.host.config import compose, instantiate
    cfg = compose(["exp=demo_3d", f"data.data_dir={SCENE_DIR}", f"data.scene_label={SCENE}", "data.height=64", "data.width=64"])
    ds = instantiate(cfg["data"])
    assert type(ds) is capture.SpaTemDataset
    assert ds.image_path_pat.endswith("/images/{spa_label}/{tem_label}.webp") and sorted(ds.cameras[SCENE]) == sorted(REF["cameras"])


# -- 5. ABI: argument errors before the device is touched -------------------------------------------------------------------------
P = 0x10000


def test_capture_entry_rejects_bad_arguments():
    lib = L.load()
    f = lib.dm4d_capture_crop_resize_f32
    last = lambda: lib.dm4d_last_error().decode()
    H = W = 8
    bounds = np.tile(np.array([0, 1], np.int32), H)
    tab = np.concatenate([bounds, np.full(H, 1 << 22, np.int32)])  # 8 outputs, ksize 1, window [0, 1)
    desc = np.array([[0, 300, 400, 10, 10, 0, 0, 8, 8, 0, 1, 0, 1, 0, 0, 1]], np.int64)

    def args(d=desc, t=tab, staging=1024, scratch=1 << 20, w=W):
        return (None, P, staging, d.ctypes.data, P, 1, t.ctypes.data, P, t.size, P, scratch, P, P, H, w)
    assert f(None, None, 1024, desc.ctypes.data, P, 1, tab.ctypes.data, P, tab.size, P, 1 << 20, P, P, H, W) == -1
    assert "null pointer" in last()
    assert f(*args(w=6)) == -1 and "multiple of 4" in last()
    assert f(*args(staging=500)) == -1 and "staging buffer" in last()
    bad = desc.copy()
    bad[0, 9] = 1000
    assert f(*args(d=bad)) == -1 and "coefficient table" in last()
    bad_tab = tab.copy()
    bad_tab[2 * 3] = 8  # a window [8, 9) outside a crop of 8 columns
    assert f(*args(t=bad_tab)) == -1 and "coefficient table" in last()
    # ksize one above this entry's limit of 1 << 16, everything else in order: a horizontal table of 8 windows [0, 1) with room
    # for its 8 x 65537 weights, then the vertical table as before
    k = (1 << 16) + 1
    wide_tab = np.concatenate([bounds, np.zeros(W * k, np.int32), tab])
    wide = desc.copy()
    wide[0, 10], wide[0, 11] = k, 2 * W + W * k
    assert f(*args(d=wide, t=wide_tab)) == -1 and "coefficient table" in last()
    assert f(*args(scratch=16)) == -1 and "scratch region" in last()
    bad = desc.copy()
    bad[0, 15] = 9  # more scratch rows than the crop has
    assert f(*args(d=bad)) == -1 and "scratch row range" in last()
