"""CPU: SpaTemDataset(skeleton_source="kp2d") (diffuman4d_amd/host/capture.py) against the file route on the same scene with lossless
skeleton files.  The three device entries are replaced by numpy stand-ins that read and write the same staging buffer: tests/skel_model.py
for the draw, kp2d_scene.rect_model for the box and mask, tests/capture_model.py for the crop and resize."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import capture_model as cm
import kp2d_scene as ks
from diffuman4d_amd.host import capture, skeleton

PALETTE = skeleton.load_palette(ks.PALETTE_PATH)
HW = ks.SIZES[0]
OUT = 64


@pytest.fixture(scope="module")
def scene_root(tmp_path_factory):
    root = tmp_path_factory.mktemp("kp2d_cpu")
    scene = ks.write_cameras_and_detections(root, HW)
    ks.detections_as_poses_2d(scene)
    ks.write_images_and_masks(scene, HW)
    ks.write_skeleton_pngs(scene, HW, PALETTE, ks.model_draw)
    return root


@pytest.fixture
def standin(monkeypatch):
    """-> the list of (staging bytes, descriptors) of every crop-resize call."""
    calls = []

    def crop_resize(blob, blob_host, n_frames, desc_off, tab_off, tab_len, H, W, meta=None):
        if meta is None:  # the file route: one buffer
            return cm.standin_crop_resize(blob, blob_host, n_frames, desc_off, tab_off, tab_len, H, W)
        assert torch.equal(meta, blob_host)
        desc = blob_host.numpy()[desc_off: desc_off + n_frames * capture.FIELDS * 8].view(np.int64).reshape(n_frames, capture.FIELDS)
        calls.append((blob.numel(), desc.copy()))
        both = torch.cat([blob, blob_host])  # the model reads planes and descriptors from one buffer: the device's planes, then meta
        return cm.standin_crop_resize(both, both, n_frames, blob.numel() + desc_off, blob.numel() + tab_off, tab_len, H, W)
    monkeypatch.setattr(capture.ops, "capture_crop_resize", crop_resize)
    monkeypatch.setattr(capture.ops, "skeleton_draw", ks.standin_skeleton_draw)
    monkeypatch.setattr(capture.ops, "skeleton_box_mask", ks.standin_box_mask, raising=False)
    return calls


def dataset(root, **kw):
    return capture.SpaTemDataset(data_dir=str(root), scene_label=ks.SCENE, device="cpu", decode_threads=4, height=OUT, width=OUT,
                                 **{**ks.patterns(), **kw})


def same(a, b):
    assert a["domain"] == b["domain"] and a["labels"] == b["labels"] and a["hws"] == b["hws"] and a["crops"] == b["crops"]
    for k in ("pixel_values", "skeletons", "Ks", "poses", "cond_masks", "plucker_embeds"):
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("has_gt_target", [True, False])
@pytest.mark.parametrize("task", ["spatial", "temporal"])
def test_kp2d_equals_the_file_route_on_lossless_maps(scene_root, standin, task, has_gt_target):
    spa, tem = ks.TASKS[task]
    want = dataset(scene_root, has_gt_target=has_gt_target).get_item(ks.SCENE, spa, tem, ks.INPUTS)
    got = dataset(scene_root, has_gt_target=has_gt_target, skeleton_source="kp2d", palette=PALETTE).get_item(ks.SCENE, spa, tem, ks.INPUTS)
    same(got, want)
    assert want["skeletons"].max() > -1.0  # something is drawn
    top, left, ch, cw = want["crops"][ks.CAMS.index(ks.BORDER_CAM) if task == "spatial" else 0][:4]
    if task == "spatial" and has_gt_target:
        assert left < 0  # the border camera's crop leaves the image


def test_kp2d_needs_no_skeleton_directory(scene_root, standin):
    ds = dataset(scene_root, has_gt_target=False, skeleton_source="kp2d", palette=str(ks.PALETTE_PATH),
                 skeleton_path_pat="{data_dir}/{scene_label}/nowhere/{spa_label}/{tem_label}.png")
    want = dataset(scene_root, has_gt_target=False).get_item(ks.SCENE, *ks.TASKS["spatial"], ks.INPUTS)
    same(ds.get_item(ks.SCENE, *ks.TASKS["spatial"], ks.INPUTS), want)


def test_score_override_and_canvas_shape(scene_root, standin, tmp_path):
    """kp2d_score_path_pat replaces the scores file by file; kp2d_canvas_shape given explicitly equals the camera's."""
    rng = np.random.default_rng(3)
    scene = scene_root / ks.SCENE
    for cam in ks.CAMS:
        p = scene / "scores" / cam / "000000.json"
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_text(json.dumps({"instance_info": [{"keypoint_scores": rng.uniform(0.3, 1.0, 133).tolist()}]}))
    kw = dict(skeleton_source="kp2d", palette=PALETTE, kp2d_score_path_pat="{data_dir}/{scene_label}/scores/{spa_label}/{tem_label}.json")
    got = dataset(scene_root, kp2d_canvas_shape=list(HW), **kw).get_item(ks.SCENE, *ks.TASKS["spatial"], ks.INPUTS)
    plain = dataset(scene_root, skeleton_source="kp2d", palette=PALETTE).get_item(ks.SCENE, *ks.TASKS["spatial"], ks.INPUTS)
    assert not torch.equal(got["skeletons"], plain["skeletons"]) and torch.equal(got["pixel_values"], plain["pixel_values"])
    for f, cam in enumerate(ks.CAMS):
        p = ks.plan_of(scene, cam, "000000", HW, PALETTE, scores="scores")
        m = ks.model_draw([p])[0]
        crop = got["crops"][f][:4]
        assert torch.equal(got["skeletons"][f], cm.epilogue(m, m[..., 0], cm.crop_resize(m, *crop, OUT, OUT))[1]), cam


def test_staging_layout(scene_root, standin):
    """Skeleton planes are tight and start the device buffer, the targets' mask slots follow them, the planes that come from files lie
    behind both; a skeleton-only frame's image IS its skeleton plane."""
    spa, tem = ks.TASKS["spatial"]
    dataset(scene_root, has_gt_target=False, skeleton_source="kp2d", palette=PALETTE).get_item(ks.SCENE, spa, tem, ks.INPUTS)
    (dev_bytes, desc), = standin
    h, w = HW
    skel = np.sort(desc[:, 2])
    assert skel[0] == 0 and (np.diff(skel) == h * w * 3).all()
    targets = np.array([cam not in ks.INPUTS for cam in spa])
    assert (desc[targets, 0] == desc[targets, 2]).all() and desc[targets, 2].max() < desc[~targets, 2].min()  # the targets come first
    masks = np.sort(desc[targets, 1])
    device_only = masks[-1] + h * w
    assert masks[0] == skel[-1] + h * w * 3 and (np.diff(masks) == h * w).all()
    files = np.sort(np.concatenate([desc[~targets, 0], desc[~targets, 1]]))
    assert files[0] == -(-device_only // 16) * 16 and files[-1] + h * w <= dev_bytes < files[-1] + h * w + 16
    assert (desc[:, 3] == h).all() and (desc[:, 4] == w).all()
    # with images for every frame there is no slot
    standin.clear()
    dataset(scene_root, skeleton_source="kp2d", palette=PALETTE).get_item(ks.SCENE, spa, tem, ks.INPUTS)
    (dev_bytes, desc), = standin
    assert np.sort(desc[:, 2])[-1] + h * w * 3 == np.concatenate([desc[:, 0], desc[:, 1]]).min() == len(spa) * h * w * 3


def test_files_mode_with_the_new_keywords_at_their_defaults(scene_root, standin):
    spa, tem = ks.TASKS["temporal"]
    a = capture.SpaTemDataset(data_dir=str(scene_root), scene_label=ks.SCENE, device="cpu", height=OUT, width=OUT, **ks.patterns())
    b = dataset(scene_root, skeleton_source="files", kp2d_path_pat=capture.KP2D_PATH_PAT, kp2d_score_path_pat=None, kp2d_canvas_shape=None,
                palette=None)
    assert b.palette is None
    same(a.get_item(ks.SCENE, spa, tem, ks.INPUTS), b.get_item(ks.SCENE, spa, tem, ks.INPUTS))


# -- errors -------------------------------------------------------------------------------------------------------------------------
def test_unknown_source_and_missing_palette(scene_root):
    with pytest.raises(ValueError, match="skeleton_source must be one of"):
        dataset(scene_root, skeleton_source="poses_3d")
    with pytest.raises(ValueError, match="load_palette"):
        dataset(scene_root, skeleton_source="kp2d")


def small_scene(tmp_path, hw):
    scene = ks.write_cameras_and_detections(tmp_path, hw)
    ks.detections_as_poses_2d(scene)
    return scene


def test_a_map_below_256_pixels_is_refused(tmp_path, standin):
    small_scene(tmp_path, (200, 160))
    ds = dataset(tmp_path, has_gt_target=False, skeleton_source="kp2d", palette=PALETTE)
    with pytest.raises(ValueError) as e:
        ds.get_item(ks.SCENE, *ks.TASKS["spatial"], ks.INPUTS[:0])
    with pytest.raises(ValueError) as want:
        skeleton._check_out_shape((200, 160))
    assert str(e.value) == str(want.value)


def test_an_empty_map_for_a_skeleton_only_target(tmp_path, standin):
    scene = small_scene(tmp_path, HW)
    p = scene / "poses_2d" / "06" / "000000.json"
    inst = ks.instance(scene, "06", "000000")
    p.write_text(json.dumps({"instance_info": [dict(inst, keypoint_scores=[0.2] * 133)]}))  # no link reaches the threshold
    ds = dataset(tmp_path, has_gt_target=False, skeleton_source="kp2d", palette=PALETTE)
    with pytest.raises(ValueError, match=r"skeleton is empty, no mask can be made from it: .*poses_2d/06/000000\.json"):
        ds.get_item(ks.SCENE, *ks.TASKS["spatial"], ks.CAMS[:0])


@pytest.mark.parametrize("hw,map_size", [((320, 256), (255, 320)), ((257, 250), (249, 257))])
def test_a_size_the_drawing_does_not_reproduce_fails_the_size_check_in_both_routes(tmp_path, standin, hw, map_size):
    """The reference's canvas rounding (kp2d_scene's docstring): at these sizes the map is a pixel narrower than the image, and the
    dataset refuses the frame with the same words whether the map comes from a file or is drawn."""
    scene = small_scene(tmp_path, hw)
    ks.write_images_and_masks(scene, hw)
    ks.write_skeleton_pngs(scene, hw, PALETTE, ks.model_draw)
    text = rf"image size: \({hw[1]}, {hw[0]}\) != fmask size: \({hw[1]}, {hw[0]}\) != skeleton size: \({map_size[0]}, {map_size[1]}\)"
    for kw in ({}, {"skeleton_source": "kp2d", "palette": PALETTE}):
        with pytest.raises(AssertionError, match=text):
            dataset(tmp_path, **kw).get_item(ks.SCENE, ["03"], ks.FRAMES, ks.INPUTS)


# -- config -------------------------------------------------------------------------------------------------------------------------
def test_config_resolves_kp2d_to_the_native_class(scene_root, monkeypatch):
    import sys
    import types
    from diffuman4d_amd.host import config
    base = ["exp=demo_3d", f"data.data_dir={scene_root}", f"data.scene_label={ks.SCENE}", "data.height=64", "data.width=64"]
    cfg = config.compose(base + ["data.skeleton_source=kp2d", f"data.palette={ks.PALETTE_PATH}", "data.kp2d_canvas_shape=[320,255]",
                                 "data.kp2d_path_pat='{data_dir}/{scene_label}/poses_2d/{spa_label}/{tem_label}.json'",
                                 "data.kp2d_score_path_pat=null"])
    assert cfg["data"]["skeleton_source"] == "kp2d" and cfg["data"]["kp2d_canvas_shape"] == [320, 255]

    class Reference:  # a reference class that imports, and does not know the keyword
        def __init__(self, data_dir, camera_path_pat=None, image_path_pat=None, fmask_path_pat=None, skeleton_path_pat=None,
                     scene_label=None, height=1024, width=1024, has_gt_target=True):
            pass
    for name in ("src", "src.data"):
        monkeypatch.setitem(sys.modules, name, types.ModuleType(name))
    mod = types.ModuleType("src.data.spatem_dataset")
    mod.SpaTemDataset = Reference
    monkeypatch.setitem(sys.modules, "src.data.spatem_dataset", mod)
    ds = config.instantiate(cfg["data"])
    assert type(ds) is capture.SpaTemDataset and ds.skeleton_source == "kp2d" and ds.kp2d_canvas_shape == (320, 255)
    assert ds.palette == PALETTE and ds.kp2d_score_path_pat is None
    # without the key, and with the default, the resolution is what it was: the reference's class wins where it imports
    assert type(config.instantiate(config.compose(base)["data"])) is Reference
    assert config.locate("src.data.spatem_dataset.SpaTemDataset", native=False) is Reference
    # the new keys at their defaults ask for nothing new: the reference's class is taken and is not handed them
    defaults = ["data.skeleton_source=files", "data.palette=null", "data.kp2d_score_path_pat=null", "data.kp2d_canvas_shape=null",
                "data.kp2d_path_pat='{data_dir}/{scene_label}/poses_2d/{spa_label}/{tem_label}.json'"]
    assert type(config.instantiate(config.compose(base + defaults)["data"])) is Reference
    assert type(config.instantiate(config.compose(base + defaults[:1])["data"])) is Reference
    # any of them set selects the native class, which then says what is missing
    with pytest.raises(ValueError, match="load_palette"):
        config.instantiate(config.compose(base + ["data.skeleton_source=kp2d"])["data"])
    ds = config.instantiate(config.compose(base + [f"data.palette={ks.PALETTE_PATH}"])["data"])
    assert type(ds) is capture.SpaTemDataset and ds.skeleton_source == "files"
    monkeypatch.delitem(sys.modules, "src.data.spatem_dataset")  # the reference does not import: the native class takes the defaults too
    monkeypatch.setitem(sys.modules, "src.data.spatem_dataset", None)
    assert type(config.instantiate(config.compose(base + defaults)["data"])) is capture.SpaTemDataset
    monkeypatch.setitem(sys.modules, "src.data.spatem_dataset", mod)
    assert config.locate("src.data.spatem_dataset.SpaTemDataset") is Reference
    for data in ("dna_rendering", "fdvai"):
        cfg = config.compose(["exp=demo_3d", f"data={data}", "data.skeleton_source=kp2d", f"data.palette={ks.PALETTE_PATH}"])
        assert config.locate(cfg["data"]["_target_"], native=True) is capture.SpaTemDataset and cfg["data"]["skeleton_source"] == "kp2d"


# -- the rectangle identity ---------------------------------------------------------------------------------------------------------
def random_maps():
    rng = np.random.default_rng(2024)
    out = []
    for n in range(200):
        h, w = (1, 1) if n == 0 else (300, 300) if n == 1 else (int(v) for v in rng.integers(1, 301, 2))
        m = np.zeros((h, w, 3), np.uint8)
        kind = n % 5
        if kind == 0:  # one pixel
            m[rng.integers(h), rng.integers(w), rng.integers(3)] = rng.integers(1, 256)
        elif kind == 1:  # blue-only pixels
            for _ in range(int(rng.integers(1, 6))):
                m[rng.integers(h), rng.integers(w), 2] = rng.integers(1, 256)
        elif kind == 2:  # one corner after the other, then all four
            corners = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)]
            for y, x in (corners if (n // 5) % 5 == 4 else [corners[(n // 5) % 4]]):
                m[y, x] = rng.integers(1, 256, 3)
        elif kind == 3:  # a blob
            y0, x0 = rng.integers(h), rng.integers(w)
            m[y0: y0 + rng.integers(1, 40), x0: x0 + rng.integers(1, 40)] = rng.integers(0, 256, 3)
            m[y0, x0, 0] = 7
        else:  # sparse noise, values down to 1
            hit = rng.random((h, w)) < 0.01
            m[hit] = rng.integers(0, 3, (int(hit.sum()), 3))
            m[rng.integers(h), rng.integers(w), 1] = 1
        out.append(m)
    return out


def test_the_rectangle_model_is_skeleton_mask():
    for m in random_maps():
        h, w = m.shape[:2]
        want = capture.skeleton_mask(m)
        boxes, masks = ks.rect_model(m[None], capture.skeleton_mask_pads(h, w))
        assert np.array_equal(masks[0], want), (h, w)
        c0, r0, c1, r1 = capture.skeleton_mask_rect(boxes[0], h, w)
        rect = np.zeros((h, w), np.uint8)
        rect[r0:r1, c0:c1] = 255
        assert np.array_equal(rect, want)
        assert capture._crop_from_bbox((c0 - 1, r0 - 1, c1, r1), h, w) == capture.crop_box(want)
    boxes, masks = ks.rect_model(np.zeros((1, 9, 7, 3), np.uint8), (3, 1, 1))
    assert boxes.tolist() == [[7, 9, -1, -1]] and not masks.any()


# -- ABI: argument errors before the device is touched ------------------------------------------------------------------------------
def test_box_mask_entry_rejects_bad_arguments_and_there_is_no_cpu_path():
    from diffuman4d_amd.host import lib as L, ops
    lib = L.load()
    f, ws = lib.dm4d_skeleton_box_mask_u8, lib.dm4d_skeleton_box_mask_ws_bytes
    last = lambda: lib.dm4d_last_error().decode()
    P = 0x10000
    assert ws(3, 257, 250) == 3 * 6 * 16  # a 192 750-byte frame: six blocks of 32 KiB, four int32 each
    assert ws(1, 8192, 8192) == 256 * 16 and ws(1, 1, 1) == 16
    assert ws(0, 4, 4) == 0 and ws(1, 1 << 16, 4) == 0 and ws(1, 4, 0) == 0

    def args(maps=P, n=1, h=4, w=4, pads=(0, 0, 0), boxes=P, masks=P, stride=16, wsp=P, ws_bytes=1 << 20):
        return (None, maps, n, h, w, *pads, boxes, masks, stride, wsp, ws_bytes)
    assert f(*args(maps=None)) == -1 and "null pointer" in last()
    assert f(*args(n=0)) == -1 and "shape" in last()
    assert f(*args(w=(1 << 15) + 1)) == -1 and "shape" in last()
    assert f(*args(pads=(0, -1, 0))) == -1 and "padding" in last()
    assert f(*args(stride=15)) == -1 and "mask_stride" in last()
    assert f(*args(boxes=P + 2)) == -1 and "4-byte aligned" in last()
    assert f(*args(ws_bytes=15)) == -1 and "workspace" in last()
    with pytest.raises(L.Dm4dError, match="HIP device"):
        ops.skeleton_box_mask(torch.zeros((1, 4, 4, 3), dtype=torch.uint8), (0, 0, 0))
