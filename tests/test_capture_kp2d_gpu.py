"""GPU: dm4d_skeleton_box_mask_u8 against the rectangle model byte for byte, and SpaTemDataset(skeleton_source="kp2d") against the file
route on a scene whose skeleton files hold the drawn maps losslessly, against the numpy models of draw, box and resize, with the draw
cut into several launches, and through tools/capture_bench.py."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import capture_model as cm
import kp2d_scene as ks
from diffuman4d_amd.host import capture, ops, skeleton, triang

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
PALETTE = skeleton.load_palette(ks.PALETTE_PATH)
OUT = 64


# tests/test_capture_gpu.py's _HostTensors swaps capture.ops.capture_crop_resize for the host model around every get_item (read, set,
# restore, without a lock); when the runner loads two tasks at once the second call reads the model as "the real one" and restores it
# last, and the host model stays installed for the rest of the process.  The tests here are about the device entries: every one of them
# runs with the wrappers this module saw when it was imported, which is before any test ran.
GENUINE = {name: getattr(ops, name) for name in ("capture_crop_resize", "skeleton_draw", "skeleton_box_mask")}
assert all(f.__module__ == ops.__name__ for f in GENUINE.values())


@pytest.fixture(autouse=True)
def genuine_ops(monkeypatch):
    for name, f in GENUINE.items():
        monkeypatch.setattr(ops, name, f)


# -- the entry ------------------------------------------------------------------------------------------------------------------------
def box_mask(dev, maps: np.ndarray, pads, shift: int = 0):
    """ops.skeleton_box_mask on maps that start `shift` bytes into a buffer, masks likewise (the dataset's planes are not aligned)."""
    n, h, w, _ = maps.shape
    buf = torch.zeros(shift + maps.size, dtype=torch.uint8, device=dev)
    buf[shift:] = torch.from_numpy(maps.reshape(-1)).to(dev)
    mbuf = torch.full((shift + n * h * w + 32,), 77, dtype=torch.uint8, device=dev)
    boxes, masks = ops.skeleton_box_mask(buf[shift:].view(n, h, w, 3), pads, masks=mbuf[shift: shift + n * h * w].view(n, h, w))
    assert (mbuf[:shift] == 77).all() and (mbuf[shift + n * h * w:] == 77).all()  # nothing outside the slots is written
    return boxes.cpu().numpy(), masks.cpu().numpy()


def check(dev, maps, pads=None, shifts=(0, 5)):
    n, h, w, _ = maps.shape
    pads = capture.skeleton_mask_pads(h, w) if pads is None else pads
    want_boxes, want_masks = ks.rect_model(maps, pads)
    for shift in shifts:
        boxes, masks = box_mask(dev, maps, pads, shift)
        assert boxes.tolist() == want_boxes.tolist(), (shift, boxes.tolist(), want_boxes.tolist())
        assert np.array_equal(masks, want_masks), shift
    return want_boxes, want_masks


def test_box_mask_one_pixel_maps(hip_device):
    zero, one = np.zeros((1, 1, 1, 3), np.uint8), np.zeros((1, 1, 1, 3), np.uint8)
    one[0, 0, 0, 1] = 9
    boxes, masks = check(hip_device, zero, shifts=(0, 1, 15))
    assert boxes.tolist() == [[1, 1, -1, -1]] and not masks.any()
    boxes, masks = check(hip_device, one, shifts=(0, 1, 15))
    assert boxes.tolist() == [[0, 0, 0, 0]] and masks.tolist() == [[[255]]]


def test_box_mask_a_blue_only_pixel_in_the_last_column(hip_device):
    m = np.zeros((1, 5, 7, 3), np.uint8)  # 21-byte rows
    m[0, 3, 6, 2] = 1
    boxes, _ = check(hip_device, m, pads=(1, 0, 2), shifts=(0, 3, 11))
    assert boxes.tolist() == [[6, 3, 6, 3]]
    check(hip_device, m)


def corner_maps():
    m = np.zeros((3, 257, 250, 3), np.uint8)  # 750-byte rows, a 192 750-byte frame: neither a multiple of 4 or of 16
    m[0, 0, 249, 0] = 255     # top right ...
    m[0, 200, 3, 2] = 1       # ... and low left
    m[2, 256, 0, 1] = 4       # bottom left ...
    m[2, 10, 249, 2] = 200    # ... and high right; frame 1 stays empty
    return m


def test_box_mask_unaligned_frames_with_an_empty_one_in_the_middle(hip_device):
    m = corner_maps()
    boxes, masks = check(hip_device, m, shifts=(0, 7))
    assert boxes.tolist() == [[3, 0, 249, 200], [250, 257, -1, -1], [0, 10, 249, 256]] and not masks[1].any() and masks[0].any()


def test_box_mask_the_last_pixel_of_a_large_map(hip_device):
    m = np.zeros((1, 1024, 1024, 3), np.uint8)
    m[0, 1023, 1023, 2] = 1
    boxes, masks = check(hip_device, m, shifts=(0,))
    assert boxes.tolist() == [[1023, 1023, 1023, 1023]]
    assert masks[0, 1023 - 1 - 90:, 1023 - 1 - 30:].all() and int((masks != 0).sum()) == 92 * 32


def test_box_mask_padding_clamped_at_all_four_borders(hip_device):
    m = np.zeros((1, 100, 120, 3), np.uint8)
    m[0, 2, 1, 0] = 1
    m[0, 98, 118, 1] = 1
    _, masks = check(hip_device, m)  # pads (9, 3, 3)
    assert masks.all()
    _, masks = check(hip_device, m, pads=(0, 0, 0))
    assert masks[0, 1:99, 0:119].all() and not masks[0, 0].any() and not masks[0, 99].any() and not masks[0, :, 119].any()


def test_box_mask_a_frame_alone_equals_the_frame_in_the_batch_and_two_runs_agree(hip_device):
    rng = np.random.default_rng(11)
    m = np.zeros((4, 300, 260, 3), np.uint8)
    for f in range(4):
        y, x = rng.integers(20, 280), rng.integers(20, 240)
        m[f, y: y + rng.integers(1, 20), x: x + rng.integers(1, 20)] = rng.integers(0, 256, 3)
        m[f, y, x, 0] = 1
    pads = capture.skeleton_mask_pads(300, 260)
    boxes, masks = box_mask(hip_device, m, pads)
    again = box_mask(hip_device, m, pads)
    assert np.array_equal(boxes, again[0]) and np.array_equal(masks, again[1])
    for f in range(4):
        b1, m1 = box_mask(hip_device, m[f: f + 1], pads, shift=f)
        assert np.array_equal(b1[0], boxes[f]) and np.array_equal(m1[0], masks[f])
    check(hip_device, m)


def test_box_mask_refuses_what_it_cannot_take(hip_device):
    from diffuman4d_amd.host import lib as L
    maps = torch.zeros((1, 4, 4, 3), dtype=torch.uint8, device=hip_device)
    with pytest.raises(L.Dm4dError, match="masks"):
        ops.skeleton_box_mask(maps, (0, 0, 0), masks=torch.zeros((1, 4, 5), dtype=torch.uint8, device=hip_device))
    with pytest.raises(L.Dm4dError, match="padding"):
        ops.skeleton_box_mask(maps, (-1, 0, 0))
    with pytest.raises(L.Dm4dError, match="HIP device"):
        ops.skeleton_box_mask(maps.cpu(), (0, 0, 0))


# -- the whole route ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scenes(hip_device, tmp_path_factory):
    """One scene per size of kp2d_scene.SIZES: poses_2d written by the native triangulate_skeleton, skeleton PNGs by the native draw."""
    roots = []
    for hw in ks.SIZES:
        root = tmp_path_factory.mktemp(f"kp2d_{hw[0]}x{hw[1]}")
        d = ks.write_cameras_and_detections(root, hw)
        triang.triangulate_skeleton(str(d / "transforms.json"), str(d / "poses_sapiens"), str(d / "poses_3d"),
                                    out_kp2d_proj_dir=str(d / "poses_2d"), spa_labels_proj=list(range(8)))
        ks.write_images_and_masks(d, hw)
        ks.write_skeleton_pngs(d, hw, PALETTE, skeleton.draw_plans)
        roots.append(root)
    return roots


def dataset(root, **kw):
    return capture.SpaTemDataset(data_dir=str(root), scene_label=ks.SCENE, height=OUT, width=OUT, decode_threads=4,
                                 **{**ks.patterns(), **kw})


def same(a, b):
    assert a["domain"] == b["domain"] and a["labels"] == b["labels"] and a["hws"] == b["hws"] and a["crops"] == b["crops"]
    for k in ("pixel_values", "skeletons", "Ks", "poses", "cond_masks", "plucker_embeds"):
        assert torch.equal(a[k], b[k]), (k, where(a[k], b[k]))


def where(a, b):
    """What differs between two [n, c, H, W] tensors: per frame the count, the rows and the columns of the differing elements."""
    d = (a != b).cpu()
    out = {"elements": int(d.sum()), "max_abs": float((a - b).abs().max())}
    for f in range(d.shape[0]):
        if d[f].any() and d.dim() == 4:
            rows, cols = d[f].any(dim=0).any(dim=1).nonzero().flatten(), d[f].any(dim=0).any(dim=0).nonzero().flatten()
            out[f] = (int(d[f].sum()), [int(rows[0]), int(rows[-1])], [int(cols[0]), int(cols[-1])], d[f].flatten(1).any(dim=1).tolist())
    return out


@pytest.mark.parametrize("size,task,has_gt_target", [(0, "spatial", True), (0, "spatial", False), (0, "temporal", True),
                                                      (0, "temporal", False), (1, "spatial", True), (1, "spatial", False)])
def test_kp2d_equals_the_file_route_on_lossless_maps(scenes, size, task, has_gt_target):
    spa, tem = ks.TASKS[task]
    want = dataset(scenes[size], has_gt_target=has_gt_target).get_item(ks.SCENE, spa, tem, ks.INPUTS)
    got = dataset(scenes[size], has_gt_target=has_gt_target, skeleton_source="kp2d", palette=PALETTE).get_item(ks.SCENE, spa, tem, ks.INPUTS)
    same(got, want)
    assert got["pixel_values"].is_cuda and got["skeletons"].max() > -1.0


def test_kp2d_against_the_models_of_draw_box_and_resize(scenes):
    """Without the file route: one frame's skeletons row is the modelled map, cropped and resized by the model; a skeleton-only frame's
    pixel_values are the same model fed with the rectangle mask."""
    hw = ks.SIZES[0]
    spa, tem = ks.TASKS["spatial"]
    got = dataset(scenes[0], has_gt_target=False, skeleton_source="kp2d", palette=PALETTE).get_item(ks.SCENE, spa, tem, ks.INPUTS)
    for f in (spa.index(ks.INPUTS[0]), spa.index("06")):
        plan = ks.plan_of(scenes[0] / ks.SCENE, spa[f], tem[0], hw, PALETTE)
        m = skeleton_map = ks.model_draw([plan])[0]
        crop = got["crops"][f][:4]
        if spa[f] in ks.INPUTS:
            from PIL import Image
            img = np.asarray(Image.open(scenes[0] / ks.SCENE / "images" / spa[f] / f"{tem[0]}.png"))
            mask = np.asarray(Image.open(scenes[0] / ks.SCENE / "fmasks" / spa[f] / f"{tem[0]}.png"))
        else:
            img, mask = skeleton_map, ks.rect_model(m[None], capture.skeleton_mask_pads(*hw))[1][0]
            assert capture.crop_box(mask)[:4] == list(crop)
        args = (*crop, OUT, OUT)
        pix, sk = cm.epilogue(cm.crop_resize(img, *args), cm.crop_resize(mask, *args), cm.crop_resize(m, *args))
        assert torch.equal(got["skeletons"][f].cpu(), sk), spa[f]
        assert torch.equal(got["pixel_values"][f].cpu(), pix), spa[f]


def test_a_task_cut_into_several_draw_launches(scenes, monkeypatch):
    spa, tem = ks.TASKS["spatial"]
    ds = dataset(scenes[0], has_gt_target=False, skeleton_source="kp2d", palette=PALETTE)
    want = ds.get_item(ks.SCENE, spa, tem, ks.INPUTS)
    h, w = ks.SIZES[0]
    monkeypatch.setattr(skeleton, "LAUNCH_BYTES", 2 * h * w * 3)  # two maps a launch: eight frames take four
    launches = []
    real = ops.skeleton_draw
    monkeypatch.setattr(ops, "skeleton_draw", lambda *a, **k: launches.append(a[2].numel() - 1) or real(*a, **k))
    same(ds.get_item(ks.SCENE, spa, tem, ks.INPUTS), want)
    assert launches == [2, 2, 2, 2]


def test_the_bench_tool_runs_the_route(hip_device, tmp_path):
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "capture_bench.py"), "--src", "256x256", "--out", "64", "--frames", "2",
                        "--skeleton-source", "kp2d", "--palette", str(ks.PALETTE_PATH), "--no-gt-target", "--dir", str(tmp_path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    for task, frames in (("spatial", 48), ("temporal", 4)):
        row = res[task]
        assert row["frames"] == frames and row["skeleton_source"] == "kp2d" and row["has_gt_target"] is False
        assert all(k in row for k in ("read_kp2d_s", "plan_s", "draw_kernel_s", "box_mask_kernel_s", "decode_s", "kernel_s", "get_item_s"))
        assert row["draw_kernel_s"] > 0 and row["box_mask_kernel_s"] > 0
