"""Test-side builder of a small captured scene with keypoint files, for SpaTemDataset(skeleton_source="kp2d")
(tests/test_capture_kp2d_cpu.py, tests/test_capture_kp2d_gpu.py), and the numpy models those tests share.

The scene is tests/golden/triang_scene/ring8 (8 cameras on a ring, 2 frames, 133-keypoint detections on a 1024 x 1024 grid) brought to
a camera size of (h, w): intrinsics and detections are scaled per axis.  Images and masks are synthetic and deterministic, saved as PNG;
the skeleton files are PNG too, so that the file route reads exactly the maps that were drawn.

Map sizes.  The reference paints on a canvas of int(s * 2048 / max(h, w)) pixels per side and reduces it to int(canvas / (2048 /
max(h, w))): for most non-square sizes the map comes out one pixel short of the size asked for ((320, 256) gives 320 x 255, (257, 250)
gives 257 x 249) and the dataset's size check refuses the frame -- in the file route and in the "kp2d" route alike.  SIZES are sizes
the drawing reproduces (s * 2048 / max(h, w) is an integer, as for every square), one with rows that are no multiple of 4 bytes and an
odd square whose tight planes start on odd addresses."""
import json
import shutil
from pathlib import Path

import numpy as np
import torch
from PIL import Image

import skel_model
from diffuman4d_amd.host import skeleton

GOLDEN = Path(__file__).resolve().parent / "golden"
RING8 = GOLDEN / "triang_scene" / "ring8"
PALETTE_PATH = GOLDEN / "skel_palette.json"
SCENE = "ring8"
CAMS = [f"{c:02d}" for c in range(8)]
FRAMES = ["000000", "000001"]
INPUTS = ["01", "05"]
SIZES = ((320, 255), (257, 257))  # (h, w): 765-byte rows; 771-byte rows and a 198 147-byte frame: planes that start on odd addresses
BORDER_CAM = "02"                 # its mask touches the left border: the crop leaves the image


def write_cameras_and_detections(root: Path, hw) -> Path:
    """ring8's transforms.json and poses_sapiens at the camera size hw -> the scene directory."""
    h, w = hw
    scene = root / SCENE
    scene.mkdir(parents=True)
    sx, sy = w / 1024, h / 1024
    tfs = json.loads((RING8 / "transforms.json").read_text())
    tfs["w"], tfs["h"] = w, h
    for fr in tfs["frames"]:
        fr.update(w=w, h=h, fl_x=fr["fl_x"] * sx, cx=fr["cx"] * sx, fl_y=fr["fl_y"] * sy, cy=fr["cy"] * sy)
    (scene / "transforms.json").write_text(json.dumps(tfs))
    for cam in CAMS:
        for frame in FRAMES:
            inst = json.loads((RING8 / "poses_sapiens" / cam / f"{frame}.json").read_text())["instance_info"][0]
            inst["keypoints"] = [[x * sx, y * sy] for x, y in inst["keypoints"]]
            p = scene / "poses_sapiens" / cam / f"{frame}.json"
            p.parent.mkdir(parents=True, exist_ok=True)
            p.write_text(json.dumps({"instance_info": [inst]}))
    return scene


def detections_as_poses_2d(scene: Path) -> None:
    """Without a device: every camera's own detections serve as its poses_2d."""
    shutil.copytree(scene / "poses_sapiens", scene / "poses_2d")


def instance(scene: Path, cam: str, frame: str, sub: str = "poses_2d"):
    return json.loads((scene / sub / cam / f"{frame}.json").read_text())["instance_info"][0]


def write_images_and_masks(scene: Path, hw) -> None:
    h, w = hw
    yy, xx = np.mgrid[:h, :w]
    for c, cam in enumerate(CAMS):
        for t, frame in enumerate(FRAMES):
            k = np.array(instance(scene, cam, frame, "poses_sapiens")["keypoints"])
            cx, cy = (0.08 * w, k[:, 1].mean()) if cam == BORDER_CAM else k.mean(axis=0)
            inside = ((xx - cx) / (0.2 * w)) ** 2 + ((yy - cy) / (0.4 * h)) ** 2 < 1
            img = np.stack([(xx * 3 + 20 * c) % 256, (yy * 2 + 37 * t) % 256, (xx + yy + 11 * c) % 256], -1).astype(np.uint8)
            for sub, arr in (("images", img), ("fmasks", np.where(inside, 255, 0).astype(np.uint8))):
                p = scene / sub / cam / f"{frame}.png"
                p.parent.mkdir(parents=True, exist_ok=True)
                Image.fromarray(arr).save(p)


def plan_of(scene: Path, cam: str, frame: str, hw, palette, scores: str = None):
    sc = None if scores is None else instance(scene, cam, frame, scores)
    return skeleton.plan_draw_calls(instance(scene, cam, frame), sc, (hw, hw), palette)


def write_skeleton_pngs(scene: Path, hw, palette, draw, scores: str = None) -> None:
    """skeletons/{cam}/{frame}.png = draw(plans)[k] (uint8 [n, h, w, 3]) for every frame's plan, lossless."""
    jobs = [(cam, frame) for cam in CAMS for frame in FRAMES]
    maps = draw([plan_of(scene, cam, frame, hw, palette, scores) for cam, frame in jobs])
    for (cam, frame), m in zip(jobs, maps):
        p = scene / "skeletons" / cam / f"{frame}.png"
        p.parent.mkdir(parents=True, exist_ok=True)
        Image.fromarray(np.asarray(m)).save(p)


def patterns() -> dict:
    """The dataset keywords that name this scene's PNG files."""
    return {"image_path_pat": "{data_dir}/{scene_label}/images/{spa_label}/{tem_label}.png",
            "skeleton_path_pat": "{data_dir}/{scene_label}/skeletons/{spa_label}/{tem_label}.png"}


TASKS = {"spatial": (CAMS, FRAMES[:1]), "temporal": (["03"], FRAMES)}


# -- models -------------------------------------------------------------------------------------------------------------------------
def rect_model(maps: np.ndarray, pads):
    """dm4d_skeleton_box_mask_u8 in numpy: uint8 [n, h, w, 3], (pad_top, pad_bottom, pad_x) -> (boxes int32 [n, 4], masks uint8 [n, h, w])."""
    n, h, w, _ = maps.shape
    pt, pb, px = pads
    boxes, masks = np.empty((n, 4), np.int32), np.zeros((n, h, w), np.uint8)
    for f in range(n):
        nz = maps[f].any(axis=2)
        rows, cols = np.flatnonzero(nz.any(axis=1)), np.flatnonzero(nz.any(axis=0))
        boxes[f] = (w, h, -1, -1) if rows.size == 0 else (cols[0], rows[0], cols[-1], rows[-1])
        if rows.size:
            masks[f, max(rows[0] - 1 - pt, 0): min(rows[-1] + 1 + pb, h), max(cols[0] - 1 - px, 0): min(cols[-1] + 1 + px, w)] = 255
    return boxes, masks


def calls_of(records: np.ndarray):
    """skeleton.pack_calls undone: int32 [n, SKEL_FIELDS] -> the draw-call dictionaries."""
    calls = []
    for kind, x1, y1, x2, y2, size, color, _ in records.tolist():
        rgb = [color & 255, (color >> 8) & 255, (color >> 16) & 255]
        calls.append({"type": "line", "p1": [x1, y1], "p2": [x2, y2], "color": rgb, "thickness": size} if kind == 0 else
                     {"type": "circle", "center": [x1, y1], "radius": size, "color": rgb})
    return calls


_MAPS = {}


def model_map(records: np.ndarray, canvas_shape, out_size) -> np.ndarray:
    """skel_model.expected_map of packed records, kept per distinct frame (a scene's maps are asked for several times)."""
    key = (records.tobytes(), tuple(canvas_shape), tuple(out_size))
    if key not in _MAPS:
        _MAPS[key] = skel_model.expected_map(calls_of(records), canvas_shape, out_size)
    return _MAPS[key]


def model_draw(plans):
    return [model_map(skeleton.pack_calls(p.calls), p.canvas_shape, p.out_size) for p in plans]


def standin_skeleton_draw(prims_host, prims, offsets_host, offsets, htab_host, htab, hk, vtab_host, vtab, vk, H, W, h, w, out=None):
    """Drop-in for ops.skeleton_draw on the host."""
    recs, offs = prims_host.numpy(), offsets_host.numpy()
    if out is None:
        out = torch.empty((len(offs) - 1, h, w, 3), dtype=torch.uint8)
    for f in range(len(offs) - 1):
        out[f] = torch.from_numpy(model_map(recs[offs[f]: offs[f + 1]], (H, W), (w, h)).copy())
    return out


def standin_box_mask(maps, pads, masks=None):
    """Drop-in for ops.skeleton_box_mask on the host."""
    boxes, m = rect_model(maps.numpy(), pads)
    if masks is None:
        masks = torch.empty(m.shape, dtype=torch.uint8)
    masks.copy_(torch.from_numpy(m))
    return torch.from_numpy(boxes), masks
