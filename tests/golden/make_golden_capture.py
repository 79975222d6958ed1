#!/usr/bin/env python
"""The captured-scene fixture of tests/test_capture_cpu.py and tests/test_capture_gpu.py.

  python tests/golden/make_golden_capture.py --scene   writes tests/golden/capture_scene/ring8/: 8 cameras on a ring x 3 frames,
                                                       nerfstudio transforms.json (per-frame intrinsics on even cameras, the global
                                                       ones on odd cameras), WebP images and skeletons, PNG L masks whose boxes
                                                       touch the image border (crops extend past it)
  python tests/golden/make_golden_capture.py           runs the REFERENCE's SpaTemDataset (src/data/spatem_dataset.py, imported
                                                       unmodified through oracle/refshim.py) on that scene and records
                                                       capture_reference.pt: spatial and temporal queries, has_gt_target True and
                                                       False, an output size below and one above the crop size

torchvision is not installed here: a Pillow-backed stand-in of torchvision.transforms.functional (crop, resize, to_tensor,
to_pil_image, as torchvision implements them for PIL images) goes into sys.modules before refshim.install(), which leaves
existing entries alone.  Large tensors are recorded as sha256 digests of their bytes (plus a strided thumbnail to diagnose a
mismatch), so that the file stays small.
"""
from __future__ import annotations

import hashlib
import json
import math
import sys
import types
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
OUT = Path(__file__).resolve().parent
SCENE_DIR = OUT / "capture_scene"
SCENE = "ring8"
N_CAMS, N_FRAMES, IMG_H, IMG_W = 8, 3, 200, 160
INPUTS = ["01", "05"]
QUERIES = [  # (name, height/width, has_gt_target, spa_labels, tem_labels)
    ("spatial_down", 64, True, [f"{c:02d}" for c in range(N_CAMS)], ["000001"]),
    ("temporal_down", 64, True, ["03"], ["000000", "000001", "000002"]),
    ("spatial_up_skel", 256, False, [f"{c:02d}" for c in range(N_CAMS)], ["000002"]),
    ("temporal_up_skel", 256, False, ["06"], ["000000", "000001", "000002"]),
]


def digest(t) -> str:
    a = t.detach().cpu().contiguous().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
    return hashlib.sha256(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


def write_scene() -> None:
    from PIL import Image, ImageDraw
    root = SCENE_DIR / SCENE
    rng = np.random.default_rng(7)
    frames = []
    for c in range(N_CAMS):
        a = 2 * math.pi * c / N_CAMS
        o = np.array([3.0 * math.cos(a), 0.2 * math.sin(3 * a), 3.0 * math.sin(a)])
        back = o / np.linalg.norm(o)  # OpenGL: the camera looks down -z, so +z points away from the subject
        right = np.cross([0.0, 1.0, 0.0], back)
        right /= np.linalg.norm(right)
        up = np.cross(back, right)
        m = np.eye(4)
        m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = right, up, back, o
        fr = {"camera_label": f"{c:02d}", "file_path": f"images/{c:02d}/000000.webp", "h": IMG_H, "w": IMG_W,
              "transform_matrix": [[round(float(v), 6) for v in row] for row in m]}
        if c % 2 == 0:
            fr.update(fl_x=200.0 + 3.5 * c, fl_y=201.25 + 3.5 * c, cx=80.5 - c, cy=99.75 + 0.5 * c)
        frames.append(fr)
        for t in range(N_FRAMES):
            # subject: an ellipse that drifts so that its box touches the left / top / right / bottom border on some views
            cx = [4, 80, 156, 60, 100, 20, 140, 80][c] + 6 * t
            cy = [100, 3, 100, 197, 60, 150, 120, 100][c] - 4 * t
            rx, ry = 38 + 3 * t, 70 - 2 * c
            yy, xx = np.mgrid[:IMG_H, :IMG_W]
            inside = ((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 < 1.0
            mask = np.where(inside, 255, 0).astype(np.uint8)
            mask[inside & (((xx + yy + t) % 23) == 0)] = 128  # soft pixels, as matting leaves them
            base = np.stack([(xx * 1.4 + 40 * c) % 256, (yy * 1.2 + 30 * t) % 256, (xx + yy) % 256], axis=-1)
            img = np.clip(base + rng.integers(-12, 13, base.shape), 0, 255).astype(np.uint8)
            skel = Image.new("RGB", (IMG_W, IMG_H))
            d = ImageDraw.Draw(skel)
            pts = [(cx, cy - ry // 2), (cx, cy + ry // 3), (cx - rx // 2, cy + ry // 2), (cx + rx // 2, cy + ry // 2),
                   (cx - rx // 2, cy - ry // 4), (cx + rx // 2, cy - ry // 4)]
            for k, (p, q) in enumerate([(0, 1), (1, 2), (1, 3), (0, 4), (0, 5)]):
                d.line([pts[p], pts[q]], fill=(60 + 40 * k, 255 - 30 * k, 90 + 25 * c), width=3)
            for sub, im, ext in (("images", Image.fromarray(img), "webp"), ("skeletons", skel, "webp"),
                                 ("fmasks", Image.fromarray(mask), "png")):
                p = root / sub / f"{c:02d}" / f"{t:06d}.{ext}"
                p.parent.mkdir(parents=True, exist_ok=True)
                im.save(p, quality=80) if ext == "webp" else im.save(p)
    tfs = {"fl_x": 205.0, "fl_y": 204.5, "cx": 79.25, "cy": 100.5, "w": IMG_W, "h": IMG_H, "frames": frames}
    (root / "transforms.json").write_text(json.dumps(tfs, indent=2))


def install_torchvision_standin() -> None:
    """torchvision.transforms.functional for PIL inputs (what the reference's dataset calls), backed by Pillow."""
    from PIL import Image

    class InterpolationMode:
        NEAREST, BILINEAR, BICUBIC = "nearest", "bilinear", "bicubic"

    pil_filter = {"nearest": Image.NEAREST, "bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}

    def crop(img, top, left, height, width):
        return img.crop((left, top, left + width, top + height))

    def resize(img, size, interpolation="bilinear", max_size=None, antialias=True):
        h, w = (size, size) if isinstance(size, int) else size
        if (img.size[1], img.size[0]) == (h, w):
            return img
        return img.resize((w, h), pil_filter[interpolation])

    def to_tensor(pic):
        a = torch.from_numpy(np.array(pic, np.uint8, copy=True))
        a = a.view(pic.size[1], pic.size[0], len(pic.getbands())).permute((2, 0, 1)).contiguous()
        return a.to(dtype=torch.float32).div(255)

    def to_pil_image(pic, mode=None):
        if pic.ndim == 2:
            pic = pic.unsqueeze(0)
        if pic.is_floating_point() and mode != "F":
            pic = pic.mul(255).byte()
        a = np.transpose(pic.cpu().numpy(), (1, 2, 0))
        return Image.fromarray(a[:, :, 0] if a.shape[2] == 1 else a)

    tv = types.ModuleType("torchvision")
    tv.__path__ = []
    tr = types.ModuleType("torchvision.transforms")
    tr.__path__ = []
    tr.InterpolationMode = InterpolationMode
    fn = types.ModuleType("torchvision.transforms.functional")
    fn.crop, fn.resize, fn.to_tensor, fn.to_pil_image = crop, resize, to_tensor, to_pil_image
    tv.transforms, tr.functional = tr, fn
    sys.modules.update({"torchvision": tv, "torchvision.transforms": tr, "torchvision.transforms.functional": fn})


def record() -> None:
    install_torchvision_standin()
    from oracle import refshim
    refshim.install()
    import src.data.spatem_dataset as sd
    masks = []
    inner = sd.skeleton_to_mask

    def recording(skeleton, *a, **k):
        m = inner(skeleton, *a, **k)
        masks.append(np.asarray(m).copy())
        return m
    sd.skeleton_to_mask = recording
    out = {"scene": SCENE, "inputs": INPUTS, "queries": {}}
    for name, size, gt, spa, tem in QUERIES:
        torch.manual_seed(0)
        ds = sd.SpaTemDataset(data_dir=str(SCENE_DIR), scene_label=SCENE, height=size, width=size, has_gt_target=gt)
        masks.clear()
        s = ds.get_item(SCENE, spa, tem, INPUTS)
        rec = {"kw": {"height": size, "width": size, "has_gt_target": gt}, "spa": spa, "tem": tem,
               "domain": s["domain"], "labels": s["labels"], "Ks": s["Ks"], "poses": s["poses"], "hws": s["hws"],
               "crops": [[int(v) for v in c] for c in s["crops"]], "cond_masks": s["cond_masks"][:, 0, 0, 0].clone(),
               "cond_masks_shape": tuple(s["cond_masks"].shape), "skeleton_masks": [digest(m) for m in masks]}
        for k in ("pixel_values", "skeletons", "plucker_embeds"):
            rec[k + "_sha256"] = digest(s[k])
            rec[k + "_shape"] = tuple(s[k].shape)
            rec[k + "_thumb"] = s[k][:, :, ::16, ::16].clone()
        out["queries"][name] = rec
        print(name, s["domain"], tuple(s["pixel_values"].shape), s["crops"][:2])
    out["cameras"] = {lab: {"K": c["K"], "pose": c["pose"]} for lab, c in ds.cameras[SCENE].items()}
    torch.save(out, OUT / "capture_reference.pt")


if __name__ == "__main__":
    if "--scene" in sys.argv:
        write_scene()
    else:
        record()
