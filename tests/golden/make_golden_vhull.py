#!/usr/bin/env python
"""The visual-hull fixture of tests/test_vhull_cpu.py and tests/test_vhull_gpu.py.

  python tests/golden/make_golden_vhull.py --scene   writes tests/golden/vhull_scene/body6/: 6 cameras on a ring of radius 2.6 with
                                                     distinct intrinsics (transforms.json carries camera_label), 2 frames of 96 x 80
                                                     PNG masks of two ellipsoids (a torso and a head, moved between the frames)
                                                     rendered through each pixel centre, a sprinkle of soft pixels (127 and 128);
                                                     camera 03 stores its masks in mode "1", the others in mode "L"
  python tests/golden/make_golden_vhull.py           runs the REFERENCE's scripts/preprocess/carve_visual_hull.py, imported unmodified,
                                                     on that scene on the CPU and records vhull_reference.pt: carve_visual_hull(...,
                                                     device="cpu") per case of CASES, and main(...) once

Stand-ins go into sys.modules for what the reference imports and this machine lacks: fire, open3d and easyvolcap (unused by the
recorded paths, except parallel_execution and tqdm, which become a plain loop), plyfile (captures the vertex array instead of
writing it), and torchvision's to_tensor backed by Pillow, as torchvision implements it for PIL images.

Exactness: the reference projects with a BLAS fp64 matmul whose summation order is not the one of include/dm4d.h, so a decision
can differ only where a projected coordinate lies within ~1e-12 of a rounding tie or of z = 0.  For every case this script asserts
that no u or v of a voxel-view pair with z > 0 lies within 1e-9 of a half-integer and that no |z| < 1e-9, stores the smallest
margins, and asserts that tests/vhull_model.py reproduces the reference's points exactly.  If a scene constant violates the
margin, change the constant, not the margin.

The every-voxel-kept case is 10^3, not 11^3: torch.arange(-0.05, 0.05, 0.01) has 10 elements in the torch build that recorded the
fixture.  That the element count is torch's own and is never re-derived is pinned by the case "arange4" instead.
"""
from __future__ import annotations

import importlib.util
import json
import math
import sys
import tempfile
import types
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
OUT = Path(__file__).resolve().parent
SCENE_DIR = OUT / "vhull_scene" / "body6"
N_CAMS, N_FRAMES, IMG_H, IMG_W = 6, 2, 96, 80
MODE_1_CAMERA = 3
MARGIN = 1e-9
# (centre, radii) of the torso and the head in frame 0; frame t moves both by t * SHIFT
TORSO = ((0.0, 0.0, 0.0), (0.25, 0.55, 0.18))
HEAD = ((0.02, 0.70, 0.01), (0.13, 0.15, 0.14))
SHIFT = (0.06, -0.03, 0.04)

CASES = [  # name, frame, bounds, voxel_size, batch_size, min_views
    ("cube40_all", 0, (-1.0, 1.0, -1.0, 1.0, -1.0, 1.0), 0.05, 1e4, None),
    ("cube40_min4", 0, (-1.0, 1.0, -1.0, 1.0, -1.0, 1.0), 0.05, 7777, 4),
    ("cube67_all", 0, (-1.0, 1.0, -1.0, 1.0, -1.0, 1.0), 0.03, 1e6, None),
    ("slab_min1", 0, (-3.0, 3.0, -1.0, 1.2, -3.0, 3.0), 0.15, 256, 1),
    ("slab_min6", 0, (-3.0, 3.0, -1.0, 1.2, -3.0, 3.0), 0.15, 256, 6),
    ("dense10", 0, (-0.05, 0.05, -0.05, 0.05, -0.05, 0.05), 0.01, 1e6, None),
    ("empty", 0, (1.2, 3.2, -1.0, 1.0, -1.0, 1.0), 0.05, 1e6, None),
    # 0.2 - (-0.1) = 0.30000000000000004: torch.arange gives 4 elements per axis where (max - min) / voxel_size suggests 3
    ("arange4", 0, (-0.1, 0.2, -0.1, 0.2, -0.1, 0.2), 0.1, 1e6, None),
]
MAIN_KW = {"bounds": (-1.0, 1.0, -1.0, 1.0, -1.0, 1.0), "voxel_size": 0.05, "batch_size": 3000, "min_views": None}


def cameras():
    """-> list of (label, fl_x, fl_y, cx, cy, camera-to-world 4 x 4 in OpenGL axes, rounded to 6 decimals as the file stores it)."""
    out = []
    for c in range(N_CAMS):
        a = 2 * math.pi * c / N_CAMS + 0.3
        o = np.array([2.6 * math.cos(a), 0.1 + 0.15 * math.sin(2 * a), 2.6 * math.sin(a)])
        back = o / np.linalg.norm(o)  # OpenGL: the camera looks down -z
        right = np.cross([0.0, 1.0, 0.0], back)
        right /= np.linalg.norm(right)
        up = np.cross(back, right)
        m = np.eye(4)
        m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = right, up, back, o
        m = np.array([[round(float(v), 6) for v in row] for row in m])
        out.append((f"{c:02d}", 118.0 + 2.5 * c, 119.25 + 2.5 * c, 39.3 + 0.45 * c, 47.6 - 0.35 * c, m))
    return out


def write_scene() -> None:
    from PIL import Image
    frames = []
    vv, uu = np.mgrid[:IMG_H, :IMG_W]
    for c, (label, fx, fy, cx, cy, m) in enumerate(cameras()):
        frames.append({"camera_label": label, "file_path": f"images/{label}/000000.webp", "h": IMG_H, "w": IMG_W, "fl_x": fx, "fl_y": fy,
                       "cx": cx, "cy": cy, "transform_matrix": m.tolist()})
        c2w = m.copy()
        c2w[:3, 1:3] *= -1  # OpenCV axes: the ray of pixel centre (u, v) is ((u - cx) / fx, (v - cy) / fy, 1)
        d = np.stack([(uu - cx) / fx, (vv - cy) / fy, np.ones_like(uu, dtype=np.float64)], axis=-1) @ c2w[:3, :3].T
        o = c2w[:3, 3]
        for t in range(N_FRAMES):
            hit = np.zeros((IMG_H, IMG_W), bool)
            for centre, radii in (TORSO, HEAD):
                ctr = np.array(centre) + t * np.array(SHIFT)
                dd, oo = d / np.array(radii), (o - ctr) / np.array(radii)  # unit sphere in scaled space
                A, Bq, Cq = (dd * dd).sum(-1), (dd * oo).sum(-1), (oo * oo).sum() - 1.0
                hit |= (Bq * Bq - A * Cq >= 0) & (-Bq > 0)
            mask = np.where(hit, 255, 0).astype(np.uint8)
            mask[hit & ((uu * 7 + vv * 13 + c + t) % 29 == 0)] = 128   # soft pixels that stay foreground
            mask[hit & (vv < 36) & ((uu * 3 + vv * 11 + c + t) % 37 == 0)] = 127   # ... and, above the torso's centre, some that are carved
            mask[~hit & ((uu * 5 + vv * 3 + c + t) % 31 == 0)] = 127
            if c == MODE_1_CAMERA:
                im = Image.fromarray(np.where(mask >= 128, 255, 0).astype(np.uint8)).convert("1", dither=Image.Dither.NONE)
            else:
                im = Image.fromarray(mask)
            p = SCENE_DIR / "fmasks" / label / f"{t:06d}.png"
            p.parent.mkdir(parents=True, exist_ok=True)
            im.save(p)
    (SCENE_DIR / "transforms.json").write_text(json.dumps({"w": IMG_W, "h": IMG_H, "frames": frames}, indent=2))


def install_standins(captured: dict) -> None:
    def to_tensor(pic):  # torchvision.transforms.functional.to_tensor for 8-bit and 1-bit PIL images
        a = torch.from_numpy(np.array(pic, np.uint8, copy=True))
        if pic.mode == "1":
            a = 255 * a
        a = a.view(pic.size[1], pic.size[0], len(pic.getbands())).permute((2, 0, 1)).contiguous()
        return a.to(dtype=torch.float32).div(255)

    class PlyElement:
        def __init__(self, data, name):
            self.data, self.name = data, name

        @staticmethod
        def describe(data, name):
            return PlyElement(data, name)

    class PlyData:
        def __init__(self, elements, text=False):
            self.elements, self.text = elements, text

        def write(self, path):
            assert not self.text and len(self.elements) == 1 and self.elements[0].name == "vertex"
            captured[str(path)] = self.elements[0].data.copy()

    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__path__ = []
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m

    module("fire", Fire=lambda fn: None)
    module("open3d")
    module("plyfile", PlyData=PlyData, PlyElement=PlyElement)
    module("torchvision")
    module("torchvision.transforms")
    module("torchvision.transforms.functional", to_tensor=to_tensor)
    module("easyvolcap")
    module("easyvolcap.utils")
    module("easyvolcap.utils.easy_utils", read_camera=None)
    module("easyvolcap.utils.console_utils", tqdm=lambda it, **kw: it)
    module("easyvolcap.utils.parallel_utils", parallel_execution=lambda items, action, **kw: [action(i) for i in items])


def record() -> None:
    import vhull_model
    from oracle import refshim
    captured: dict = {}
    install_standins(captured)
    spec = importlib.util.spec_from_file_location("ref_carve_visual_hull",
                                                  Path(refshim.REFERENCE_ROOT) / "scripts" / "preprocess" / "carve_visual_hull.py")
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    # route 2 first: main() builds P, which route 1 reuses
    seen = {}
    inner = ref.carve_visual_hull

    def recording(fmasks, Ps, *a, **k):
        seen["P"] = Ps.clone()
        return inner(fmasks, Ps, *a, **k)
    ref.carve_visual_hull = recording
    with tempfile.TemporaryDirectory() as tmp:
        surfs = str(Path(tmp) / "surfs")
        ref.main(fmasks_dir=str(SCENE_DIR / "fmasks"), cameras_path=str(SCENE_DIR / "transforms.json"), out_vhull_dir=surfs, device="cpu",
                 **MAIN_KW)
        main_frames = {Path(p).stem: torch.from_numpy(np.stack([v["x"], v["y"], v["z"]], axis=-1).copy()) for p, v in captured.items()}
        for v in captured.values():
            assert (v["red"] == 255).all() and (v["green"] == 255).all() and (v["blue"] == 255).all()
        main_bounds = json.load(open(surfs + "_bounds.json"))
    ref.carve_visual_hull = inner
    P = seen["P"]
    assert P.dtype == torch.float64 and tuple(P.shape) == (N_CAMS, 3, 4)

    labels = sorted(p.name for p in (SCENE_DIR / "fmasks").iterdir())
    masks = [torch.stack([ref.load_binary_mask(str(SCENE_DIR / "fmasks" / lab / f"{t:06d}.png")) for lab in labels]) for t in range(N_FRAMES)]
    for t, (label, pts) in enumerate(sorted(main_frames.items())):
        want = vhull_model.carve(masks[t].numpy(), P.numpy(), MAIN_KW["bounds"], MAIN_KW["voxel_size"], MAIN_KW["min_views"])
        assert pts.dtype == torch.float32 and np.array_equal(pts.numpy(), want), f"main route, frame {label}: the model differs"
        print(f"main {label}: {len(pts)} points")

    cases = []
    for name, frame, bounds, voxel, batch, min_views in CASES:
        pts = ref.carve_visual_hull(masks[frame], P, bounds, voxel_size=voxel, batch_size=batch, min_views=min_views, device="cpu")
        pts = pts.float()  # what the reference's main does with the result
        tie, zmin = vhull_model.margins(masks[frame].shape, P.numpy(), bounds, voxel)
        assert tie >= MARGIN and zmin >= MARGIN, f"{name}: tie margin {tie:.3e}, |z| margin {zmin:.3e}: change a scene constant"
        want = vhull_model.carve(masks[frame].numpy(), P.numpy(), bounds, voxel, min_views)
        assert np.array_equal(pts.numpy(), want), f"{name}: the model differs from the reference"
        grid = tuple(len(a) for a in vhull_model.grid_axes(bounds, voxel))
        cases.append({"name": name, "frame": frame, "bounds": bounds, "voxel_size": voxel, "batch_size": batch, "min_views": min_views,
                      "grid": grid, "points": pts.clone(), "tie_margin": tie, "z_margin": zmin})
        print(f"{name}: grid {grid}, {len(pts)} points, tie margin {tie:.2e}, min |z| {zmin:.2e}")
    torch.save({"scene": "body6", "labels": labels, "P": P, "cases": cases,
                "main": {"kw": MAIN_KW, "frames": main_frames, "bounds_json": main_bounds}}, OUT / "vhull_reference.pt")


if __name__ == "__main__":
    if "--scene" in sys.argv:
        write_scene()
    else:
        record()
