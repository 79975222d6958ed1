#!/usr/bin/env python
"""The skeleton-drawing fixture of tests/test_skel_cpu.py and tests/test_skel_gpu.py.

  python tests/golden/make_golden_skel.py    runs the REFERENCE's scripts/preprocess/draw_skeleton.py::draw_one_skeleton, imported
                                             unmodified, on every case of build_cases() and writes
                                               skel_reference.json  per case: the input instance (and the score-override instance), the
                                                                    arguments, the recorded draw calls, the canvas shape and the size
                                                                    of the file the reference saved
                                               skel_palette.json    the keypoint colours, links and the "x" link colour the reference
                                                                    drew with (data of its sapiens/lite/demo/classes_and_palettes.py), in
                                                                    the layout diffuman4d_amd.host.skeleton.load_palette reads

Stand-ins go into sys.modules for what the reference imports and this project does not depend on: fire, easyvolcap and cv2.  The cv2 stand-in does
not draw: cv2.line and cv2.circle append their arguments to a list, and cv2.cvtColor, which the reference applies to the finished
canvas, reverses the channel order of every recorded colour (and of the array), so the list holds the colours of the saved image.  What
is pinned is therefore everything around the rasteriser -- scores, scaling, rounding, colours, radii, thicknesses, the link filter and
the paint order -- and the saved file's size; OpenCV's rasteriser itself is not available and is not pinned ("Skeleton
maps").  No image is stored.

The cases are built on the frames of tests/golden/triang_scene/ring8 (133 keypoints on a 1024 x 1024 canvas); see build_cases().
"""
from __future__ import annotations

import copy
import importlib.util
import json
import sys
import tempfile
import types
from pathlib import Path

import numpy as np
from PIL import Image

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
OUT = Path(__file__).resolve().parent
RING8 = OUT / "triang_scene" / "ring8" / "poses_sapiens"

CALLS: list = []     # the draw calls of the canvas being painted
CANVAS: list = []    # its shape, as cvtColor saw it


# -- stand-ins --------------------------------------------------------------------------------------------------------------------
def _point(p):
    assert len(p) == 2 and all(isinstance(v, int) for v in p), p
    return [int(p[0]), int(p[1])]


def _line(canvas, p1, p2, color, thickness):
    CALLS.append({"type": "line", "p1": _point(p1), "p2": _point(p2), "color": [int(c) for c in color], "thickness": int(thickness)})


def _circle(canvas, center, radius, color, thickness):
    assert thickness == -1  # filled
    CALLS.append({"type": "circle", "center": _point(center), "radius": int(radius), "color": [int(c) for c in color]})


def _cvt_color(canvas, code):
    assert code == "BGR2RGB"
    for call in CALLS:
        call["color"] = call["color"][::-1]
    CANVAS.append([int(canvas.shape[0]), int(canvas.shape[1])])
    return np.ascontiguousarray(canvas[..., ::-1])


def install_standins() -> None:
    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__path__ = []
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m

    module("cv2", line=_line, circle=_circle, cvtColor=_cvt_color, COLOR_BGR2RGB="BGR2RGB")
    module("fire", Fire=lambda fn: None)
    module("easyvolcap")
    module("easyvolcap.utils")
    module("easyvolcap.utils.parallel_utils", parallel_execution=None)


def load_reference():
    from oracle import refshim
    install_standins()
    pre = Path(refshim.REFERENCE_ROOT) / "scripts" / "preprocess"
    sys.path.insert(0, str(pre))  # the reference runs this file as a script: its directory is on the path, `sapiens` is found there
    spec = importlib.util.spec_from_file_location("ref_draw_skeleton", pre / "draw_skeleton.py")
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    return ref


# -- cases ------------------------------------------------------------------------------------------------------------------------
def ring8(cam: int, frame: int) -> dict:
    return json.loads((RING8 / f"{cam:02d}" / f"{frame:06d}.json").read_text())["instance_info"][0]


def build_cases(links) -> list:
    """-> list of {"name", "instance", "score_instance" | None, "kp2d_canvas_shape", "out_kpmap_shape"}.  `links`: the palette's
    (i1, i2) per link id, used to place ties and the hands."""
    cases = []

    def add(name, instance, out_shape=(1024, 1024), score_instance=None, canvas_shape=(1024, 1024)):
        cases.append({"name": name, "instance": instance, "score_instance": score_instance, "kp2d_canvas_shape": list(canvas_shape),
                      "out_kpmap_shape": list(out_shape)})

    # the three sort branches
    add("scores_only", ring8(0, 0))
    rng = np.random.default_rng(31)
    inst = ring8(1, 0)
    depth = rng.uniform(2.0, 4.0, size=133)
    (a1, a2), (b1, b2) = links[8], links[9]  # two arm links without a common keypoint: equal mean depth, the stable sort keeps 8 first
    depth[[a1, a2, b1, b2]] = [3.0, 2.0, 2.0, 3.0]
    for i in (a1, a2, b1, b2):
        inst["keypoint_scores"][i] = 0.95
    inst["keypoint_depths"] = [round(float(d), 4) for d in depth]
    add("depths_with_a_tie", inst)
    inst = ring8(2, 0)
    del inst["keypoint_scores"]
    add("ones_no_depths", inst)

    # score thresholds: exactly 0.5 and 0.9, just below 0.5, negative coordinates
    inst = ring8(3, 0)
    sc = inst["keypoint_scores"]
    sc[15], sc[13], sc[11] = 0.5, 0.9, 0.95       # left leg: a link at exactly low_thr, one between
    sc[16], sc[14] = 0.4999, 0.95                 # right leg: just below low_thr
    sc[5], sc[6], sc[7], sc[8] = 0.9, 0.9, 0.5, 0.7
    inst["keypoints"][9] = [-3.5, 400.25]         # left wrist: a negative x zeroes its score
    inst["keypoints"][10] = [512.0, -0.01]
    sc[9] = sc[10] = 0.99
    add("thresholds_and_negative_coordinates", inst)

    # a score-override file
    inst = ring8(4, 0)
    rng = np.random.default_rng(32)
    over = {"keypoints": inst["keypoints"], "keypoint_scores": [round(float(s), 3) for s in rng.uniform(0.3, 1.0, size=133)]}
    add("score_override", inst, score_instance=over)

    # rounding ties: with both shapes 1024 the keypoints are doubled, so x.25 lands on k + 0.5 with k even and x.75 with k odd
    inst = ring8(5, 0)
    for i in range(0, 23):
        x, y = inst["keypoints"][i]
        inst["keypoints"][i] = [float(int(x)) + (0.25 if i % 2 == 0 else 0.75), float(int(y)) + (0.75 if i % 3 == 0 else 0.25)]
    add("rounding_ties", inst)

    # shapes
    for k, shape in enumerate([(1000, 600), (720, 1280), (512, 512), (2048, 2048), (2500, 1500)]):
        add(f"shape_{shape[0]}x{shape[1]}", ring8(k, 1), out_shape=shape)
    add("canvas_shape_768x1024", ring8(6, 1), out_shape=(1024, 768), canvas_shape=(768, 1024))

    # capacity: every link of both hands inside one 32 x 32 output tile (output pixels 288 .. 319), two links of length zero
    inst = ring8(7, 0)
    rng = np.random.default_rng(33)
    for i in range(91, 133):
        inst["keypoints"][i] = [round(float(rng.uniform(290.0, 317.0)), 2), round(float(rng.uniform(290.0, 317.0)), 2)]
        inst["keypoint_scores"][i] = round(float(rng.uniform(0.55, 1.0)), 3)
    inst["keypoints"][95] = inst["keypoints"][94]      # link 28 (94, 95)
    inst["keypoints"][132] = inst["keypoints"][131]    # link 64 (131, 132)
    add("hands_in_one_tile", inst)

    # off the canvas: inside +-8191 on the 2048 canvas (drawn, clipped), and beyond it (the native code drops such a link)
    inst = ring8(6, 0)
    inst["keypoints"][15] = [2900.5, 700.0]     # -> 5801
    inst["keypoints"][7] = [300.0, 4000.0]      # -> 8000
    inst["keypoints"][10] = [4095.5, 100.0]     # -> 8191
    for i in (15, 13, 7, 5, 9, 10, 8):
        inst["keypoint_scores"][i] = 0.97
    add("off_canvas_inside_range", inst)
    inst = ring8(6, 0)
    inst["keypoints"][16] = [4096.0, 500.0]     # -> 8192: one past the range
    inst["keypoints"][9] = [600.0, 50000.0]
    for i in (16, 14, 20, 21, 22, 9, 7):
        inst["keypoint_scores"][i] = 0.97
    add("off_canvas_beyond_range", inst)
    return cases


def record() -> None:
    ref = load_reference()
    colors, skeleton, blue = ref.COCO_WHOLEBODY_KPTS_COLORS, ref.COCO_WHOLEBODY_SKELETON_INFO, ref.BLUE
    assert sorted(skeleton) == list(range(65)) and all(v["id"] == k for k, v in skeleton.items())
    palette = {"keypoint_colors": [None if c is None else [int(v) for v in c] for c in colors],
               "links": [{"id": int(v["id"]), "link": [int(v["link"][0]), int(v["link"][1])], "color": [int(c) for c in v["color"]]}
                         for v in skeleton.values()],
               "x_link_color": [int(c) for c in blue]}
    links = {v["id"]: v["link"] for v in palette["links"]}
    (OUT / "skel_palette.json").write_text(json.dumps(palette, separators=(",", ":")) + "\n")

    out = []
    with tempfile.TemporaryDirectory() as tmp:
        for case in build_cases(links):
            kp_path, score_path, img_path = f"{tmp}/kp.json", None, f"{tmp}/{case['name']}/map.webp"
            Path(kp_path).write_text(json.dumps({"instance_info": [case["instance"]]}))
            if case["score_instance"] is not None:
                score_path = f"{tmp}/score.json"
                Path(score_path).write_text(json.dumps({"instance_info": [case["score_instance"]]}))
            del CALLS[:], CANVAS[:]
            ref.draw_one_skeleton(kp_path, img_path, kp2d_score_path=score_path, kp2d_canvas_shape=tuple(case["kp2d_canvas_shape"]),
                                  out_kpmap_shape=tuple(case["out_kpmap_shape"]))
            assert len(CANVAS) == 1 and len(CALLS) % 3 == 0
            with Image.open(img_path) as im:
                size = [int(im.size[0]), int(im.size[1])]
            out.append({**case, "calls": copy.deepcopy(CALLS), "canvas_shape": CANVAS[0], "saved_size": size})
            print(f"{case['name']}: {len(CALLS)} calls, canvas {CANVAS[0]}, saved {size[0]} x {size[1]}")
    by = {c["name"]: c for c in out}
    assert by["shape_1000x600"]["saved_size"] == [599, 1000] and by["shape_720x1280"]["saved_size"] == [1280, 720]
    assert by["scores_only"]["saved_size"] == [1024, 1024]
    path = OUT / "skel_reference.json"
    path.write_text(json.dumps({"cases": out}, separators=(",", ":")) + "\n")
    print("wrote", path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    record()
