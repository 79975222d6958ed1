"""Skeleton maps: ``skeletons/{cam}/{frame}.webp`` from ``poses_2d/{cam}/{frame}.json``, the image the denoiser's pose encoder is
conditioned on (host/capture.py reads it back).

The reference's ``scripts/preprocess/draw_skeleton.py`` (the ``draw_skeleton`` action of ``preprocess.sh``) with the same function
names, arguments and defaults, built from its behaviour.  The reference paints one frame at a time with OpenCV on a 2048-pixel
canvas and reduces it with Pillow; here

  * ``plan_draw_calls`` (numpy, no device, no library) turns one frame's keypoints into the ordered list of primitives the reference
    hands to ``cv2.line`` / ``cv2.circle`` -- scores, scaling, rounding, colours, radii, the link filter and the paint order are the
    reference's, pinned call for call by tests/golden/skel_reference.json;
  * one launch (``dm4d_skeleton_draw_u8``) rasterises a batch of frames and applies Pillow's bicubic ``Image.resize`` byte for byte;
    the 2048-pixel canvas exists only tile by tile in LDS;
  * the host reads the JSON files and encodes the images (Pillow's ``Image.save(path, quality=...)``) in a thread pool.

The rasteriser is NOT OpenCV's: a primitive covers the pixels given by the exact integer rule in DESIGN.md ("Skeleton maps"), which
differs from OpenCV's edge walker in pixels on a primitive's rim only.  The colour and link tables are not part of this package: the
caller names a palette file (``load_palette``).  There is no CPU path: a ``device`` that is not a HIP device is an error.

Opt-in, the ``poses_2d`` directory can be left out altogether: ``draw_skeleton_maps_kp3d`` and ``draw_skeleton(kp3d_dir=...,
camera_path=...)`` take the scene's 3-D keypoints (``poses_3d/{frame}.json``) and cameras, and project, plan
(``dm4d_skeleton_plan_kp3d``: ``plan_draw_calls`` on the device, one wave per map) and draw (``dm4d_skeleton_draw_planned_u8``) there:
no file per camera and frame, no host plan, no records over PCIe -- the same records and the same bytes (DESIGN.md "Skeleton maps from
poses_3d").  ``map_params`` and ``plan_tables`` are what the host still computes: per map shape and per palette.
"""
from __future__ import annotations

import contextlib
import json
import logging
import os
import time
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import lib as _l
from . import ops
from .resample import TableSet
from .staging import MAX_HOST_THREADS  # noqa: F401  (importable from here as before)

log = logging.getLogger(__name__)

DRAWING_SIZE = 2048        # the longer side of the canvas the reference paints on ("draw skeleton map at 2048p for anti-aliasing")
X_LINKS = ((65, (5, 12)), (66, (6, 11)))  # "add x links for the body": left shoulder - right hip, right shoulder - left hip
MAJOR_LINKS = 25           # link ids below this are painted at twice the radius and thickness
COORD_MIN, COORD_MAX = ops.SKEL_COORD_MIN, ops.SKEL_COORD_MAX
MIN_OUT, MAX_OUT = 256, 8192   # supported max(out_kpmap_shape): below, a tile's canvas footprint no longer fits in LDS
LAUNCH_BYTES = 1 << 28     # the frame axis is cut so that one launch's maps stay below this

PALETTE_HELP = ("a palette is a JSON file {\"keypoint_colors\": [[r, g, b] | null, ...], \"links\": [{\"id\": 0, \"link\": [i1, i2], "
                "\"color\": [r, g, b]}, ...], \"x_link_color\": [r, g, b]}: for the reference's drawing, write COCO_WHOLEBODY_KPTS_COLORS, "
                "COCO_WHOLEBODY_SKELETON_INFO and BLUE of its sapiens/lite/demo/classes_and_palettes.py into one "
                "(tests/golden/make_golden_skel.py does)")


class Palette(NamedTuple):
    keypoint_colors: List[Optional[List[int]]]
    links: List[Dict]          # {"id", "link": (i1, i2), "color"} in the file's order
    x_link_color: List[int]


class DrawPlan(NamedTuple):
    calls: List[Dict]                 # {"type": "line", "p1", "p2", "color", "thickness"} | {"type": "circle", "center", "radius", "color"}
    canvas_shape: Tuple[int, int]     # (H, W) of the canvas the calls refer to
    out_size: Tuple[int, int]         # (w, h) of the reduced map, Pillow's order
    dropped_links: int                # links with an endpoint outside [COORD_MIN, COORD_MAX], not drawn


# -- palette ------------------------------------------------------------------------------------------------------------------------
def _rgb(c, what: str) -> List[int]:
    if not isinstance(c, (list, tuple)) or len(c) != 3 or not all(isinstance(v, int) and 0 <= v <= 255 for v in c):
        raise ValueError(f"palette: {what} must be [r, g, b] with integers in 0 .. 255, got {c!r}")
    return [int(v) for v in c]


def make_palette(data: Dict) -> Palette:
    """The parsed content of a palette file -> Palette, validated."""
    try:
        colors, links, x_color = data["keypoint_colors"], data["links"], data["x_link_color"]
    except (KeyError, TypeError):
        raise ValueError(f"palette: expected the keys keypoint_colors, links and x_link_color; {PALETTE_HELP}") from None
    n = len(colors)
    colors = [None if c is None else _rgb(c, f"keypoint_colors[{i}]") for i, c in enumerate(colors)]
    out, seen = [], set()
    for k, l in enumerate(links):
        i1, i2 = (int(v) for v in l["link"])
        lid = int(l["id"])
        if lid in seen or lid < 0:
            raise ValueError(f"palette: links[{k}] has the id {lid}, which is negative or used twice")
        seen.add(lid)
        if not (0 <= i1 < n and 0 <= i2 < n):
            raise ValueError(f"palette: links[{k}] joins keypoints {i1} and {i2}, but there are {n} keypoint colours")
        out.append({"id": lid, "link": (i1, i2), "color": _rgb(l["color"], f"links[{k}].color")})
    return Palette(colors, out, _rgb(x_color, "x_link_color"))


def load_palette(path) -> Palette:
    """Read a palette file.  The package ships no table of its own: without a file there is nothing to draw with."""
    if path is None:
        raise ValueError(f"no palette given: {PALETTE_HELP}")
    if isinstance(path, Palette):
        return path
    if not os.path.isfile(path):
        raise FileNotFoundError(f"palette {path!r} not found: {PALETTE_HELP}")
    with open(path, "r") as f:
        return make_palette(json.load(f))


# -- the plan -----------------------------------------------------------------------------------------------------------------------
def score_to_color(rgb, score, low=0.5, high=0.9) -> List[int]:
    """A colour dimmed by its score: black at `low`, full at `high`, in float32, rounded half to even (draw_skeleton.py:18-23)."""
    score = np.clip(score, low, high)
    norm_score = (score - low) / (high - low)
    rgb = np.array(rgb, dtype=np.float32) * norm_score
    return np.round(rgb, decimals=0).astype(np.uint8).tolist()


def plan_draw_calls(instance: Dict, score_instance: Optional[Dict], shapes, palette: Palette, low_thr=0.5, high_thr=0.9, radius=2,
                    thickness=2, draw_face_keypoints: bool = False) -> DrawPlan:
    """One frame's ``instance_info[0]`` -> the primitives the reference paints, in its order (draw_one_skeleton, draw_skeleton.py:49-161).

    `shapes` = (kp2d_canvas_shape, out_kpmap_shape), both (h, w).  `score_instance`: the ``instance_info[0]`` of a score-override
    file, or None.  Every array operation below has the operand types of the reference's, so that NumPy promotes and rounds as it
    does there: float32 keypoints times a float64 ratio, float32 colour arithmetic, ``int(round(.))`` half to even.  Colours are RGB
    (the reference reverses them for OpenCV and reverses the canvas back).  A link with an endpoint outside [-8192, 8191] is left out
    with its two circles and counted in `dropped_links`: the device's coverage test is exact in 64-bit integers inside that range."""
    if draw_face_keypoints:
        raise NotImplementedError("draw_face_keypoints: the reference's own branch passes an array as a radius and fails; not built")
    kp2d_canvas_shape, out_kpmap_shape = shapes
    kpts = np.array(instance["keypoints"], dtype=np.float32)
    if score_instance is not None:
        scores = np.array(score_instance["keypoint_scores"], dtype=np.float32)
    elif "keypoint_scores" in instance:
        scores = np.array(instance["keypoint_scores"], dtype=np.float32)
    else:
        scores = np.ones(kpts.shape[0], dtype=np.float32)
    if "keypoint_depths" in instance:
        depths = np.array(instance["keypoint_depths"], dtype=np.float32)
    else:
        depths = np.zeros_like(scores)
    scores[kpts.min(axis=1) < 0] = 0.0  # invalid keypoints

    drawing_scale = DRAWING_SIZE / max(out_kpmap_shape)
    canvas_shape = (np.array(out_kpmap_shape) * drawing_scale).astype(np.int32)
    kp_shape = np.array(kp2d_canvas_shape)
    scale_ratio = canvas_shape.min() / kp_shape.min()
    kpts = kpts * scale_ratio
    kp_shape = kp_shape * scale_ratio
    kpts += (canvas_shape.min() - kp_shape.min()) / 2

    if len(palette.keypoint_colors) != len(kpts):
        raise ValueError(f"the length of kpt_color ({len(palette.keypoint_colors)}) does not matches that of keypoints ({len(kpts)})")
    links = list(palette.links) + [{"id": lid, "link": link, "color": palette.x_link_color} for lid, link in X_LINKS
                                   if all(l["id"] != lid for l in palette.links)]
    if max(max(l["link"]) for l in links) >= len(kpts):
        raise ValueError(f"a link joins keypoint {max(max(l['link']) for l in links)}, but the frame has {len(kpts)} keypoints")

    # per-link radius and thickness, indexed by link id as in the reference
    radius = int(round(radius * scale_ratio))
    thickness = int(round(thickness * scale_ratio))
    if thickness < 1:
        raise ValueError(f"thickness rounds to {thickness} on the canvas (scale {float(scale_ratio):.4g}): a line needs at least 1")
    if max(l["id"] for l in links) >= len(links):
        raise ValueError(f"link ids must be below the number of links ({len(links)}): the per-link arrays are indexed by id")
    radii = np.ones(len(links)) * radius
    thicknesses = np.ones(len(links)) * thickness
    radii[:MAJOR_LINKS] *= 2
    thicknesses[:MAJOR_LINKS] *= 2
    radii, thicknesses = radii.astype(np.int32), thicknesses.astype(np.int32)

    # the links at once: the same float32 / float64 operations element by element as the reference's loop over links
    i1, i2 = (np.array([l["link"][k] for l in links]) for k in (0, 1))
    p1_score, p2_score = scores[i1], scores[i2]
    line_score = np.minimum(p1_score, p2_score)
    keep = ~(line_score < low_thr)
    ends = np.concatenate([kpts[i1], kpts[i2]], axis=1)  # [links, 4]: x1, y1, x2, y2
    if not np.isfinite(ends[keep]).all():
        raise ValueError("a keypoint of a drawn link is not finite")
    ends = np.rint(ends)  # int(round(.)): half to even
    inside = ((ends >= COORD_MIN) & (ends <= COORD_MAX)).all(axis=1)
    dropped = int((keep & ~inside).sum())
    keep &= inside
    ends = np.where(keep[:, None], ends, 0).astype(np.int64)
    for l, k in zip(links, keep):
        if k and (palette.keypoint_colors[l["link"][0]] is None or palette.keypoint_colors[l["link"][1]] is None):
            raise ValueError(f"palette: link {l['id']} joins keypoints {l['link'][0]} and {l['link'][1]}, one of which has no colour")
    kp_rgb = np.array([[0, 0, 0] if c is None else c for c in palette.keypoint_colors], dtype=np.float32)
    link_rgb = np.array([l["color"] for l in links], dtype=np.float32)

    def dimmed(rgb, score):  # score_to_color over rows
        norm_score = (np.clip(score, low_thr, high_thr) - low_thr) / (high_thr - low_thr)
        return np.round(rgb * norm_score[:, None], decimals=0).astype(np.uint8).tolist()

    p1_color, p2_color, line_color = dimmed(kp_rgb[i1], p1_score), dimmed(kp_rgb[i2], p2_score), dimmed(link_rgb, line_score)
    depth = ((depths[i1].astype(np.float64) + depths[i2].astype(np.float64)) / 2).tolist()
    order = [k for k in range(len(links)) if keep[k]]
    if (depths != 0.0).any():
        order = sorted(order, key=lambda k: depth[k], reverse=True)  # far links first; sorted() is stable, also when reversed
    elif (scores != 1.0).any():
        score_key = line_score.tolist()
        order = sorted(order, key=lambda k: score_key[k])
    ends = ends.tolist()
    calls = []
    for k in order:
        lid = links[k]["id"]
        calls.append({"type": "line", "p1": ends[k][:2], "p2": ends[k][2:], "color": line_color[k], "thickness": int(thicknesses[lid])})
        calls.append({"type": "circle", "center": ends[k][:2], "radius": int(radii[lid]), "color": p1_color[k]})
        calls.append({"type": "circle", "center": ends[k][2:], "radius": int(radii[lid]), "color": p2_color[k]})
    H, W = int(canvas_shape[0]), int(canvas_shape[1])
    return DrawPlan(calls, (H, W), (int(W / drawing_scale), int(H / drawing_scale)), dropped)


def pack_calls(calls: Sequence[Dict]) -> np.ndarray:
    """Draw calls -> int32 [n, SKEL_FIELDS] records of include/dm4d.h: {kind, x1, y1, x2, y2, size, r | g << 8 | b << 16, 0}."""
    rows = []
    for c in calls:
        r, g, b = c["color"]
        if c["type"] == "line":
            rows.append((ops.SKEL_LINE, *c["p1"], *c["p2"], c["thickness"], r | (g << 8) | (b << 16), 0))
        else:
            rows.append((ops.SKEL_CIRCLE, *c["center"], *c["center"], c["radius"], r | (g << 8) | (b << 16), 0))
    return np.array(rows, dtype=np.int32).reshape(len(rows), ops.SKEL_FIELDS)


# -- the launch ---------------------------------------------------------------------------------------------------------------------
def _check_out_shape(out_kpmap_shape) -> None:
    if len(out_kpmap_shape) != 2 or not MIN_OUT <= max(out_kpmap_shape) <= MAX_OUT or min(out_kpmap_shape) < 1:
        raise ValueError(f"out_kpmap_shape {tuple(out_kpmap_shape)}: max(out_kpmap_shape) must lie in {MIN_OUT} .. {MAX_OUT} (the canvas is "
                         f"{DRAWING_SIZE} pixels on its longer side, and below {MIN_OUT} an output tile's part of it does not fit in LDS)")


def _draw_chunks(plans: Sequence[DrawPlan], dev: torch.device, out: Optional[torch.Tensor] = None):
    """The device half of draw_plans: yields (first frame, uint8 [b, h, w, 3] tensor on `dev`) launch by launch, on the current stream,
    and reads nothing back.  With `out` ([B, h, w, 3] on `dev`) every launch writes its frames of it; without, a launch allocates its own."""
    if not plans:
        raise ValueError("draw_plans: no frames")
    (H, W), (w, h) = plans[0].canvas_shape, plans[0].out_size
    if any(p.canvas_shape != (H, W) or p.out_size != (w, h) for p in plans):
        raise ValueError("draw_plans: the frames of one batch must share the canvas shape and the output size")
    tables = TableSet()
    (ho, hk), (vo, vk) = tables.add(W, w), tables.add(H, h)
    step = max(1, LAUNCH_BYTES // (h * w * 3))
    with torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext():
        tab_h = torch.from_numpy(tables.array())
        tab_d = tab_h.to(dev)  # dm4d_skeleton_draw_u8 takes each axis' table by pointer: views of the one array
        htab_h, htab_d = (t[ho:ho + w * (2 + hk)] for t in (tab_h, tab_d))
        vtab_h, vtab_d = (t[vo:vo + h * (2 + vk)] for t in (tab_h, tab_d))
        for b0 in range(0, len(plans), step):
            chunk = plans[b0:b0 + step]
            recs = [pack_calls(p.calls) for p in chunk]
            offsets = torch.from_numpy(np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int32))
            prims = torch.from_numpy(np.concatenate(recs + [np.zeros((1, ops.SKEL_FIELDS), dtype=np.int32)]))  # never empty
            yield b0, ops.skeleton_draw(prims, prims.to(dev), offsets, offsets.to(dev), htab_h, htab_d, hk, vtab_h, vtab_d,
                                        vk, H, W, h, w, out=None if out is None else out[b0:b0 + len(chunk)])


def draw_plans_into(plans: Sequence[DrawPlan], out: torch.Tensor) -> torch.Tensor:
    """Plans of one canvas shape and output size drawn into `out`, uint8 [B, h, w, 3] on the device (a view of a larger buffer is
    fine), on the current stream; the maps stay where they are drawn (host/capture.py consumes them there).  Cut along B as draw_plans."""
    (w, h) = plans[0].out_size if plans else (0, 0)
    if not isinstance(out, torch.Tensor) or tuple(out.shape) != (len(plans), h, w, 3):
        raise ValueError(f"draw_plans_into: out must be [{len(plans)}, {h}, {w}, 3], got {tuple(getattr(out, 'shape', ()))}")
    for _ in _draw_chunks(plans, out.device, out):
        pass
    return out


def draw_plans(plans: Sequence[DrawPlan], device="cuda") -> np.ndarray:
    """Plans of one canvas shape and output size -> uint8 [B, h, w, 3], one launch (cut along B where the maps pass 256 MiB)."""
    if not plans:
        raise ValueError("draw_plans: no frames")
    dev = _l.hip_device(device, "draw_skeleton_maps")
    out = [maps.cpu().numpy() for _, maps in _draw_chunks(plans, dev)]
    return out[0] if len(out) == 1 else np.concatenate(out)


def _read_instance(path) -> Optional[Dict]:
    if path is None:
        return None
    with open(path, "r") as f:
        return json.load(f)["instance_info"][0]  # "currently, we only support one instance per image"


def draw_skeleton_maps(kp2d_paths: Sequence[str], kp2d_score_paths: Optional[Sequence[Optional[str]]] = None,
                       kp2d_canvas_shape=(1024, 1024), out_kpmap_shape=(1024, 1024), low_thr=0.5, high_thr=0.9, radius=2, thickness=2,
                       draw_face_keypoints: bool = False, palette=None, num_workers: int = 16, device="cuda", stats: Optional[Dict] = None,
                       pool: Optional[ThreadPoolExecutor] = None, out: Optional[torch.Tensor] = None):
    """The maps of many keypoint files -> uint8 [B, h, w, 3] (RGB), drawn in one launch; the files are read in a pool of `num_workers`
    threads (at most 16).  `stats`, when given, receives dropped_links and the seconds spent reading, planning and on the device.
    With `out` (uint8 [B, h, w, 3] on the device) the maps are drawn into it (draw_plans_into) and it is returned: nothing is read back."""
    palette = load_palette(palette)
    _check_out_shape(out_kpmap_shape)
    if kp2d_score_paths is None:
        kp2d_score_paths = [None] * len(kp2d_paths)
    own = pool is None
    if own:
        pool = ThreadPoolExecutor(max_workers=max(1, min(int(num_workers), MAX_HOST_THREADS)), thread_name_prefix="dm4d-skel")
    try:
        t0 = time.perf_counter()
        instances = list(pool.map(_read_instance, kp2d_paths))
        score_instances = list(pool.map(_read_instance, kp2d_score_paths))
    finally:
        if own:
            pool.shutdown()
    t1 = time.perf_counter()
    plans = [plan_draw_calls(inst, sc, (kp2d_canvas_shape, out_kpmap_shape), palette, low_thr, high_thr, radius, thickness, draw_face_keypoints)
             for inst, sc in zip(instances, score_instances)]
    t2 = time.perf_counter()
    maps = draw_plans(plans, device=device) if out is None else draw_plans_into(plans, out)
    t3 = time.perf_counter()
    if stats is not None:
        stats["dropped_links"] = stats.get("dropped_links", 0) + sum(p.dropped_links for p in plans)
        for key, dt in (("read", t1 - t0), ("plan", t2 - t1), ("launch", t3 - t2)):
            stats[key] = stats.get(key, 0.0) + dt
    return maps


# -- from poses_3d: project, plan and draw on the device --------------------------------------------------------------------------------
class MapParams(NamedTuple):
    scale_ratio: float                # fp64, as plan_draw_calls forms it
    offset: float                     # fp64: the centring term added after the scaling
    radius: int                       # int(round(radius * scale_ratio))
    thickness: int
    canvas_shape: Tuple[int, int]     # (H, W)
    out_size: Tuple[int, int]         # (w, h)


class PlanTables(NamedTuple):
    links: np.ndarray                 # int32 [L, SKEL_LINK_FIELDS] = {i1, i2, id, radius multiplier, thickness multiplier, 0, 0, 0}
    colors: np.ndarray                # float32 [k + L, 4] = {r, g, b, has-colour}: the keypoints, then the links
    low_thr: float                    # the three thresholds as the float32 values NumPy's weak scalars take
    high_thr: float
    thr_span: float                   # float32(high_thr - low_thr), the difference formed in fp64
    n_keypoints: int


def read_kp3d(path) -> np.ndarray:
    """A ``poses_3d/{frame}.json`` file (triang.write_kp3d) -> fp64 [k, 3] keypoints of ``instance_info[0]``, -1e6 where not triangulated."""
    with open(path, "r") as f:
        kp = np.array(json.load(f)["instance_info"][0]["keypoints"], dtype=np.float64)
    if kp.ndim != 2 or kp.shape[1] != 3 or kp.shape[0] < 1:
        raise ValueError(f"{path}: keypoints must have shape (k, 3), got {kp.shape}")
    return kp


def map_params(shapes, radius=2, thickness=2) -> MapParams:
    """What plan_draw_calls derives from `shapes` = (kp2d_canvas_shape, out_kpmap_shape) alone, in its arithmetic and with its error."""
    kp2d_canvas_shape, out_kpmap_shape = shapes
    drawing_scale = DRAWING_SIZE / max(out_kpmap_shape)
    canvas_shape = (np.array(out_kpmap_shape) * drawing_scale).astype(np.int32)
    kp_shape = np.array(kp2d_canvas_shape)
    scale_ratio = canvas_shape.min() / kp_shape.min()
    offset = (canvas_shape.min() - (kp_shape * scale_ratio).min()) / 2
    r, t = int(round(radius * scale_ratio)), int(round(thickness * scale_ratio))
    if t < 1:
        raise ValueError(f"thickness rounds to {t} on the canvas (scale {float(scale_ratio):.4g}): a line needs at least 1")
    H, W = int(canvas_shape[0]), int(canvas_shape[1])
    return MapParams(float(scale_ratio), float(offset), r, t, (H, W), (int(W / drawing_scale), int(H / drawing_scale)))


def plan_links(palette: Palette) -> List[Dict]:
    """The links in the order plan_draw_calls lists them: the palette's, then the X links whose ids it does not use."""
    return list(palette.links) + [{"id": lid, "link": link, "color": palette.x_link_color} for lid, link in X_LINKS
                                  if all(l["id"] != lid for l in palette.links)]


def plan_tables(palette, low_thr=0.5, high_thr=0.9) -> PlanTables:
    """The per-palette tables of dm4d_skeleton_plan_kp3d (include/dm4d.h), with plan_draw_calls' palette errors."""
    if isinstance(palette, PlanTables):
        return palette
    palette = load_palette(palette)
    links, k = plan_links(palette), len(palette.keypoint_colors)
    if max(max(l["link"]) for l in links) >= k:
        raise ValueError(f"a link joins keypoint {max(max(l['link']) for l in links)}, but the frame has {k} keypoints")
    if max(l["id"] for l in links) >= len(links):
        raise ValueError(f"link ids must be below the number of links ({len(links)}): the per-link arrays are indexed by id")
    if 3 * len(links) > ops.SKEL_MAX_PRIMS:
        raise ValueError(f"palette: {len(links)} links give {3 * len(links)} records a map, above SKEL_MAX_PRIMS = {ops.SKEL_MAX_PRIMS}")
    table = np.zeros((len(links), ops.SKEL_LINK_FIELDS), dtype=np.int32)
    for row, l in zip(table, links):
        mul = 2 if l["id"] < MAJOR_LINKS else 1
        row[:5] = (l["link"][0], l["link"][1], l["id"], mul, mul)
    colors = np.zeros((k + len(links), 4), dtype=np.float32)
    for row, c in zip(colors, list(palette.keypoint_colors) + [l["color"] for l in links]):
        if c is not None:
            row[:] = (*c, 1.0)
    return PlanTables(table, colors, float(np.float32(low_thr)), float(np.float32(high_thr)), float(np.float32(high_thr - low_thr)), k)


def plan_error(flags: int, tables: PlanTables) -> Optional[ValueError]:
    """The ValueError plan_draw_calls raises for a map whose status flag bits are `flags`, None when there is none."""
    if flags & ops.SKEL_ST_NONFINITE:
        return ValueError("a keypoint of a drawn link is not finite")
    if flags & ops.SKEL_ST_NOCOLOR:
        i1, i2, lid = tables.links[flags >> ops.SKEL_ST_LINK_SHIFT, :3].tolist()
        return ValueError(f"palette: link {lid} joins keypoints {i1} and {i2}, one of which has no colour")
    return None


class DeviceScene(NamedTuple):
    """A scene's poses_3d and cameras on the device: what every map of the scene is planned from."""
    kp3d: torch.Tensor                # fp64 [F, k, 3]
    K: torch.Tensor                   # fp64 [m, 3, 3]
    T: torch.Tensor                   # fp64 [m, 4, 4]


def upload_scene(kp3d, Ks, Ts, dev: torch.device) -> DeviceScene:
    """kp3d [F, k, 3], Ks [m, 3, 3], Ts [m, 4, 4] (numpy or tensors) as fp64 tensors on `dev`, once for every map of the scene."""
    def up(a):
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
        return t.to(device=dev, dtype=torch.float64).contiguous()
    kp3d, Ks, Ts = up(kp3d), up(Ks), up(Ts)
    if kp3d.dim() != 3 or kp3d.shape[2] != 3 or kp3d.numel() == 0:
        raise ValueError(f"kp3d must have shape (F, k, 3), got {tuple(kp3d.shape)}")
    if Ks.dim() != 3 or tuple(Ks.shape[1:]) != (3, 3) or Ks.shape[0] < 1:
        raise ValueError(f"Ks must have shape (n, 3, 3), got {tuple(Ks.shape)}")
    if tuple(Ts.shape) != (Ks.shape[0], 4, 4):
        raise ValueError(f"Ts must have shape (n, 4, 4), got {tuple(Ts.shape)}")
    return DeviceScene(kp3d, Ks, Ts)


class Kp3dJob(NamedTuple):
    """One map to plan on the device; canvas_shape and out_size as a DrawPlan names them (maps of one pair are drawn in one launch)."""
    frame: int                        # index into the scene's kp3d
    camera: int                       # index into the scene's cameras
    params: MapParams
    scores: Optional[np.ndarray] = None   # fp32 [k]: the score override

    @property
    def canvas_shape(self) -> Tuple[int, int]:
        return self.params.canvas_shape

    @property
    def out_size(self) -> Tuple[int, int]:
        return self.params.out_size


def plan_and_draw(scene: DeviceScene, jobs: Sequence[Kp3dJob], groups: Sequence[Tuple[int, int, Optional[torch.Tensor]]], tables: PlanTables):
    """One dm4d_skeleton_plan_kp3d launch for `jobs` and one dm4d_skeleton_draw_planned_u8 launch per group = (first job, number of
    jobs, uint8 [n, h, w, 3] tensor on the device to draw into or None), whose jobs share canvas_shape and out_size (cut along the maps
    as draw_plans is), on the current stream of scene's device; nothing is read back -> ([the maps per group], status int32
    [len(jobs), 2] on the device = {flag bits, dropped links}; plan_error explains the bits).  The maps of a job whose flag bits are set
    are drawn all the same (the records are in range by construction): the caller raises."""
    dev, n, k = scene.kp3d.device, len(jobs), scene.kp3d.shape[1]
    if n < 1 or n > 65535:
        raise ValueError(f"draw_skeleton_maps_kp3d: between 1 and 65535 maps a call, got {n}")
    if tables.n_keypoints != k:
        raise ValueError(f"the length of kpt_color ({tables.n_keypoints}) does not matches that of keypoints ({k})")
    jobs_h = torch.tensor([[j.frame, j.camera] for j in jobs], dtype=torch.int32)
    if int(jobs_h[:, 0].min()) < 0 or int(jobs_h[:, 0].max()) >= scene.kp3d.shape[0]:
        raise ValueError(f"jobs: a frame index outside [0, {scene.kp3d.shape[0]})")
    if int(jobs_h[:, 1].min()) < 0 or int(jobs_h[:, 1].max()) >= scene.K.shape[0]:
        raise ValueError(f"jobs: a camera index outside [0, {scene.K.shape[0]})")
    scale_h = torch.tensor([[j.params.scale_ratio, j.params.offset] for j in jobs], dtype=torch.float64)
    sizes_h = torch.tensor([[j.params.radius, j.params.thickness] for j in jobs], dtype=torch.int32)
    links_h, colors_h = torch.from_numpy(tables.links), torch.from_numpy(tables.colors)
    scores_d = None
    if any(j.scores is not None for j in jobs):
        rows = [np.ones(k, dtype=np.float32) if j.scores is None else np.asarray(j.scores, dtype=np.float32) for j in jobs]
        if any(r.shape != (k,) for r in rows):
            raise ValueError(f"scores must have shape ({n}, {k}), got a row of {next(r.shape for r in rows if r.shape != (k,))}")
        scores_d = torch.from_numpy(np.stack(rows)).to(dev)
    outs = []
    with torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext():
        records, counts, status = ops.skeleton_plan_kp3d(scene.kp3d, scene.K, scene.T, jobs_h, jobs_h.to(dev), scores_d, scale_h, scale_h.to(dev),
                                                         sizes_h, sizes_h.to(dev), links_h, links_h.to(dev), colors_h, colors_h.to(dev),
                                                         tables.low_thr, tables.high_thr, tables.thr_span)
        for start, count, out in groups:
            (H, W), (w, h) = jobs[start].canvas_shape, jobs[start].out_size
            if any(j.canvas_shape != (H, W) or j.out_size != (w, h) for j in jobs[start:start + count]):
                raise ValueError("draw_skeleton_maps_kp3d: the maps of one group must share the canvas shape and the output size")
            tabs = TableSet()
            (ho, hk), (vo, vk) = tabs.add(W, w), tabs.add(H, h)
            tab_h = torch.from_numpy(tabs.array())
            tab_d = tab_h.to(dev)
            htab_h, htab_d = (t[ho:ho + w * (2 + hk)] for t in (tab_h, tab_d))
            vtab_h, vtab_d = (t[vo:vo + h * (2 + vk)] for t in (tab_h, tab_d))
            if out is None:
                out = torch.empty((count, h, w, 3), dtype=torch.uint8, device=dev)
            if tuple(out.shape) != (count, h, w, 3):
                raise ValueError(f"draw_skeleton_maps_kp3d: out must be [{count}, {h}, {w}, 3], got {tuple(out.shape)}")
            step = max(1, LAUNCH_BYTES // (h * w * 3))
            for b0 in range(0, count, step):
                b1 = min(count, b0 + step)
                ops.skeleton_draw_planned(records[start + b0:start + b1], counts[start + b0:start + b1], htab_h, htab_d, hk, vtab_h, vtab_d, vk,
                                          H, W, h, w, out=out[b0:b1])
            outs.append(out)
    return outs, status


def _shape_pairs(shapes, n: int) -> List[Tuple[Tuple[int, int], Tuple[int, int]]]:
    """`shapes`: one (kp2d_canvas_shape, out_kpmap_shape) pair for all n maps, or one pair per map."""
    shapes = list(shapes)
    if len(shapes) == 2 and all(isinstance(v, (int, np.integer)) for v in shapes[0]):
        shapes = [shapes] * n
    if len(shapes) != n:
        raise ValueError(f"shapes: expected one (kp2d_canvas_shape, out_kpmap_shape) pair or {n} of them, got {len(shapes)}")
    return [(tuple(int(v) for v in c), tuple(int(v) for v in o)) for c, o in shapes]


def draw_skeleton_maps_kp3d(kp3d, Ks, Ts, jobs: Sequence[Tuple[int, int]], shapes, palette, scores=None, out=None, radius=2, thickness=2,
                            device="cuda"):
    """The maps of `jobs` = [(frame index, camera index)] straight from the scene's 3-D keypoints: kp3d [F, k, 3], Ks [m, 3, 3], Ts
    [m, 4, 4] (world -> camera, as triang.scene_cameras gives them; numpy, or fp64 tensors already on the device) are projected, planned
    and drawn on the device -- byte for byte draw_skeleton_maps on the poses_2d files triang.triangulate_skeleton writes for those
    frames and cameras.  `shapes`: one (kp2d_canvas_shape, out_kpmap_shape) pair, or one per job (the maps are grouped by shape: one
    draw launch per distinct pair); `palette`: a path, a Palette, or plan_tables(palette, low_thr, high_thr) for other thresholds;
    `scores` [len(jobs), k]: the score override (kp2d_score_dir's keypoint_scores).  One plan launch, one status read-back.

    -> (maps, dropped): maps uint8 [n, h, w, 3] (numpy) when all jobs share a shape, else a list of [h, w, 3] arrays in job order;
    with `out` (uint8 [n, h, w, 3] on the device; one shape only) the maps are drawn into it and it is returned instead, nothing but
    the status crosses PCIe.  dropped: int64 [n], the links left out per map because an endpoint lies outside [COORD_MIN, COORD_MAX].
    Raises plan_draw_calls' ValueError for the first map in job order that it would refuse."""
    tables = plan_tables(palette)
    n = len(jobs)
    pairs = _shape_pairs(shapes, n)
    for _, o in pairs:
        _check_out_shape(o)
    dev = out.device if out is not None else _l.hip_device(device, "draw_skeleton_maps_kp3d")
    scene = kp3d if isinstance(kp3d, DeviceScene) else upload_scene(kp3d, Ks, Ts, dev)
    if tables.n_keypoints != scene.kp3d.shape[1]:
        raise ValueError(f"the length of kpt_color ({tables.n_keypoints}) does not matches that of keypoints ({scene.kp3d.shape[1]})")
    by_shape: Dict[Tuple, List[int]] = {}
    for i, pair in enumerate(pairs):
        by_shape.setdefault(pair, []).append(i)
    if out is not None and len(by_shape) != 1:
        raise ValueError("draw_skeleton_maps_kp3d: out= takes maps of one shape")
    params = {pair: map_params(pair, radius, thickness) for pair in by_shape}  # raises in job order: a dict keeps first appearance
    if scores is not None:
        scores = np.asarray(scores, dtype=np.float32)
        if scores.shape != (n, tables.n_keypoints):
            raise ValueError(f"scores must have shape ({n}, {tables.n_keypoints}), got {scores.shape}")
    order = [i for idx in by_shape.values() for i in idx]
    planned = [Kp3dJob(int(jobs[i][0]), int(jobs[i][1]), params[pairs[i]], None if scores is None else scores[i]) for i in order]
    groups, start = [], 0
    for idx in by_shape.values():
        groups.append((start, len(idx), out))
        start += len(idx)
    outs, status = plan_and_draw(scene, planned, groups, tables)
    st = status.cpu().numpy()  # the one read-back; waits for the stream
    rows = np.empty_like(st)
    rows[order] = st
    for flags in rows[:, 0].tolist():
        err = plan_error(flags, tables)
        if err is not None:
            raise err
    dropped = rows[:, 1].astype(np.int64)
    if out is not None:
        return out, dropped
    host = [o.cpu().numpy() for o in outs]
    if len(host) == 1:
        return host[0], dropped
    maps: List = [None] * n
    for idx, arr in zip(by_shape.values(), host):
        for k_, i in enumerate(idx):
            maps[i] = arr[k_]
    return maps, dropped


def _read_scores(path) -> np.ndarray:
    return np.array(_read_instance(path)["keypoint_scores"], dtype=np.float32)


# -- a scene --------------------------------------------------------------------------------------------------------------------------
def _valid_image(path: str) -> bool:
    from PIL import Image
    try:
        Image.open(path).verify()
        return True
    except Exception as e:  # noqa: BLE001 -- whatever Pillow raises on a broken file: the reference redraws it
        print(f"Error reading {path}: {e}")
        return False


def _save(path: str, arr: np.ndarray, quality: int) -> None:
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(arr).save(path, quality=quality)


def _write(path: str, data: bytes) -> None:
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        f.write(data)


def draw_skeleton(kp2d_dir: Optional[str], out_kpmap_dir: str, kp2d_score_dir: Optional[str] = None, kp2d_canvas_shape=(1024, 1024),
                  out_kpmap_shape=(1024, 1024), spa_labels=None, tem_labels=None, image_ext: str = ".webp", image_quality: int = 85,
                  num_workers: int = 16, skip_exists: bool = False, palette=None, device="cuda", kp3d_dir: Optional[str] = None,
                  camera_path: Optional[str] = None, intri_scale: Optional[float] = None, *, device_webp: bool = False) -> Dict:
    """Draw every selected frame of a scene (draw_skeleton.py:182-226): reads ``kp2d_dir/{spa:02d}/{tem:06d}.json`` (and the scores of
    the same path under `kp2d_score_dir`) and writes ``out_kpmap_dir/{spa:02d}/{tem:06d}{image_ext}``.  Labels are lists of integers or
    default to the sorted listings of `kp2d_dir` and of its first camera, and the output path is the input path with `kp2d_dir`
    replaced by `out_kpmap_dir` and ".json" by `image_ext`, all as in the reference.  With `skip_exists` a file that Pillow's
    ``Image.open(path).verify()`` accepts is left untouched and a corrupt one is drawn again.

    Frames are read by a pool of `num_workers` threads (at most 16), drawn (one launch per 256 MiB of maps) and encoded with
    ``Image.save(path, quality=image_quality)`` by a second pool of as many; a batch is encoded while the next one is read and drawn.  host/imgwrite.py's package
    writer is not used: it skips a path that exists, and a corrupt file has to be replaced here.  Returns counts: frames, skipped,
    files, dropped_links (links left out because an endpoint lies outside [-8192, 8191] on the canvas; logged once), and seconds
    per phase (read, plan, launch, and write = the time the run waited for the encoder).

    With `kp3d_dir` (and `camera_path`, a nerfstudio transforms.json) the maps come straight from ``kp3d_dir/{tem:06d}.json`` and the
    cameras `spa_labels` of `camera_path` -- triang.scene_cameras(camera_path, labels, intri_scale): un-normalised, float32 inverse,
    as triangulate_skeleton builds them -- through draw_skeleton_maps_kp3d: `kp2d_dir` is not read and need not exist, and the files
    written are byte for byte those drawn from the poses_2d directory triangulate_skeleton(out_kp2d_proj_dir=...) writes.  Labels
    default to the sorted cameras of `camera_path` and the sorted listing of `kp3d_dir`.  The poses go up once; there is no plan phase.

    With `device_webp` a batch's maps stay on the device where they are drawn (both routes) and are encoded there as lossless WebP
    (host/webp.py; DESIGN.md "Device WebP (lossless)"): only the files' bytes cross PCIe, they are written verbatim, and they decode to
    exactly the maps draw_skeleton_maps returns.  `image_ext` must be ".webp"; `image_quality` is ignored (nothing is lost); seconds
    gains "encode" (the device encoder and the copy of its files), and "write" is the time waited for the file writes."""
    if device_webp and image_ext != ".webp":
        raise ValueError(f"draw_skeleton(device_webp=True) writes WebP files: image_ext must be '.webp', got {image_ext!r}")
    palette = load_palette(palette)
    _check_out_shape(out_kpmap_shape)
    dev = _l.hip_device(device, "draw_skeleton")
    from_kp3d = kp3d_dir is not None
    if from_kp3d and camera_path is None:
        raise ValueError("draw_skeleton(kp3d_dir=...) needs camera_path=: the transforms.json whose cameras the poses are projected into")
    if spa_labels is not None:
        spa_labels = [f"{spa_label:02d}" for spa_label in spa_labels]
    elif from_kp3d:
        from .capture import read_cameras
        spa_labels = sorted(read_cameras(camera_path, normalize_scene=False))
    else:
        spa_labels = sorted(os.listdir(kp2d_dir))
    if tem_labels is None:
        tem_labels = [tem_label.split(".")[0] for tem_label in sorted(os.listdir(kp3d_dir if from_kp3d else f"{kp2d_dir}/{spa_labels[0]}"))]
    else:
        tem_labels = [f"{tem_label:06d}" for tem_label in tem_labels]
    if from_kp3d:
        labels = [(c, f) for c in range(len(spa_labels)) for f in range(len(tem_labels))]  # cameras outermost, as the file route lists them
        out_paths = [f"{out_kpmap_dir}/{spa_labels[c]}/{tem_labels[f]}{image_ext}" for c, f in labels]
        score_paths = [f"{kp2d_score_dir}/{spa_labels[c]}/{tem_labels[f]}.json" if kp2d_score_dir is not None else None for c, f in labels]
    else:
        kp2d_paths = [f"{kp2d_dir}/{spa_label}/{tem_label}.json" for spa_label in spa_labels for tem_label in tem_labels]
        out_paths = [p.replace(kp2d_dir, out_kpmap_dir).replace(".json", image_ext) for p in kp2d_paths]
        score_paths = [p.replace(kp2d_dir, kp2d_score_dir) for p in kp2d_paths] if kp2d_score_dir is not None else [None] * len(kp2d_paths)

    todo = [i for i, p in enumerate(out_paths) if not (skip_exists and os.path.exists(p) and _valid_image(p))]
    counts = {"frames": len(todo), "skipped": len(out_paths) - len(todo), "files": 0, "dropped_links": 0}
    if not todo:
        return counts
    drawing_scale = DRAWING_SIZE / max(out_kpmap_shape)
    h, w = (int(int(s * drawing_scale) / drawing_scale) for s in out_kpmap_shape)
    step = max(1, LAUNCH_BYTES // (h * w * 3))
    stats: Dict = {}
    pending = []
    threads = max(1, min(int(num_workers), MAX_HOST_THREADS))
    # two pools: a batch's files are encoded (in Pillow, outside the interpreter lock) while the next batch is read, planned and drawn;
    # in one pool the reads would queue behind the encodes
    with ThreadPoolExecutor(max_workers=threads, thread_name_prefix="dm4d-skel-read") as readers, \
            ThreadPoolExecutor(max_workers=threads, thread_name_prefix="dm4d-skel-write") as writers:
        if from_kp3d:  # the frames that are drawn go up once, with the cameras; a batch then names them by index
            from . import triang
            t0 = time.perf_counter()
            used = sorted({labels[i][1] for i in todo})
            slot = {f: k for k, f in enumerate(used)}
            kp3d = np.stack(list(readers.map(read_kp3d, [f"{kp3d_dir}/{tem_labels[f]}.json" for f in used])))
            scene = upload_scene(kp3d, *triang.scene_cameras(camera_path, spa_labels, intri_scale), dev)
            tables = plan_tables(palette)
            stats["read"] = time.perf_counter() - t0
        for b0 in range(0, len(todo), step):
            idx = todo[b0:b0 + step]
            on_dev = torch.empty((len(idx), h, w, 3), dtype=torch.uint8, device=dev) if device_webp else None
            if from_kp3d:
                t0 = time.perf_counter()
                scores = None if kp2d_score_dir is None else np.stack(list(readers.map(_read_scores, [score_paths[i] for i in idx])))
                t1 = time.perf_counter()
                maps, dropped = draw_skeleton_maps_kp3d(scene, None, None, [(slot[labels[i][1]], labels[i][0]) for i in idx],
                                                        (kp2d_canvas_shape, out_kpmap_shape), tables, scores=scores, out=on_dev, device=dev)
                stats["read"] += t1 - t0
                stats["launch"] = stats.get("launch", 0.0) + time.perf_counter() - t1
                stats["dropped_links"] = stats.get("dropped_links", 0) + int(dropped.sum())
            else:
                maps = draw_skeleton_maps([kp2d_paths[i] for i in idx], [score_paths[i] for i in idx], kp2d_canvas_shape, out_kpmap_shape,
                                          palette=palette, device=dev, stats=stats, pool=readers, out=on_dev)
            if device_webp:
                from . import webp
                t0 = time.perf_counter()
                files = webp.encode_webp_batch(list(maps))  # synchronises
                stats["encode"] = stats.get("encode", 0.0) + time.perf_counter() - t0
            t0 = time.perf_counter()
            for f in pending:  # the previous batch's files; at most two batches of maps are alive
                f.result()
            stats["write"] = stats.get("write", 0.0) + time.perf_counter() - t0
            if device_webp:
                pending = [writers.submit(_write, out_paths[i], files[k]) for k, i in enumerate(idx)]
            else:
                pending = [writers.submit(_save, out_paths[i], maps[k], image_quality) for k, i in enumerate(idx)]
            counts["files"] += len(idx)
        t0 = time.perf_counter()
        for f in pending:
            f.result()
        stats["write"] = stats.get("write", 0.0) + time.perf_counter() - t0
    counts["dropped_links"] = stats.pop("dropped_links", 0)
    if counts["dropped_links"]:
        log.warning("draw_skeleton: %d links have an endpoint outside [%d, %d] on the canvas and were not drawn", counts["dropped_links"],
                    COORD_MIN, COORD_MAX)
    counts["seconds"] = {k: round(v, 4) for k, v in stats.items()}
    return counts
