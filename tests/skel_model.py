"""numpy restatement of the skeleton-map rasteriser (include/dm4d.h, dm4d_skeleton_draw_u8; DESIGN.md "Skeleton maps"): the reference of
tests/test_skel_cpu.py and tests/test_skel_gpu.py.  int64 throughout; every primitive is evaluated inside its bounding box only.

  circle(c, r)      covers (x - cx)^2 + (y - cy)^2 <= r^2
  line(p1, p2, t)   with d = p2 - p1, L2 = d . d, v = (x, y) - p1 covers the union of
                      0 <= v . d <= L2 and 4 (v x d)^2 <= t^2 L2        (only when L2 > 0)
                      4 |(x, y) - p1|^2 <= t^2
                      4 |(x, y) - p2|^2 <= t^2
  primitives are painted in list order: a pixel has the colour of the last one that covers it, black if none does

The expected map is Pillow's own reduction of that canvas: Image.fromarray(canvas).resize(out_size).
"""
import numpy as np
from PIL import Image


def _box(lo_x, hi_x, lo_y, hi_y, H, W):
    x0, x1, y0, y1 = max(lo_x, 0), min(hi_x, W - 1), max(lo_y, 0), min(hi_y, H - 1)
    if x0 > x1 or y0 > y1:
        return None
    ys, xs = np.mgrid[y0:y1 + 1, x0:x1 + 1].astype(np.int64)
    return (slice(y0, y1 + 1), slice(x0, x1 + 1)), xs, ys


def cover_circle(center, radius, H, W):
    """-> (index of the bounding box inside the canvas, bool mask over it) or None when the box misses the canvas."""
    cx, cy = center
    box = _box(cx - radius, cx + radius, cy - radius, cy + radius, H, W)
    if box is None:
        return None
    idx, xs, ys = box
    return idx, (xs - cx) ** 2 + (ys - cy) ** 2 <= radius * radius


def cover_line(p1, p2, thickness, H, W):
    (x1, y1), (x2, y2) = p1, p2
    g = (thickness + 1) // 2
    box = _box(min(x1, x2) - g, max(x1, x2) + g, min(y1, y2) - g, max(y1, y2) + g, H, W)
    if box is None:
        return None
    idx, xs, ys = box
    t2 = thickness * thickness
    vx, vy = xs - x1, ys - y1
    mask = (4 * (vx * vx + vy * vy) <= t2) | (4 * ((xs - x2) ** 2 + (ys - y2) ** 2) <= t2)
    dx, dy = x2 - x1, y2 - y1
    l2 = dx * dx + dy * dy
    if l2 > 0:
        dot = vx * dx + vy * dy
        cross = vx * dy - vy * dx
        mask |= (dot >= 0) & (dot <= l2) & (4 * cross * cross <= t2 * l2)
    return idx, mask


def paint(calls, canvas_shape) -> np.ndarray:
    """Draw calls (diffuman4d_amd.host.skeleton.plan_draw_calls' dictionaries) -> uint8 [H, W, 3]."""
    H, W = canvas_shape
    canvas = np.zeros((H, W, 3), dtype=np.uint8)
    for c in calls:
        hit = cover_line(c["p1"], c["p2"], c["thickness"], H, W) if c["type"] == "line" else cover_circle(c["center"], c["radius"], H, W)
        if hit is not None:
            idx, mask = hit
            canvas[idx][mask] = c["color"]
    return canvas


def expected_map(calls, canvas_shape, out_size) -> np.ndarray:
    """-> uint8 [h, w, 3]: the painted canvas reduced by Pillow (RGB, the default BICUBIC), out_size = (w, h)."""
    return np.asarray(Image.fromarray(paint(calls, canvas_shape)).resize(tuple(out_size)))
