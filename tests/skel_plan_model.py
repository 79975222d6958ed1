"""numpy restatement of dm4d_skeleton_plan_kp3d (include/dm4d.h; DESIGN.md "Skeleton maps from poses_3d"), stepwise in the kernel's own
operand widths: the reference of tests/test_skel_plan_cpu.py and tests/test_skel_plan_gpu.py.  It is written from the kernel's
definition with explicit dtypes and loops, not by calling host/skeleton.py plan_draw_calls: the CPU test holds it against
pack_calls(plan_draw_calls(.)) of the file route, the GPU test holds the kernel against both.

Input is what the shared projection gives for one map: uv fp64 [k, 2], depth fp64 [k] (dm4d_project_points_f64, or
triang_model.project on the host).
"""
import numpy as np

COORD_MIN, COORD_MAX = -8192, 8191
LINE, CIRCLE = 0, 1
ST_NONFINITE, ST_NOCOLOR, ST_LINK_SHIFT = 1, 2, 8

f32, f64 = np.float32, np.float64


def _dim(rgb, score, low, high, span):
    """c * ((clip(score, low, high) - low) / span) per channel in fp32, rint, uint8 -> r | g << 8 | b << 16."""
    clipped = score if np.isnan(score) else min(max(score, low), high)
    norm = f32(f32(clipped - low) / span)
    out = 0
    for c in range(3):
        v = np.rint(f32(f32(rgb[c]) * norm))
        out |= (255 if v >= 255 else int(v) if v > 0 else 0) << (8 * c)
    return out


def _min_nan(a, b):
    return a if np.isnan(a) else b if np.isnan(b) else min(a, b)


def plan(uv, depth, scores, scale_ratio, offset, radius, thickness, links, colors, low, high, span):
    """-> (records int32 [count, 8], flag bits, dropped links).  links int32 [L, 8] and colors fp32 [k + L, 4] as the kernel takes them;
    scores fp32 [k] or None; low, high, span: the three fp32 thresholds."""
    k, L = len(uv), len(links)
    low, high, span = f32(low), f32(high), f32(span)
    x, y, flag = np.zeros(k, np.int64), np.zeros(k, np.int64), np.zeros(k, np.int64)
    score, dep = np.ones(k, f32), np.zeros(k, f32)
    with np.errstate(all="ignore"):
        for i in range(k):
            uf, vf, dep[i] = f32(uv[i, 0]), f32(uv[i, 1]), f32(depth[i])
            if scores is not None:
                score[i] = f32(scores[i])
            if not np.isnan(uf) and not np.isnan(vf) and (uf < 0 or vf < 0):
                score[i] = f32(0)
            xs = f64(f64(uf) * f64(scale_ratio)) + f64(offset)   # two roundings: no fused multiply-add
            ys = f64(f64(vf) * f64(scale_ratio)) + f64(offset)
            rx, ry = np.rint(xs), np.rint(ys)
            if np.isfinite(xs) and np.isfinite(ys):
                flag[i] |= 1
            if COORD_MIN <= rx <= COORD_MAX and COORD_MIN <= ry <= COORD_MAX:
                flag[i] |= 2
                x[i], y[i] = int(rx), int(ry)
        by_depth = bool(any(d != 0 for d in dep))          # a NaN differs from 0
        by_score = not by_depth and bool(any(s != 1 for s in score))

        keep, key, line_score = [False] * L, [0.0] * L, [f32(0)] * L
        bits, dropped, first_nocolor = 0, 0, None
        for l in range(L):
            i1, i2 = int(links[l, 0]), int(links[l, 1])
            line_score[l] = _min_nan(score[i1], score[i2])
            kept = not (line_score[l] < low)
            if kept and not (flag[i1] & flag[i2] & 1):
                bits |= ST_NONFINITE
            inside = bool(flag[i1] & flag[i2] & 2)
            if kept and not inside:
                dropped += 1
            kept = kept and inside
            if kept and (colors[i1, 3] == 0 or colors[i2, 3] == 0) and first_nocolor is None:
                first_nocolor = l
            key[l] = -((f64(dep[i1]) + f64(dep[i2])) / 2) if by_depth else f64(line_score[l]) if by_score else 0.0
            keep[l] = kept
        if first_nocolor is not None:
            bits |= ST_NOCOLOR | (first_nocolor << ST_LINK_SHIFT)

        n_keep = sum(keep)
        records = np.zeros((3 * n_keep, 8), np.int64)
        for l in range(L):
            if not keep[l]:
                continue
            rank = sum(1 for j in range(L) if keep[j] and (key[j] < key[l] or (key[j] == key[l] and j < l)))
            i1, i2 = int(links[l, 0]), int(links[l, 1])
            records[3 * rank] = (LINE, x[i1], y[i1], x[i2], y[i2], thickness * links[l, 4], _dim(colors[k + l], line_score[l], low, high, span), 0)
            records[3 * rank + 1] = (CIRCLE, x[i1], y[i1], x[i1], y[i1], radius * links[l, 3], _dim(colors[i1], score[i1], low, high, span), 0)
            records[3 * rank + 2] = (CIRCLE, x[i2], y[i2], x[i2], y[i2], radius * links[l, 3], _dim(colors[i2], score[i2], low, high, span), 0)
    return records.astype(np.int32), bits, dropped
