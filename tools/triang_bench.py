#!/usr/bin/env python
"""Time skeleton triangulation (diffuman4d_amd/host/triang.py) on a synthetic scene of the reference's size: 48 views x 150 frames x
133 keypoints, fixed seed (cameras on a ring, a body's keypoints projected with 1 px of Gaussian noise, gross outliers in a few
views, varied scores).

Two measurements, appended as JSON lines to --log (default profiles/triang_bench.log):
  scene    triangulate_skeleton on the scene written as poses_sapiens/{cam}/{frame}.json files in a temporary directory: wall clock of
           its three phases (read = 7200 JSON files in the thread pool; launch = uploads, the two launches, downloads; write = 150 +
           7200 JSON files), the median of --reps runs
  kernels  the two launches alone with the inputs already on the device, HIP events, the median of --reps
For scale only, the fixture's record of the reference's CPU seconds per frame (tests/golden/triang_reference.pt; 8 and 30 views,
measured on the machine that recorded the fixture, not on this one) is quoted beside them.

  python tools/triang_bench.py [--views 48 --frames 150 --reps 5]
"""
from __future__ import annotations

import argparse
import json
import math
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from diffuman4d_amd.host import ops, triang  # noqa: E402

K_POINTS = 133


def scene(views: int, frames: int, seed: int = 0):
    """-> (transforms.json dict, kp2d [frames, views, 133, 2], score [frames, views, 133])."""
    rng = np.random.default_rng(seed)
    tf, Ks, Ts = [], [], []
    for c in range(views):
        a = 2 * math.pi * c / views + 0.3
        o = np.array([2.8 * math.cos(a), 0.1 + 0.25 * math.sin(2 * a), 2.8 * math.sin(a)])
        back = o / np.linalg.norm(o)
        right = np.cross([0.0, 1.0, 0.0], back)
        right /= np.linalg.norm(right)
        m = np.eye(4)
        m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = right, np.cross(back, right), back, o
        fx, fy, cx, cy = 1100.0 + 7.5 * (c % 11), 1104.25 + 6.5 * (c % 7), 509.3 + 1.45 * (c % 5), 515.6 - 1.35 * (c % 9)
        tf.append({"camera_label": f"{c:02d}", "h": 1024, "w": 1024, "fl_x": fx, "fl_y": fy, "cx": cx, "cy": cy, "transform_matrix": m.tolist()})
        c2w = m.copy()
        c2w[:3, 1:3] *= -1
        Ks.append(np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]]))
        Ts.append(np.linalg.inv(c2w))
    P = np.stack(Ks) @ np.stack(Ts)[:, :3]
    base = rng.uniform([-0.4, -0.9, -0.25], [0.4, 0.8, 0.25], size=(K_POINTS, 3))
    kp2d = np.empty((frames, views, K_POINTS, 2))
    for t in range(frames):
        pts = base + 0.2 * np.array([math.sin(0.05 * t), 0.1 * math.sin(0.11 * t), math.cos(0.07 * t)])
        h = np.einsum("nrc,kc->nkr", P[:, :, :3], pts) + P[:, None, :, 3]
        kp2d[t] = h[..., :2] / h[..., 2:3]
    kp2d += rng.standard_normal(kp2d.shape)
    out = rng.random(kp2d.shape[:3]) < 0.01  # gross outliers: 1 % of the observations
    kp2d[out] += rng.uniform(-60, 60, size=(int(out.sum()), 2))
    score = rng.uniform(0.45, 1.0, size=kp2d.shape[:3])
    score[:, :, 91] = rng.uniform(0.93, 1.0, size=(frames, views))
    score[:, :, 112] = rng.uniform(0.8, 1.0, size=(frames, views))
    return {"w": 1024, "h": 1024, "frames": tf}, kp2d, score


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--views", type=int, default=48)
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--num_workers", type=int, default=16)
    ap.add_argument("--log", default=str(ROOT / "profiles" / "triang_bench.log"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("triang_bench needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda", torch.cuda.current_device())
    tf, kp2d, score = scene(args.views, args.frames)
    rows = [{"views": args.views, "frames": args.frames, "keypoints": K_POINTS, "problems": args.frames * K_POINTS, "seed": 0,
             "device": torch.cuda.get_device_name(dev)}]

    with tempfile.TemporaryDirectory() as tmp:
        root = Path(tmp)
        (root / "transforms.json").write_text(json.dumps(tf))
        for c in range(args.views):
            d = root / "poses_sapiens" / f"{c:02d}"
            d.mkdir(parents=True)
            for t in range(args.frames):
                inst = {"keypoints": np.round(kp2d[t, c], 2).tolist(), "keypoint_scores": np.round(score[t, c], 3).tolist()}
                (d / f"{t:06d}.json").write_text(json.dumps({"instance_info": [inst]}))
        runs = []
        for rep in range(args.reps + 1):  # the first run loads the code objects and warms the file cache: not counted
            t0 = time.perf_counter()
            res = triang.triangulate_skeleton(str(root / "transforms.json"), str(root / "poses_sapiens"), str(root / f"poses_3d_{rep}"),
                                              out_kp2d_proj_dir=str(root / f"poses_2d_{rep}"), num_workers=args.num_workers, device=dev)
            res["seconds"]["total"] = round(time.perf_counter() - t0, 4)
            if rep:
                runs.append(res)
        med = {k: statistics.median(r["seconds"][k] for r in runs) for k in ("read", "launch", "write", "total")}
        rows.append({"measure": "scene", "what": "triangulate_skeleton, wall clock seconds, median of %d" % args.reps, **med,
                     "files_read": args.views * args.frames, "files_written": runs[0]["files"], "valid_keypoints": runs[0]["valid"],
                     "host_threads": min(args.num_workers, triang.MAX_HOST_THREADS), "seconds_per_frame": round(med["total"] / args.frames, 5)})

    # the launches alone: what read_kp2d gives (the finger rescale applied), already on the device
    with tempfile.TemporaryDirectory() as tmp:
        (Path(tmp) / "transforms.json").write_text(json.dumps(tf))
        Ks, Ts = triang.scene_cameras(str(Path(tmp) / "transforms.json"), [f"{c:02d}" for c in range(args.views)])
    sc = np.round(score, 3)
    sc[:, :, 92:112] *= sc[:, :, 91:92] ** 2
    sc[:, :, 113:133] *= sc[:, :, 112:113] ** 2
    thr = triang.score_thresholds(sc)
    K_d, T_d = torch.from_numpy(Ks).to(dev), torch.from_numpy(Ts).to(dev)
    kp_d, sc_d, thr_d = torch.from_numpy(np.round(kp2d, 2)).to(dev), torch.from_numpy(sc).to(dev), torch.from_numpy(thr).to(dev)

    def timed(fn):
        for _ in range(2):
            out = fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out = fn()
            e.record()
            e.synchronize()
            ms.append(s.elapsed_time(e))
        return out, statistics.median(ms), min(ms), max(ms)

    (kp3d, _, n_views), t_ms, t_lo, t_hi = timed(lambda: ops.triangulate_points(K_d, T_d, kp_d, sc_d, thr_d, 3))
    _, p_ms, p_lo, p_hi = timed(lambda: ops.project_points(kp3d, K_d, T_d))
    rows.append({"measure": "kernels", "what": "HIP events, inputs on the device, milliseconds, median of %d" % args.reps,
                 "triangulate_ms": round(t_ms, 3), "triangulate_ms_range": [round(t_lo, 3), round(t_hi, 3)], "project_ms": round(p_ms, 3),
                 "project_ms_range": [round(p_lo, 3), round(p_hi, 3)], "problems_per_ms": round(args.frames * K_POINTS / t_ms, 1),
                 "mean_views_selected": round(float(n_views.float().mean()), 2), "valid_keypoints": int((n_views >= 3).sum())})

    fixture = ROOT / "tests" / "golden" / "triang_reference.pt"
    if fixture.exists():
        ref = torch.load(fixture, weights_only=False)["scenes"]
        rows.append({"measure": "reference", "what": "the reference's CPU seconds per frame as recorded in the fixture: measured on a DIFFERENT "
                     "machine (the one that recorded the fixture), for scale only",
                     **{f"{name}_views{len(s['labels'])}_seconds_per_frame": round(s["ref_cpu_seconds_per_frame"], 4) for name, s in ref.items()}})
    Path(args.log).parent.mkdir(parents=True, exist_ok=True)
    with open(args.log, "w") as f:
        for row in rows:
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
