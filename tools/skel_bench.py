#!/usr/bin/env python
"""Time skeleton-map drawing (diffuman4d_amd/host/skeleton.py) on a scene of the reference's size: 48 cameras x 150 frames = 7200
maps of 1024 x 1024, synthesised from the frames of tests/golden/triang_scene/ring8 (each frame's keypoints moved and turned a
little, fixed seed) and drawn with the palette tests/golden/skel_palette.json.

Measurements, written as JSON lines to --log (default profiles/skel_bench.log):
  kernel   dm4d_skeleton_draw_u8 alone, records and tables already on the device: HIP events around --inner launches of one batch
           (the batch draw_skeleton itself launches: 256 MiB of maps), after two warm-up launches, median of --reps windows -> time
           per map
  decode   reading and parsing all keypoint files in the pool of 16 threads, wall clock
  plan     plan_draw_calls over all frames (numpy, one thread), wall clock
  encode   Pillow's Image.save(quality=85) of one batch's maps: per image on one thread, and the batch through the pool of 16
  scene    draw_skeleton end to end with num_workers=16: wall clock, maps per second, and its own seconds per phase
  imagedraw  for information only: the share of pixels in which a map differs from one painted by Pillow's ImageDraw (lines with a
           width, filled ellipses: an independent rasteriser, not the reference's OpenCV) and reduced the same way

  python tools/skel_bench.py [--cameras 48 --frames 150 --reps 5]
"""
from __future__ import annotations

import argparse
import json
import math
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from diffuman4d_amd.host import ops, skeleton  # noqa: E402
from diffuman4d_amd.host.capture import bicubic_table  # noqa: E402

RING8 = ROOT / "tests" / "golden" / "triang_scene" / "ring8" / "poses_sapiens"
SHAPES = ((1024, 1024), (1024, 1024))


def write_scene(root: Path, cameras: int, frames: int, seed: int = 0) -> None:
    """poses_2d/{cam}/{frame}.json: a ring8 frame turned about the image centre by up to +-0.3 rad and moved by up to +-60 px."""
    base = [json.loads(p.read_text())["instance_info"][0] for p in sorted(RING8.rglob("*.json"))]
    rng = np.random.default_rng(seed)
    for c in range(cameras):
        d = root / "poses_2d" / f"{c:02d}"
        d.mkdir(parents=True)
        for t in range(frames):
            src = base[(c * frames + t) % len(base)]
            a = rng.uniform(-0.3, 0.3)
            rot = np.array([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]])
            kp = (np.array(src["keypoints"]) - 512.0) @ rot.T + 512.0 + rng.uniform(-60, 60, size=2)
            inst = {"keypoints": np.round(kp, 2).tolist(), "keypoint_scores": src["keypoint_scores"]}
            (d / f"{t:06d}.json").write_text(json.dumps({"instance_info": [inst]}))


def imagedraw_map(plan) -> np.ndarray:
    from PIL import Image, ImageDraw
    H, W = plan.canvas_shape
    im = Image.new("RGB", (W, H))
    draw = ImageDraw.Draw(im)
    for c in plan.calls:
        if c["type"] == "line":
            draw.line([tuple(c["p1"]), tuple(c["p2"])], fill=tuple(c["color"]), width=c["thickness"])
        else:
            (x, y), r = c["center"], c["radius"]
            draw.ellipse([x - r, y - r, x + r, y + r], fill=tuple(c["color"]))
    return np.asarray(im.resize(plan.out_size))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cameras", type=int, default=48)
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10, help="launches per timed window")
    ap.add_argument("--num_workers", type=int, default=16)
    ap.add_argument("--palette", default=str(ROOT / "tests" / "golden" / "skel_palette.json"))
    ap.add_argument("--log", default=str(ROOT / "profiles" / "skel_bench.log"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("skel_bench needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda", torch.cuda.current_device())
    palette = skeleton.load_palette(args.palette)
    n_maps = args.cameras * args.frames
    rows = [{"cameras": args.cameras, "frames": args.frames, "maps": n_maps, "map_shape": [1024, 1024], "seed": 0,
             "device": torch.cuda.get_device_name(dev), "host_threads": min(args.num_workers, skeleton.MAX_HOST_THREADS)}]

    with tempfile.TemporaryDirectory() as tmp:
        root = Path(tmp)
        write_scene(root, args.cameras, args.frames)
        paths = [str(p) for p in sorted((root / "poses_2d").rglob("*.json"))]

        with ThreadPoolExecutor(max_workers=min(args.num_workers, skeleton.MAX_HOST_THREADS)) as pool:
            list(pool.map(skeleton._read_instance, paths))  # warms the file cache
            t0 = time.perf_counter()
            instances = list(pool.map(skeleton._read_instance, paths))
            decode_s = time.perf_counter() - t0
        rows.append({"measure": "decode", "what": "json.load of every keypoint file in the thread pool, wall clock", "seconds": round(decode_s, 4),
                     "ms_per_map": round(1e3 * decode_s / n_maps, 4)})

        t0 = time.perf_counter()
        plans = [skeleton.plan_draw_calls(inst, None, SHAPES, palette) for inst in instances]
        plan_s = time.perf_counter() - t0
        rows.append({"measure": "plan", "what": "plan_draw_calls of every frame, one thread, wall clock", "seconds": round(plan_s, 4),
                     "ms_per_map": round(1e3 * plan_s / n_maps, 4), "mean_primitives": round(float(np.mean([len(p.calls) for p in plans])), 1)})

        # the kernel alone: one batch as draw_plans launches it
        (H, W), (w, h) = plans[0].canvas_shape, plans[0].out_size
        batch = plans[:max(1, min(len(plans), skeleton.LAUNCH_BYTES // (h * w * 3)))]
        hb, hk = bicubic_table(W, w)
        vb, vk = bicubic_table(H, h)
        htab = torch.from_numpy(np.concatenate([hb.reshape(-1), hk.reshape(-1)]).astype(np.int32))
        vtab = torch.from_numpy(np.concatenate([vb.reshape(-1), vk.reshape(-1)]).astype(np.int32))
        recs = [skeleton.pack_calls(p.calls) for p in batch]
        offsets = torch.from_numpy(np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int32))
        prims = torch.from_numpy(np.concatenate(recs + [np.zeros((1, ops.SKEL_FIELDS), dtype=np.int32)]))
        prims_d, offsets_d, htab_d, vtab_d = prims.to(dev), offsets.to(dev), htab.to(dev), vtab.to(dev)

        def launch():
            return ops.skeleton_draw(prims, prims_d, offsets, offsets_d, htab, htab_d, hk.shape[1], vtab, vtab_d, vk.shape[1], H, W, h, w)

        for _ in range(2):
            maps_d = launch()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(args.inner):
                maps_d = launch()
            e.record()
            e.synchronize()
            ms.append(s.elapsed_time(e) / args.inner)
        med = statistics.median(ms)
        rows.append({"measure": "kernel", "what": "dm4d_skeleton_draw_u8, HIP events over %d launches (each includes the entry's host-side "
                     "validation), median of %d" % (args.inner, args.reps), "maps_per_launch": len(batch), "ms_per_launch": round(med, 4),
                     "ms_per_launch_range": [round(min(ms), 4), round(max(ms), 4)], "us_per_map": round(1e3 * med / len(batch), 3),
                     "output_gb_per_s": round(len(batch) * h * w * 3 / (med * 1e-3) / 1e9, 2)})

        maps = maps_d.cpu().numpy()
        enc = root / "encode"
        t0 = time.perf_counter()
        for k in range(min(8, len(maps))):
            skeleton._save(str(enc / "single" / f"{k}.webp"), maps[k], 85)
        single_ms = 1e3 * (time.perf_counter() - t0) / min(8, len(maps))
        with ThreadPoolExecutor(max_workers=min(args.num_workers, skeleton.MAX_HOST_THREADS)) as pool:
            t0 = time.perf_counter()
            list(pool.map(lambda k: skeleton._save(str(enc / "pool" / f"{k}.webp"), maps[k], 85), range(len(maps))))
            pool_s = time.perf_counter() - t0
        rows.append({"measure": "encode", "what": "Image.save(quality=85) to .webp: one thread per image; one batch through the thread pool",
                     "ms_per_map_one_thread": round(single_ms, 3), "maps": len(maps), "pool_seconds": round(pool_s, 4),
                     "ms_per_map_pool": round(1e3 * pool_s / len(maps), 3)})

        runs = []
        for rep in range(2):  # the first run warms the code objects and the file cache: not counted
            t0 = time.perf_counter()
            res = skeleton.draw_skeleton(str(root / "poses_2d"), str(root / f"skeletons_{rep}"), palette=palette, num_workers=args.num_workers,
                                         device=dev)
            res["seconds"]["total"] = round(time.perf_counter() - t0, 4)
            runs.append(res)
        res = runs[-1]
        rows.append({"measure": "scene", "what": "draw_skeleton end to end, wall clock, second of two runs; launch = uploads, launch, download; "
                     "write = the time the run waited for the encoder, which works beside the other phases", **res["seconds"],
                     "files": res["files"], "maps_per_second": round(res["files"] / res["seconds"]["total"], 1)})

        shares, painted, diffs = [], [], []
        for p, m in list(zip(batch, maps))[:8]:
            other = imagedraw_map(p)
            differ = (other != m).any(axis=-1)
            shares.append(float(differ.mean()))
            painted.append(float((m.any(axis=-1) | other.any(axis=-1)).mean()))
            diffs.append(float(np.abs(other.astype(np.int32) - m.astype(np.int32))[differ].mean()) if differ.any() else 0.0)
        rows.append({"measure": "imagedraw", "what": "share of map pixels that differ from Pillow's ImageDraw painting of the same calls, reduced "
                     "the same way; an independent rasteriser, for information only (OpenCV is not a dependency: the distance to it is not measured)",
                     "maps": len(shares), "mean_share": round(float(np.mean(shares)), 6), "max_share": round(float(np.max(shares)), 6),
                     "mean_share_of_pixels_painted_by_either": round(float(np.mean(painted)), 6),
                     "mean_abs_difference_where_they_differ": round(float(np.mean(diffs)), 2)})

    Path(args.log).parent.mkdir(parents=True, exist_ok=True)
    with open(args.log, "w") as f:
        for row in rows:
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
