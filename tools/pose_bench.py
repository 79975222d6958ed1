#!/usr/bin/env python
"""Time the keypoint stage's own arithmetic (diffuman4d_amd/host/pose.py, csrc/pose.hip) at the reference's sizes: 133 heatmaps of
256 x 192 per image, and the network input 1024 x 1024 -> 1024 x 768.  The pose network itself is the caller's and is not timed.

Measurements, written as JSON lines to --log (default profiles/pose_bench.log):
  decode    dm4d_pose_udp_decode_f32 on --batch images' heatmaps already on the device (Gaussian peaks with 1 % noise, fixed seed): HIP
            events around a window of launches that lasts about --window seconds (at least --inner launches), after two warm-up
            launches, median of --reps windows -> time per image.  Taken twice: on one buffer, which the launches re-read from the
            256 MB Infinity Cache ("cache_warm"), and in turn on --rotate copies of it at different addresses, together larger than
            that cache, as a network's fresh output would be ("rotating")
  input     dm4d_pose_input_u8_f32 on --batch staged images with masks, the same way -> time per image
  maskbox   dm4d_pose_mask_box_u8 on the same masks, the same way -> time per mask
  stage     pose_inputs end to end from arrays (staging copy, upload, tables, launch), wall clock ending in a synchronise
  numpy     the model of tests/pose_model.py (numpy + scipy, float32) on --numpy_maps of one image's heatmaps, one thread and a pool
            of 16 threads, wall clock -> time per image of 133 maps; what the device kernel is compared against
  cv2       with --cv2: the share of values in which the network input differs from OpenCV's own warpAffine + the reference's
            normalisation, and the largest difference in 8-bit steps; "not measured" where cv2 does not import

  python tools/pose_bench.py [--batch 4 --reps 7 --window 0.5 --rotate 6 --cv2]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from diffuman4d_amd.host import ops, pose, staging  # noqa: E402

K, HH, WH = 133, 256, 192
SHAPE = (1024, 768)
SRC = (1024, 1024)


def heatmaps(n: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:HH, 0:WH].astype(np.float32)
    out = np.empty((n, K, HH, WH), dtype=np.float32)
    for i in range(n):
        for k in range(K):
            cx, cy, amp = rng.uniform(4, WH - 5), rng.uniform(4, HH - 5), rng.uniform(0.2, 1.0)
            out[i, k] = amp * np.exp(-((xs - cx) ** 2 + (ys - cy) ** 2) / 8.0) + amp * 0.01 * rng.random((HH, WH), dtype=np.float32)
    return out


def device_time(fn, reps: int, inner: int, window: float) -> tuple:
    """Median over `reps` windows of the HIP-event time per launch, in seconds -> (time, launches per window).  A window holds at least
    `inner` launches and enough of them to last about `window` seconds, counted from a first short window that is not kept."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()

    def one(count: int) -> float:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(count):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / 1e3 / count
    count = max(inner, int(window / one(inner)) + 1)
    return statistics.median(one(count) for _ in range(reps)), count


def cv2_distance(image: np.ndarray, mask: np.ndarray, x: np.ndarray) -> dict:
    try:
        import cv2
    except ImportError:
        return {"what": "cv2", "result": "not measured (cv2 does not import here)"}
    from PIL import Image
    comp = np.asarray(Image.composite(Image.fromarray(image), Image.new("RGB", image.shape[1::-1]), Image.fromarray(mask)))
    c, s = pose.box_center_scale([0, 0, image.shape[1], image.shape[0]], SHAPE)
    warped = cv2.warpAffine(comp, pose.udp_warp_matrix(c, s, SHAPE), (SHAPE[1], SHAPE[0]), flags=cv2.INTER_LINEAR)
    ref = (torch.from_numpy(warped.transpose(2, 0, 1).copy()).float() - torch.tensor(pose.MEAN).view(-1, 1, 1)) / torch.tensor(pose.STD).view(-1, 1, 1)
    diff = np.abs(x - ref.numpy()) * np.array(pose.STD, dtype=np.float32).reshape(3, 1, 1)
    return {"what": "cv2", "cv2": cv2.__version__, "share_of_values_that_differ": float(np.mean(diff > 0)), "max_difference_8bit_steps": float(diff.max())}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=300, help="launches per timed window at least")
    ap.add_argument("--window", type=float, default=0.5, help="seconds a timed window lasts, about")
    ap.add_argument("--rotate", type=int, default=6, help="copies of the heatmaps the rotating decode measurement goes through")
    ap.add_argument("--numpy_maps", type=int, default=32, help="maps the numpy model decodes (its time is scaled to 133)")
    ap.add_argument("--cv2", action="store_true")
    ap.add_argument("--log", default=str(ROOT / "profiles" / "pose_bench.log"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("pose_bench needs a HIP device: a time taken elsewhere says nothing")
    import pose_model as M
    dev = torch.device("cuda", torch.cuda.current_device())
    lines = [{"what": "setup", "device": torch.cuda.get_device_name(dev), "batch": args.batch, "heatmaps": [K, HH, WH], "input": list(SHAPE),
              "source": list(SRC), "reps": args.reps, "window_seconds": args.window,
              "rotate": args.rotate}]

    heat_host = heatmaps(args.batch)
    heat = torch.from_numpy(heat_host).to(dev)
    bufs = [heat] + [heat.clone() for _ in range(max(args.rotate, 1) - 1)]
    turn = [0]

    def rotating():
        turn[0] = (turn[0] + 1) % len(bufs)
        ops.pose_udp_decode(bufs[turn[0]])
    for what, fn in (("cache_warm", lambda: ops.pose_udp_decode(heat)), ("rotating", rotating)):
        t, count = device_time(fn, args.reps, args.inner, args.window)
        lines.append({"what": "decode", "heatmaps": what, "seconds_per_image": t / args.batch, "images_per_second": args.batch / t,
                      "heatmap_bytes_per_second": heat.numel() * 4 / t, "launches_per_window": count,
                      "bytes_rotated_through": heat.numel() * 4 * (len(bufs) if what == "rotating" else 1)})
    del bufs
    locs, scores = (a.cpu().numpy() for a in ops.pose_udp_decode(heat))

    rng = np.random.default_rng(1)
    images = [rng.integers(0, 256, SRC + (3,), dtype=np.uint8) for _ in range(args.batch)]
    ys, xs = np.mgrid[0:SRC[0], 0:SRC[1]]
    masks = [(255 * (((xs - 512) / (200 + 20 * i)) ** 2 + ((ys - 540) / 430) ** 2 < 1)).astype(np.uint8) for i in range(args.batch)]
    sizes = [SRC] * args.batch
    image_off, mask_off, total = pose.plane_layout(sizes, True, [True] * args.batch)
    host = staging.pinned(total, dev)
    staging.fill(host.numpy(), list(zip(image_off + mask_off, images + masks)), None)
    blob = host.to(dev)
    tab = np.concatenate([pose.warp_tables(pose.udp_warp_matrix(*pose.box_center_scale([0, 0, SRC[1], SRC[0]], SHAPE), SHAPE), SHAPE)] * args.batch)
    per_row = 2 * (SHAPE[0] + SHAPE[1])
    desc = pose.descriptors([(k, k * per_row) for k in range(args.batch)], sizes, image_off, mask_off)
    meta, meta_host, tab_off, tab_len, desc_off = staging.pack_meta(tab, desc, dev)
    norm = torch.tensor(pose.MEAN + pose.STD, dtype=torch.float32)
    t, count = device_time(lambda: ops.pose_input(blob, meta, meta_host, args.batch, desc_off, tab_off, tab_len, SHAPE[0], SHAPE[1], norm),
                           args.reps, args.inner, args.window)
    out_bytes = 3 * SHAPE[0] * SHAPE[1] * 4
    lines.append({"what": "input", "seconds_per_image": t / args.batch, "images_per_second": args.batch / t,
                  "output_bytes_per_second": out_bytes * args.batch / t, "launches_per_window": count,
                  "note": "the sources (16 MB) stay in the Infinity Cache between launches"})
    t, count = device_time(lambda: ops.pose_mask_box(blob, meta, meta_host, args.batch, desc_off), args.reps, args.inner, args.window)
    lines.append({"what": "maskbox", "seconds_per_mask": t / args.batch, "mask_bytes_per_second": SRC[0] * SRC[1] * args.batch / t,
                  "launches_per_window": count})

    wall = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        x, _, _ = pose.pose_inputs(images, masks, None, SHAPE, dev)
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t0)
    lines.append({"what": "stage", "seconds_per_image": statistics.median(wall) / args.batch, "note": "arrays in memory: no file decode"})

    n = min(args.numpy_maps, K)
    t0 = time.perf_counter()
    l32, _ = M.udp_decode(heat_host[0, :n], np.float32)
    one = (time.perf_counter() - t0) / n * K
    chunks = [heat_host[0, i: i + 2] for i in range(0, n, 2)]
    with ThreadPoolExecutor(max_workers=16) as pool:
        t0 = time.perf_counter()
        list(pool.map(lambda c: M.udp_decode(c, np.float32), chunks))
        sixteen = (time.perf_counter() - t0) / n * K
    lines.append({"what": "numpy", "maps": n, "seconds_per_image_1_thread": one, "seconds_per_image_16_threads": sixteen,
                  "max_distance_device_to_model_fp32": float(np.abs(locs[0, :n] - l32).max())})
    if args.cv2:
        lines.append(cv2_distance(images[0], masks[0], x[0].cpu().numpy()))
    else:
        lines.append({"what": "cv2", "result": "not measured (run with --cv2 where cv2 imports)"})
    Path(args.log).parent.mkdir(parents=True, exist_ok=True)
    with open(args.log, "w") as f:
        for line in lines:
            print(json.dumps(line))
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
