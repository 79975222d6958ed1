#!/usr/bin/env python
"""Time the person-box stage's own arithmetic (diffuman4d_amd/host/detect.py, csrc/detect.hip): 48 images of 2448 x 2048 and of
1024 x 1024 with masks, in batches of 8, into a 640 x 640 canvas, and a dense output of A = 8400 anchors per image.  The detector and
the pose network are the caller's and are not timed: stand-ins take their place.

Measurements, written as JSON lines to --log (default profiles/detect_bench.log):
  input     dm4d_detect_input_u8_f32 on the 6 staged batches: HIP events around a window of passes over all 48 images that lasts about
            --window seconds, after a warm-up pass, median of --reps windows -> time per image.  The 48 images (up to 960 MB with
            their masks) are more than the 256 MB Infinity Cache holds
  select    dm4d_detect_select_f32 on 6 batches of [8, 8400, 4] / [8, 8400, 1], the same way -> time per image; taken with about 40
            candidates per image (a detector's usual output) and with about 5000 (the radix select runs)
  numpy     tests/detect_model.py on the same images and rows through a pool of 16 threads, wall clock -> time per image; what the
            kernels are compared against, on the same machine
  stage     predict_keypoints end to end on the images as JPEG files with PNG masks (Pillow decodes), a stand-in pose network and a
            stand-in detector, bbox_source "fmask" against "detector", wall clock, median of --e2e_reps runs -> time per image

  python tools/detect_bench.py [--reps 11 --window 0.4]
"""
from __future__ import annotations

import argparse
import json
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
sys.path.insert(0, str(ROOT / "tests"))

from diffuman4d_amd.host import detect, ops, pose  # noqa: E402

SHAPE = (640, 640)
A = 8400
IMAGES, BATCH = 48, 8


def make_images(h: int, w: int, seed: int):
    """IMAGES images and elliptic masks: 8 of noise over a gradient, the others those rolled (fresh bytes at fresh addresses)."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    grad = ((xs * 200 // w)[..., None] + np.array([0, 20, 40])).astype(np.uint8)
    base = [grad + rng.integers(0, 56, (h, w, 3), dtype=np.uint8) for _ in range(BATCH)]
    images = [np.roll(base[k % BATCH], 37 * (k // BATCH), axis=1) for k in range(IMAGES)]
    masks = [(255 * ((((xs - w / 2) / (0.2 * w + 3 * (k % BATCH))) ** 2 + ((ys - 0.53 * h) / (0.42 * h)) ** 2) < 1)).astype(np.uint8) for k in range(IMAGES)]
    return images, masks


def dense(n: int, hot: int, seed: int):
    """[n, A, 4] boxes in canvas pixels around three centres per image and [n, A, 1] scores with about `hot` above 0.3."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(150, 490, (n, 3, 2))
    c = centres[np.arange(n)[:, None], rng.integers(0, 3, (n, A))] + rng.normal(0, 6, (n, A, 2))
    wh = rng.uniform(80, 260, (n, A, 2))
    boxes = np.concatenate([c - wh / 2, c + wh / 2], -1).astype(np.float32)
    scores = np.where(rng.random((n, A, 1)) < hot / A, 0.3 + 0.7 * rng.random((n, A, 1)), 0.3 * rng.random((n, A, 1))).astype(np.float32)
    return boxes, scores


def device_time(fn, reps: int, window: float) -> tuple:
    """Median over `reps` windows of the HIP-event time per call of `fn`, in seconds -> (time, calls per window); a window lasts about
    `window` seconds, counted from a first call that is not kept."""
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
    count = max(3, int(window / one(3)) + 1)
    return statistics.median(one(count) for _ in range(reps)), count


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=11, help="timed windows (the median is reported); at least 11")
    ap.add_argument("--window", type=float, default=0.4, help="seconds a timed window lasts, about")
    ap.add_argument("--e2e_reps", type=int, default=3)
    ap.add_argument("--log", default=str(ROOT / "profiles" / "detect_bench.log"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("detect_bench needs a HIP device: a time taken elsewhere says nothing")
    if args.reps < 11:
        raise SystemExit("--reps: at least 11")
    import detect_model as M
    from PIL import Image
    dev = torch.device("cuda", torch.cuda.current_device())
    lines = [{"what": "setup", "device": torch.cuda.get_device_name(dev), "images": IMAGES, "batch": BATCH, "canvas": list(SHAPE), "anchors": A,
              "reps": args.reps, "window_seconds": args.window}]

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

    # -- select -------------------------------------------------------------------------------------------------------------------------
    inv = torch.tensor([[1.0 / (640 / 2448), 1.0 / (535 / 2048)]] * BATCH, dtype=torch.float32, device=dev)
    for hot in (40, 5000):
        sets = [dense(BATCH, hot, 100 + hot + k) for k in range(IMAGES // BATCH)]
        on_dev = [(torch.from_numpy(b).to(dev), torch.from_numpy(s).to(dev)) for b, s in sets]
        t, count = device_time(lambda: [ops.detect_select(b, s, inv, 0, 0.3, 0.3, 100) for b, s in on_dev], args.reps, args.window)
        counts = torch.cat([ops.detect_select(b, s, inv, 0, 0.3, 0.3, 100)[0] for b, s in on_dev]).cpu().numpy()
        rows = [(sets[k // BATCH][0][k % BATCH], sets[k // BATCH][1][k % BATCH]) for k in range(IMAGES)]
        inv0 = tuple(np.float32(v) for v in inv[0].cpu().numpy())
        with ThreadPoolExecutor(max_workers=16) as pool:
            t0 = time.perf_counter()
            want = list(pool.map(lambda r: M.select(r[0], r[1], inv0), rows))
            t_np = (time.perf_counter() - t0) / IMAGES
        emit({"what": "select", "candidates_per_image_mean": float(counts[:, 2].mean()), "kept_per_image_mean": float(counts[:, 0].mean()),
              "device_seconds_per_image": t / IMAGES, "numpy_16_threads_seconds_per_image": t_np, "passes_per_window": count,
              "counts_equal_the_models": bool([w[0] for w in want] == counts.tolist())})
        del on_dev

    # -- input and the stage ------------------------------------------------------------------------------------------------------------
    def stand_in_pose(x):
        return torch.nn.functional.avg_pool2d(x[:, 1:2], 4).repeat(1, 17, 1, 1) + 3.0
    det_boxes, det_scores = (torch.from_numpy(a).to(dev) for a in dense(BATCH, 40, 7))

    def stand_in_detector(x):
        return det_boxes[: x.shape[0]], det_scores[: x.shape[0]]

    for h, w in ((2048, 2448), (1024, 1024)):
        images, masks = make_images(h, w, h)
        staged = [pose.stage_batch(images[i: i + BATCH], masks[i: i + BATCH], dev) for i in range(0, IMAGES, BATCH)]
        torch.cuda.synchronize()
        t, count = device_time(lambda: [detect.detector_inputs_staged(s, SHAPE) for s in staged], args.reps, args.window)
        # the launch alone: tables and descriptors made once
        from diffuman4d_amd.host import staging as st
        packed = []
        for s in staged:
            tabs, _, _ = detect.detector_tables(s.sizes, SHAPE)
            offs = np.concatenate([[0], np.cumsum([x.size for x in tabs])])
            desc = pose.descriptors([(k, int(offs[k])) for k in range(BATCH)], s.sizes, s.image_off, s.mask_off)
            packed.append((s.blob,) + st.pack_meta(np.concatenate(tabs), desc, dev))
        norm = torch.tensor(detect.MEAN + detect.STD, dtype=torch.float32)
        torch.cuda.synchronize()
        t_launch, count_launch = device_time(lambda: [ops.detect_input(blob, meta, meta_host, BATCH, desc_off, tab_off, tab_len, SHAPE[0], SHAPE[1],
                                                                       norm, detect.PAD_VALUE, False)
                                                      for blob, meta, meta_host, tab_off, tab_len, desc_off in packed], args.reps, args.window)
        x0 = detect.detector_inputs_staged(staged[0], SHAPE)[0][0].cpu().numpy()
        del staged, packed
        with ThreadPoolExecutor(max_workers=16) as pool:
            t0 = time.perf_counter()
            ref = list(pool.map(lambda k: M.detector_input(images[k], masks[k], SHAPE), range(IMAGES)))
            t_np = (time.perf_counter() - t0) / IMAGES
        emit({"what": "input", "image": [w, h], "device_seconds_per_image_launch_alone": t_launch / IMAGES,
              "seconds_per_image_with_tables_upload_and_synchronise": t / IMAGES, "numpy_16_threads_seconds_per_image": t_np,
              "passes_per_window": [count_launch, count],
              "bit_equal_to_the_model": bool(np.array_equal(x0.view(np.uint32), ref[0].view(np.uint32)))})
        del ref

        with tempfile.TemporaryDirectory() as tmp:
            root = Path(tmp)
            for k in range(IMAGES):
                for d, arr, ext in (("images", images[k], ".jpg"), ("fmasks", masks[k], ".png")):
                    path = root / d / f"{k // 12:02d}" / f"{k:06d}{ext}"
                    path.parent.mkdir(parents=True, exist_ok=True)
                    Image.fromarray(arr).save(path, **({"quality": 90} if ext == ".jpg" else {"compress_level": 1}))
            res = {}
            for source in ("fmask", "detector"):
                kw = dict(person_detector=stand_in_detector) if source == "detector" else {}
                wall = []
                for r in range(args.e2e_reps + 1):  # the first run is not kept
                    t0 = time.perf_counter()
                    out = pose.predict_keypoints(str(root / "images"), str(root / f"kp_{source}_{r}"), str(root / "fmasks"), pose_model=stand_in_pose,
                                                 batch_size=BATCH, gpu_ids=[dev.index], num_workers=16, bbox_source=source, **kw)
                    torch.cuda.synchronize()
                    wall.append(time.perf_counter() - t0)
                    assert out["written"] == IMAGES
                res[source] = statistics.median(wall[1:]) / IMAGES
                files = sorted((root / f"kp_{source}_1").rglob("*.json"))
                res[source + "_instances_per_image"] = sum(len(json.load(open(f))["instance_info"]) for f in files) / len(files)
            emit({"what": "stage", "image": [w, h], "seconds_per_image_fmask": res["fmask"], "seconds_per_image_detector": res["detector"],
                  "instances_per_image_fmask": res["fmask_instances_per_image"], "instances_per_image_detector": res["detector_instances_per_image"],
                  "note": "JPEG + PNG files decoded by Pillow in 16 threads; the pose stand-in runs once per instance"})
    Path(args.log).parent.mkdir(parents=True, exist_ok=True)
    with open(args.log, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
