#!/usr/bin/env python
"""Time the device JPEG decoder (diffuman4d_amd/host/jpegdec.py, csrc/jpegdec.hip) against Pillow, and the two stages that can use it.

Measurements, written as JSON lines to --log (default profiles/jpegdec_bench.log):
  decode    dm4d_jpeg_decode_u8 on scans already on the device, for --images result-sized files (576 x 320, quality 90) and --images
            files of 2448 x 2048: HIP events around one call (the fill and both launches), after a warm-up call, median of --reps ->
            time per image; the share of the entropy launch from torch's profiler (null where it cannot see the kernels); the rounds
            the speculative scheme needs are a property of the files (tests/jpegdec_model.py), not timed here.  Pillow's decode of
            the same files from memory through a pool of 16 threads on this machine, wall clock.
  bytes     bytes over PCIe per image: the raw pixels with the flag off, scan + tables + descriptor with it on
  equal     whether the device's pixels of every file equal Pillow's
  evaluate  wall time of ``evaluate_results`` over --pairs pairs (JPEG predictions, WebP ground truths, PNG masks; 576 x 320),
            ``device_decode`` off and on alternately
  stage     wall time per image of ``remove_background`` (stand-in network ``lambda x: x[:, :1]``) over --stage_images JPEG files of
            2448 x 2048, ``device_decode`` off and on alternately, 16 host threads

  python tools/jpegdec_bench.py [--images 48 --reps 7]
"""
from __future__ import annotations

import argparse
import io
import json
import shutil
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch
from PIL import Image

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from bench_common import alternate, device_time, kernel_shares, pillow_decode, pillow_times  # noqa: E402
from diffuman4d_amd.host import jpegdec, matting, metrics  # noqa: E402


def save_jpeg(a: np.ndarray, quality: int = 90) -> bytes:
    f = io.BytesIO()
    Image.fromarray(a).save(f, "JPEG", quality=quality)
    return f.getvalue()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=48)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--stage_images", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=2, help="times each route of a stage is run after its warm-up (alternating)")
    ap.add_argument("--log", default=str(ROOT / "profiles" / "jpegdec_bench.log"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("jpegdec_bench needs a HIP device: a time taken elsewhere says nothing")
    import png_cases
    dev = torch.device("cuda", torch.cuda.current_device())
    n = args.images
    lines = [{"what": "setup", "device": torch.cuda.get_device_name(dev), "images": n, "reps": args.reps, "pillow": Image.__version__,
              "host_threads": 16, "content": "smooth foreground on white (png_cases.result_like), four shifted copies, quality 90, 4:2:0"}]
    sources = {}
    for label, (h, w) in (("result_576x320", (320, 576)), ("capture_2448x2048", (2448, 2048))):
        rgb0, _ = png_cases.result_like(h, w)
        sources[label] = [np.ascontiguousarray(np.roll(rgb0, 37 * s, axis=1)) for s in range(4)]
        four = [save_jpeg(a) for a in sources[label]]
        files = [four[i % 4] for i in range(n)]
        plans = [jpegdec.probe(d) for d in files]
        offsets = [i * h * w * 3 for i in range(n)]
        out = torch.empty(n * h * w * 3, dtype=torch.uint8, device=dev)
        staged = jpegdec.stage_chunk(plans, files, offsets, [3] * n, dev)
        call = lambda: jpegdec.launch_chunk(staged, out)
        t = device_time(call, args.reps)
        shares = kernel_shares(call, r"jpegdec_\w+_kernel")
        status = call().cpu().tolist()
        got = out.view(n, h, w, 3)[:4].cpu().numpy()
        equal = status == [0] * n and all(np.array_equal(got[i], np.asarray(Image.open(io.BytesIO(four[i])))) for i in range(4))
        line = {"what": "decode", "files": label, "file_bytes_mean": sum(map(len, files)) / n, "device_seconds_per_image": t / n,
                "device_pixels_per_second": n * h * w / t, "kernel_seconds": shares,
                "entropy_share": (shares["jpegdec_entropy_kernel"] / sum(shares.values())
                                  if shares and "jpegdec_entropy_kernel" in shares else None),
                "timing": f"HIP events around one dm4d_jpeg_decode_u8 call for {n} files, warm, median of {args.reps}"}
        for threads, (seconds, _) in pillow_times(pillow_decode, files).items():
            line[f"pillow_seconds_per_image_{threads}_threads"] = seconds
        lines.append(line)
        lines.append({"what": "bytes", "files": label, "pcie_bytes_per_image_flag_off": h * w * 3, "pcie_bytes_per_image_flag_on": staged["bytes_up"] / n})
        lines.append({"what": "equal", "files": label, "device_equals_pillow": bool(equal)})
        del out, staged
        torch.cuda.empty_cache()

    tmp = Path(tempfile.mkdtemp(prefix="jpegdec_bench_"))
    try:
        # evaluate_results: JPEG predictions against WebP ground truths and PNG masks, as the sampler's runs are evaluated
        h, w = 320, 576
        _, mask = png_cases.result_like(h, w)
        rng = np.random.default_rng(0)
        for i in range(args.pairs):
            gt = sources["result_576x320"][i % 4]
            pred = np.clip(gt.astype(np.int16) + rng.integers(-6, 7, gt.shape), 0, 255).astype(np.uint8)
            key = f"{i % 8:02d}/{i // 8:06d}"
            for sub, a, ext, kw in (("pred", pred, ".jpg", dict(quality=90)), ("gt", gt, ".webp", dict(lossless=True)),
                                    ("fmasks", np.where(mask > 127, 255, 0).astype(np.uint8), ".png", {})):
                p = tmp / sub / f"{key}{ext}"
                p.parent.mkdir(parents=True, exist_ok=True)
                Image.fromarray(a).save(p, **kw)
        ev = {"what": "evaluate", "pairs": args.pairs, "image": [h, w], "batch_size": 16, "decode_threads": 8,
              "timing": "wall clock of evaluate_results; the first run of each route is a warm-up", "jpeg": "predictions only (ground truths are WebP)"}
        texts = {}

        def run_eval(flag, r):
            t0 = time.perf_counter()
            metrics.evaluate_results(str(tmp / "pred"), str(tmp / "gt"), str(tmp / "fmasks"), ".jpg", ".webp", ".png",
                                     out_metrics_path=str(tmp / f"m{int(flag)}.json"), background_color="white", gpu_ids=[dev.index],
                                     device_decode=flag)
            dt = time.perf_counter() - t0
            texts[flag] = (tmp / f"m{int(flag)}.json").read_text()
            return dt
        times = alternate(run_eval, args.rounds)
        ev["flag_off_seconds"], ev["flag_on_seconds"] = times[False], times[True]
        ev["flag_off_seconds_median"], ev["flag_on_seconds_median"] = statistics.median(times[False]), statistics.median(times[True])
        ev["same_metrics_json"] = texts[False] == texts[True]
        lines.append(ev)

        # remove_background: files on disk -> files on disk, with the stand-in network
        for i in range(args.stage_images):
            p = tmp / "images" / f"{i % 4:02d}" / f"{i // 4:06d}.jpg"
            p.parent.mkdir(parents=True, exist_ok=True)
            Image.fromarray(sources["capture_2448x2048"][i % 4]).save(p, quality=90)
        stage = {"what": "stage", "images": args.stage_images, "image": [2448, 2048], "batch_size": 8, "num_workers": 16,
                 "network_stand_in": "lambda x: x[:, :1]", "device_png": True,
                 "timing": "wall clock of remove_background (decode, upload, kernels, PNG files written), per image; the first run of each route is a warm-up"}
        def run_stage(flag, r):
            out = tmp / f"out_{r}_{int(flag)}"
            t0 = time.perf_counter()
            res = matting.remove_background(str(tmp / "images"), str(out / "fmasks"), str(out / "images_alpha"), image_ext=".jpg", batch_size=8,
                                            num_workers=16, gpu_ids=[dev.index], matting_model=lambda x: x[:, :1], device_png=True,
                                            device_decode=flag)
            dt = time.perf_counter() - t0
            assert res["written"] == args.stage_images
            shutil.rmtree(out)
            return dt / args.stage_images
        times = alternate(run_stage, args.rounds)
        stage["flag_off_seconds_per_image"], stage["flag_on_seconds_per_image"] = times[False], times[True]
        stage["flag_off_seconds_per_image_median"] = statistics.median(times[False])
        stage["flag_on_seconds_per_image_median"] = statistics.median(times[True])
        lines.append(stage)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    Path(args.log).parent.mkdir(parents=True, exist_ok=True)
    with open(args.log, "w") as f:
        for line in lines:
            print(json.dumps(line))
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
