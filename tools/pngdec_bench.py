#!/usr/bin/env python
"""Time the device PNG decoder (diffuman4d_amd/host/pngdec.py, csrc/pngdec.hip) against Pillow, and the two stages that can use it.

Measurements, written as JSON lines to --log (default profiles/pngdec_bench.log):
  decode    dm4d_png_decode_u8 on streams already on the device, for --images soft-edged masks of 1024 x 1024 and of 2448 x 2048 (mode
            L, as the matting stage writes them) and --images RGB files of 576 x 320: HIP events around one call (both launches), after
            a warm-up call, median of --reps -> time per image; the share of each launch from torch's profiler (null where it cannot see
            the kernels).  Pillow's decode of the same bytes from memory on this machine, on one thread and through a pool of 16.
  bytes     bytes over PCIe per image: the raw pixels with the flag off, zlib stream + descriptor with it on
  equal     whether the device's pixels of every file equal Pillow's
  carve     wall time per frame of ``carve_scene`` (48 views of 1024 x 1024 masks, --frames frames), ``device_decode`` off and on
            alternately
  evaluate  wall time of ``evaluate_results`` over --pairs pairs (PNG predictions, ground truths and masks; 576 x 320),
            ``device_decode`` off and on alternately

  python tools/pngdec_bench.py [--images 48 --reps 7]
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
from PIL import Image, ImageFilter

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from bench_common import alternate, device_time, kernel_shares, pillow_decode, pillow_times  # noqa: E402
from diffuman4d_amd.host import metrics, pngdec, vhull  # noqa: E402


def save_png(a: np.ndarray) -> bytes:
    f = io.BytesIO()
    Image.fromarray(a).save(f, "PNG")
    return f.getvalue()


def soft_mask(h: int, w: int, shift: int = 0) -> np.ndarray:
    """a soft-edged ellipse, as the matting stage's masks are: 0 outside, 255 inside, a blurred rim"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    inside = ((x - w / 2 - shift) / (0.30 * w)) ** 2 + ((y - h / 2) / (0.40 * h)) ** 2 <= 1.0
    return np.asarray(Image.fromarray((inside * 255).astype(np.uint8)).filter(ImageFilter.GaussianBlur(3)))


def camera(angle: float, dist: float) -> list:
    pos = np.array([dist * np.cos(angle), dist * np.sin(angle), 0.3])
    z = pos / np.linalg.norm(pos)
    x = np.cross([0.0, 0.0, 1.0], z)
    x /= np.linalg.norm(x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, np.cross(z, x), z, pos
    return m.tolist()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=48)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2, help="times each route of a stage is run after its warm-up (alternating)")
    ap.add_argument("--log", default=str(ROOT / "profiles" / "pngdec_bench.log"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("pngdec_bench needs a HIP device: a time taken elsewhere says nothing")
    import png_cases
    dev = torch.device("cuda", torch.cuda.current_device())
    n = args.images
    lines = [{"what": "setup", "device": torch.cuda.get_device_name(dev), "images": n, "reps": args.reps, "pillow": Image.__version__,
              "host_threads": 16, "content": "soft-edged ellipse masks (mode L) and a smooth foreground on white (png_cases.result_like), "
                                             "four shifted copies each, Pillow's default compression"}]
    rgb0, _ = png_cases.result_like(320, 576)
    sources = {"mask_1024x1024": [soft_mask(1024, 1024, 9 * s) for s in range(4)],
               "mask_2448x2048": [soft_mask(2448, 2048, 9 * s) for s in range(4)],
               "rgb_576x320": [np.ascontiguousarray(np.roll(rgb0, 37 * s, axis=1)) for s in range(4)]}
    encoded = {}
    for label, arrays in sources.items():
        h, w = arrays[0].shape[:2]
        ch = 1 if arrays[0].ndim == 2 else 3
        four = encoded[label] = [save_png(a) for a in arrays]
        files = [four[i % 4] for i in range(n)]
        plans = [pngdec.probe(d) for d in files]
        offsets = [i * h * w * ch for i in range(n)]
        out = torch.empty(n * h * w * ch, dtype=torch.uint8, device=dev)
        staged = pngdec.stage_chunk(plans, files, offsets, [ch] * n, dev)
        call = lambda: pngdec.launch_chunk(staged, out)
        t = device_time(call, args.reps)
        shares = kernel_shares(call, r"pngdec_\w+_kernel")
        status = call().cpu().tolist()
        got = out.view((n, h, w) if ch == 1 else (n, h, w, ch))[:4].cpu().numpy()
        equal = status == [0] * n and all(np.array_equal(got[i], np.asarray(Image.open(io.BytesIO(four[i])))) for i in range(4))
        line = {"what": "decode", "files": label, "file_bytes_mean": sum(map(len, files)) / n, "device_seconds_per_image": t / n,
                "device_seconds_per_call": t, "device_pixels_per_second": n * h * w / t, "kernel_seconds": shares,
                "inflate_share": shares["pngdec_inflate_kernel"] / sum(shares.values()) if shares and "pngdec_inflate_kernel" in shares else None,
                "unfilter_share": shares["pngdec_unfilter_kernel"] / sum(shares.values()) if shares and "pngdec_unfilter_kernel" in shares else None,
                "timing": f"HIP events around one dm4d_png_decode_u8 call for {n} files, warm, median of {args.reps}"}
        for threads, (seconds, _) in pillow_times(pillow_decode, files).items():
            line[f"pillow_seconds_per_image_{threads}_threads"] = seconds
        lines.append(line)
        lines.append({"what": "bytes", "files": label, "pcie_bytes_per_image_flag_off": h * w * ch, "pcie_bytes_per_image_flag_on": staged["bytes_up"] / n})
        lines.append({"what": "equal", "files": label, "device_equals_pillow": bool(equal)})
        del out, staged
        torch.cuda.empty_cache()

    tmp = Path(tempfile.mkdtemp(prefix="pngdec_bench_"))
    try:
        # carve_scene: 48 views on a circle around the ellipse, the masks of the decode measurement
        views, side, focal, dist = 48, 1024, 1000.0, 3.0
        frames = [{"camera_label": f"{c:02d}", "fl_x": focal, "fl_y": focal, "cx": side / 2, "cy": side / 2, "w": side, "h": side,
                   "transform_matrix": camera(2 * np.pi * c / views, dist)} for c in range(views)]
        (tmp / "transforms.json").write_text(json.dumps({"frames": frames}))
        for c in range(views):
            for f in range(args.frames):
                p = tmp / "fmasks" / f"{c:02d}" / f"{f:06d}.png"
                p.parent.mkdir(parents=True, exist_ok=True)
                p.write_bytes(encoded["mask_1024x1024"][0])
        carve = {"what": "carve", "views": views, "mask": [side, side], "frames": args.frames, "voxel_size": 0.025, "bounds": 1.5, "host_threads": 16,
                 "timing": "wall clock of carve_scene (files read, decoded, carved, PLY files written), per frame; the first run of each route is a warm-up"}
        trees = {}

        def run_carve(flag, r):
            out = tmp / f"surfs_{int(flag)}"
            shutil.rmtree(out, ignore_errors=True)
            t0 = time.perf_counter()
            vhull.carve_scene(str(tmp / "fmasks"), str(tmp / "transforms.json"), str(out), bounds=(-1.5, 1.5) * 3, voxel_size=0.025, device=dev,
                              host_threads=16, **({"device_decode": True} if flag else {}))
            dt = (time.perf_counter() - t0) / args.frames
            trees[flag] = {p.name: p.read_bytes() for p in sorted(out.glob("*.ply"))}
            return dt
        times = alternate(run_carve, args.rounds)
        carve["flag_off_seconds_per_frame"], carve["flag_on_seconds_per_frame"] = times[False], times[True]
        carve["flag_off_seconds_per_frame_median"] = statistics.median(times[False])
        carve["flag_on_seconds_per_frame_median"] = statistics.median(times[True])
        carve["same_ply_files"] = trees[False] == trees[True]
        lines.append(carve)

        # evaluate_results: PNG predictions, ground truths and masks
        h, w = 320, 576
        _, mask = png_cases.result_like(h, w)
        rng = np.random.default_rng(0)
        for i in range(args.pairs):
            gt = sources["rgb_576x320"][i % 4]
            pred = np.clip(gt.astype(np.int16) + rng.integers(-6, 7, gt.shape), 0, 255).astype(np.uint8)
            key = f"{i % 8:02d}/{i // 8:06d}"
            for sub, a in (("pred", pred), ("gt", gt), ("fmasks", np.where(mask > 127, 255, 0).astype(np.uint8))):
                p = tmp / sub / f"{key}.png"
                p.parent.mkdir(parents=True, exist_ok=True)
                Image.fromarray(a).save(p)
        ev = {"what": "evaluate", "pairs": args.pairs, "image": [h, w], "batch_size": 16, "decode_threads": 8,
              "timing": "wall clock of evaluate_results; the first run of each route is a warm-up", "png": "predictions, ground truths and masks"}
        texts = {}

        def run_eval(flag, r):
            t0 = time.perf_counter()
            metrics.evaluate_results(str(tmp / "pred"), str(tmp / "gt"), str(tmp / "fmasks"), ".png", ".png", ".png",
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
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    Path(args.log).parent.mkdir(parents=True, exist_ok=True)
    with open(args.log, "w") as f:
        for line in lines:
            print(json.dumps(line))
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
