#!/usr/bin/env python
"""Time the device route for result JPEGs (diffuman4d_amd/host/jpeg.py) against the existing route on the same box in the same call.

Two geometries, one task = 48 saved views each:
  small   576 x 320 images, no crops (the synthetic demo's size)
  large   1024 x 1024 images restored onto a 2048 x 2448 white canvas (crop 1800 x 1800 at row 120, column 300: the reference's captured
          frames)
Per geometry, as JSON lines in --log (default profiles/jpeg_bench.log):
  device    encode_jpeg_batch of one task: HIP events around the whole call (restore + encode launches, the read of the lengths, the copy
            of the blob) after a warm-up, median of --reps; wall clock of the same calls; bytes that cross PCIe (the scans)
  baseline  the existing route: --tasks packages of the same uint8 images through imgwrite.WriterPool(--writer-processes) ->
            write_package (Pillow restore + save), wall clock per task with all processes busy; bytes over PCIe = the uint8 images
  equal     whether every file of the device route has the bytes of the baseline's file

  python tools/jpeg_bench.py [--views 48 --tasks 12 --writer-processes 12 --reps 5]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from diffuman4d_amd.host import imgwrite, jpeg  # noqa: E402

GEOMETRIES = {"small": ((576, 320), None), "large": ((1024, 1024), (120, 300, 1800, 1800, 2048, 2448))}


def make_views(n: int, h: int, w: int, dev) -> torch.Tensor:
    """uint8 [n, h, w, 3] on the device: smooth colour fields with a little noise, different per view (fixed seed)."""
    g = torch.Generator(device=dev).manual_seed(0)
    y = torch.linspace(0, 1, h, device=dev)[None, :, None, None]
    x = torch.linspace(0, 1, w, device=dev)[None, None, :, None]
    k = torch.arange(n, device=dev, dtype=torch.float32)[:, None, None, None]
    ch = torch.tensor([1.0, 1.7, 2.3], device=dev)[None, None, None, :]
    img = 0.5 + 0.35 * torch.sin(6.0 * x * ch + 0.3 * k) * torch.cos(5.0 * y * ch - 0.2 * k)
    img = img + 0.03 * torch.randn((n, h, w, 3), generator=g, device=dev)
    return (img.clamp(0, 1) * 255.0).to(torch.uint8).contiguous()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--views", type=int, default=48)
    ap.add_argument("--tasks", type=int, default=12, help="packages in flight through the writer pool")
    ap.add_argument("--writer-processes", type=int, default=12)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--geometries", nargs="*", default=list(GEOMETRIES))
    ap.add_argument("--log", default=str(ROOT / "profiles" / "jpeg_bench.log"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_bench needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda", torch.cuda.current_device())
    rows = [{"views_per_task": args.views, "tasks": args.tasks, "writer_processes": args.writer_processes, "quality": args.quality,
             "reps": args.reps, "device": torch.cuda.get_device_name(dev)}]
    for name in args.geometries:
        (h, w), crop = GEOMETRIES[name]
        views = make_views(args.views, h, w, dev)
        crops = [crop] * args.views
        images = list(views.unbind(0))
        for _ in range(2):  # warm-up: code objects, allocator
            files = jpeg.encode_jpeg_batch(images, quality=args.quality, crops=crops)
        torch.cuda.synchronize()
        ms, wall = [], []
        for _ in range(args.reps):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            s.record()
            files = jpeg.encode_jpeg_batch(images, quality=args.quality, crops=crops)
            e.record()
            e.synchronize()
            wall.append(1e3 * (time.perf_counter() - t0))
            ms.append(s.elapsed_time(e))
        head = len(jpeg.jpeg_header(1, 1, args.quality)) + 2
        scan_bytes = sum(len(f) - head for f in files)
        rows.append({"geometry": name, "measure": "device", "image": [h, w], "crop": crop, "canvas": list(jpeg.canvas_size(h, w, crop)),
                     "ms_per_task_events": round(statistics.median(ms), 3), "ms_per_task_events_range": [round(min(ms), 3), round(max(ms), 3)],
                     "ms_per_image_events": round(statistics.median(ms) / args.views, 4), "ms_per_task_wall": round(statistics.median(wall), 3),
                     "pcie_bytes_per_task": scan_bytes + 16 * args.views, "pcie_bytes_per_image": round(scan_bytes / args.views + 16),
                     "file_bytes_per_image": round(sum(len(f) for f in files) / args.views)})

        host_views = views.cpu().numpy()
        with tempfile.TemporaryDirectory() as tmp:
            def package(t):
                return {"grid": None, "crops": [], "quality": args.quality,
                        "images": [(f"{tmp}/{t}/images/{k:02d}/000000.jpg", host_views[k], crop) for k in range(args.views)]}
            with imgwrite.WriterPool(args.writer_processes) as pool:
                pool.submit(package("warm")).result()
                t0 = time.perf_counter()
                futs = [pool.submit(package(t)) for t in range(args.tasks)]
                written = sum(f.result() for f in futs)
                seconds = time.perf_counter() - t0
            equal = all(Path(f"{tmp}/0/images/{k:02d}/000000.jpg").read_bytes() == files[k] for k in range(args.views))
        rows.append({"geometry": name, "measure": "baseline", "what": "WriterPool -> write_package (Pillow restore + save), all processes busy",
                     "files_written": written, "seconds": round(seconds, 3), "ms_per_task": round(1e3 * seconds / args.tasks, 3),
                     "ms_per_image": round(1e3 * seconds / args.tasks / args.views, 4), "pcie_bytes_per_task": int(views.numel()),
                     "pcie_bytes_per_image": h * w * 3})
        rows.append({"geometry": name, "measure": "equal", "device_files_equal_baseline_files": bool(equal), "files_compared": args.views})
        del views, images, files
        torch.cuda.empty_cache()
    Path(args.log).parent.mkdir(parents=True, exist_ok=True)
    with open(args.log, "w") as f:
        for row in rows:
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
