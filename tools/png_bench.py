#!/usr/bin/env python
"""Time the device PNG encoder (diffuman4d_amd/host/png.py, csrc/png.hip) against Pillow at the export's sizes: --images result-like
images of --height x --width (2448 x 2048), each giving one mask file (L) and one RGBA file.

Measurements, written as JSON lines to --log (default profiles/png_bench.log):
  encode    dm4d_png_encode_u8 on planes already on the device (the five launches, workspace and blob from the warm caching allocator):
            HIP events around one call for all mask files, one for all RGBA files, after a warm-up call, median of --reps -> time per
            file; and Pillow's ``save`` of the same files into memory through a pool of 16 threads on this machine, wall clock
  sizes     bytes of the files of both routes, and bytes over PCIe per image: the files on the device route, the raw mask plane on the
            Pillow route (which composes the RGBA image on the host)
  stage     ``remove_background`` (with ``out_images_alpha_dir``) over --stage_images JPEG files on disk with the stand-in network
            ``lambda x: x[:, :1]``, ``device_png`` off and on alternately, wall clock per image, 16 host threads
  equal     whether the device's files of the first image decode (Pillow) to exactly the input

  python tools/png_bench.py [--images 48 --reps 7]
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

from bench_common import alternate, device_time, pillow_times  # noqa: E402
from diffuman4d_amd.host import lib as L  # noqa: E402
from diffuman4d_amd.host import matting, ops, png  # noqa: E402


def descriptors(items):
    """host int64 descriptors, total bound and workspace bytes of `items` (png.png_encode_planes' format)."""
    lib = L.load()
    desc = torch.zeros((len(items), L.PNG_FIELDS), dtype=torch.int64)
    filt0 = stripe0 = bound = 0
    for k, it in enumerate(items):
        kind, h, w = it[:3]
        ch = 4 if kind == png.RGBA else 1
        desc[k, :len(it)] = torch.tensor(it)
        desc[k, 7], desc[k, 8] = filt0, stripe0
        filt0, stripe0, bound = filt0 + h * (1 + w * ch), stripe0 + png.n_stripes(h, w, ch), bound + int(lib.dm4d_png_bound(h, w, ch))
    return desc, bound, int(lib.dm4d_png_ws_bytes(filt0, stripe0, len(items)))


def pillow_bytes(img: Image.Image) -> int:
    buf = io.BytesIO()
    img.save(buf, format="PNG")
    return buf.tell()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=48)
    ap.add_argument("--height", type=int, default=2448)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--stage_images", type=int, default=32)
    ap.add_argument("--stage_rounds", type=int, default=2, help="times each route of the stage is run (alternating)")
    ap.add_argument("--log", default=str(ROOT / "profiles" / "png_bench.log"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("png_bench needs a HIP device: a time taken elsewhere says nothing")
    import png_cases
    dev = torch.device("cuda", torch.cuda.current_device())
    h, w, n = args.height, args.width, args.images
    lines = [{"what": "setup", "device": torch.cuda.get_device_name(dev), "images": n, "image": [h, w], "reps": args.reps,
              "pillow": Image.__version__, "host_threads": 16, "content": "smooth foreground through a JPEG round trip on white, blurred elliptical mask"}]

    # four distinct pairs (shifted copies), every image of the batch at an address of its own
    rgb0, mask0 = png_cases.result_like(h, w)
    pairs = [(np.ascontiguousarray(np.roll(rgb0, 37 * s, axis=1)), np.ascontiguousarray(np.roll(mask0, 37 * s, axis=1))) for s in range(4)]
    rgb = torch.from_numpy(np.stack([pairs[i % 4][0] for i in range(n)])).to(dev)
    masks = torch.from_numpy(np.stack([pairs[i % 4][1] for i in range(n)])).to(dev)
    l_items = [(png.L, h, w, i * h * w, w) for i in range(n)]
    a_items = [(png.RGBA, h, w, i * h * w * 3, 3 * w, i * h * w, w) for i in range(n)]
    plans = {"mask": descriptors(l_items), "rgba": descriptors(a_items)}
    enc = {"what": "encode", "timing": f"HIP events around one dm4d_png_encode_u8 call for {n} files, warm, median of {args.reps}"}
    sizes = {"what": "sizes", "raw_mask_bytes": h * w, "raw_rgba_bytes": h * w * 4}
    files = {}
    for kind, (desc, bound, ws) in plans.items():
        call = lambda: ops.png_encode(masks.view(-1), rgb.view(-1) if kind == "rgba" else None, desc, bound, ws)
        t = device_time(call, args.reps)
        blob, out = call()
        where = out.cpu().tolist()
        enc[f"device_{kind}_seconds_per_file"] = t / n
        enc[f"device_{kind}_raw_bytes_per_second"] = n * h * w * (4 if kind == "rgba" else 1) / t
        sizes[f"device_{kind}_file_bytes_mean"] = sum(where[n:]) / n
        files[kind] = bytes(blob[where[0]: where[0] + where[n]].cpu().numpy())
    enc["device_pair_seconds_per_image"] = enc["device_mask_seconds_per_file"] + enc["device_rgba_seconds_per_file"]

    # Pillow through 16 threads: the same files, into memory
    pil_masks = [Image.fromarray(pairs[i % 4][1]) for i in range(n)]
    pil_rgba = [Image.fromarray(np.dstack(pairs[i % 4])) for i in range(n)]
    for kind, ims in (("mask", pil_masks), ("rgba", pil_rgba)):
        for threads, (seconds, got) in pillow_times(pillow_bytes, ims).items():
            enc[f"pillow_{kind}_seconds_per_file_{threads}_threads"] = seconds
        sizes[f"pillow_{kind}_file_bytes_mean"] = sum(got) / len(got)
    enc["pillow_pair_seconds_per_image_16_threads"] = enc["pillow_mask_seconds_per_file_16_threads"] + enc["pillow_rgba_seconds_per_file_16_threads"]
    sizes["device_route_bytes_down_per_image"] = sizes["device_mask_file_bytes_mean"] + sizes["device_rgba_file_bytes_mean"]
    sizes["pillow_route_bytes_down_per_image"] = h * w
    lines += [enc, sizes]
    m, a = Image.open(io.BytesIO(files["mask"])), Image.open(io.BytesIO(files["rgba"]))
    lines.append({"what": "equal", "mask_decodes_to_input": bool(m.mode == "L" and np.array_equal(np.asarray(m), pairs[0][1])),
                  "rgba_decodes_to_input": bool(a.mode == "RGBA" and np.array_equal(np.asarray(a), np.dstack(pairs[0])))})
    del rgb, masks, blob
    torch.cuda.empty_cache()

    # the stage: files on disk -> files on disk, with the stand-in network
    tmp = Path(tempfile.mkdtemp(prefix="png_bench_"))
    try:
        for i in range(args.stage_images):
            p = tmp / "images" / f"{i % 4:02d}" / f"{i // 4:06d}.jpg"
            p.parent.mkdir(parents=True, exist_ok=True)
            Image.fromarray(pairs[i % 4][0]).save(p, quality=90)
        stage = {"what": "stage", "images": args.stage_images, "batch_size": 8, "num_workers": 16, "network_stand_in": "lambda x: x[:, :1]",
                 "timing": "wall clock of remove_background (decode, upload, kernels, PNG files written), per image; the first run of each route is a warm-up"}
        def run_stage(device_png, r):
            out = tmp / f"out_{r}_{int(device_png)}"
            t0 = time.perf_counter()
            res = matting.remove_background(str(tmp / "images"), str(out / "fmasks"), str(out / "images_alpha"), image_ext=".jpg", batch_size=8,
                                            num_workers=16, gpu_ids=[dev.index], matting_model=lambda x: x[:, :1], device_png=device_png)
            dt = time.perf_counter() - t0
            assert res["written"] == args.stage_images
            shutil.rmtree(out)
            return dt / args.stage_images
        times = alternate(run_stage, args.stage_rounds)
        stage["pillow_route_seconds_per_image"] = times[False]
        stage["device_png_route_seconds_per_image"] = times[True]
        stage["pillow_route_seconds_per_image_median"] = statistics.median(times[False])
        stage["device_png_route_seconds_per_image_median"] = statistics.median(times[True])
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
