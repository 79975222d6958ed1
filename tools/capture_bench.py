#!/usr/bin/env python
"""Where the time of a captured-scene ``get_item`` goes (diffuman4d_amd/host/capture.py), against the reference's host resize.

Writes a seeded on-disk scene (48 cameras; one spatial task of 48 frames and one temporal task of 2 x 150 frames; WebP images and
skeletons, PNG masks) at the source size of ``--src WxH``, then for each task reports:
  decode     Pillow decode of the task's 3 files per frame in the dataset's thread pool (wall)
  host prep  the rest of the per-frame host work: crop box, checks (wall of the full per-frame step minus decode)
  pack       table build + copy of the planes into the pinned staging buffer (wall of the device half minus H2D and kernel)
  H2D        one pinned copy of the staging buffer (device events)
  kernel     the two launches of dm4d_capture_crop_resize_f32 (device events), and the bytes they move per second against
             the ~6.3 TB/s HBM bandwidth achievable on MI355X: source planes read + scratch written and read + fp32 outputs written
  get_item   the whole call, wall
  pillow     Pillow crop + resize (BICUBIC) of the same 3 planes per frame on the host, same thread count (the reference's path)

  python tools/capture_bench.py --src 2448x2048 --out 1024 --threads 8 [--plucker cameras]
"""
from __future__ import annotations

import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from diffuman4d_amd.host import capture  # noqa: E402

HBM_TBPS = 6.3


def write_scene(root: Path, W: int, H: int, n_cams: int, n_frames: int, temporal_cams, threads: int) -> None:
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    import math
    root.mkdir(parents=True, exist_ok=True)
    frames = []
    for c in range(n_cams):
        a = 2 * math.pi * c / n_cams
        o = np.array([3.0 * math.cos(a), 0.0, 3.0 * math.sin(a)])
        back = o / np.linalg.norm(o)
        right = np.cross([0.0, 1.0, 0.0], back)
        right /= np.linalg.norm(right)
        m = np.eye(4)
        m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = right, np.cross(back, right), back, o
        frames.append({"camera_label": f"{c:02d}", "h": H, "w": W, "transform_matrix": m.tolist()})
    (root / "transforms.json").write_text(json.dumps({"fl_x": 1.2 * W, "fl_y": 1.2 * W, "cx": W / 2, "cy": H / 2,
                                                      "w": W, "h": H, "frames": frames}))
    yy, xx = np.mgrid[:H, :W]

    def one(job):
        c, t = job
        rng = np.random.default_rng(1000 * c + t)
        cx, cy = W / 2 + 0.1 * W * math.sin(c + t / 10), H / 2 + 0.05 * H * math.cos(c)
        inside = ((xx - cx) / (0.22 * W)) ** 2 + ((yy - cy) / (0.42 * H)) ** 2 < 1
        mask = np.where(inside, 255, 0).astype(np.uint8)
        img = np.stack([(xx // 3 + 20 * c) % 256, (yy // 3 + t) % 256, ((xx + yy) // 5) % 256], -1).astype(np.uint8)
        img = np.clip(img.astype(np.int16) + rng.integers(-8, 9, img.shape), 0, 255).astype(np.uint8)
        skel = np.zeros_like(img)
        skel[int(cy) - H // 4: int(cy) + H // 4, int(cx) - 4: int(cx) + 4] = (200, 80, 40 + c)
        for sub, arr, ext in (("images", img, "webp"), ("skeletons", skel, "webp"), ("fmasks", mask, "png")):
            p = root / sub / f"{c:02d}" / f"{t:06d}.{ext}"
            p.parent.mkdir(parents=True, exist_ok=True)
            Image.fromarray(arr).save(p, quality=90) if ext == "webp" else Image.fromarray(arr).save(p)

    jobs = [(c, 0) for c in range(n_cams)] + [(int(c), t) for c in temporal_cams for t in range(1, n_frames)]
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(one, jobs))


def bench_task(ds, spa, tem, inputs, threads: int) -> dict:
    from PIL import Image
    scene = ds.scene_label
    dev = torch.device("cuda", torch.cuda.current_device())
    if len(tem) == 1:
        labels = [(scene, s, tem[0]) for s in spa]
    else:
        near = ds._nearest(ds.cameras[scene], spa[0], inputs)
        labels = [(scene, s, t) for s in [near] + spa for t in tem]
    paths = [[ds.get_file_path(p, *lab) for p in (ds.image_path_pat, ds.fmask_path_pat, ds.skeleton_path_pat)] for lab in labels]
    modes = ("RGB", "L", "RGB")
    t0 = time.perf_counter()
    list(ds._pool.map(lambda ps: [capture._open(p, m) for p, m in zip(ps, modes)], paths))
    t_decode = time.perf_counter() - t0
    t0 = time.perf_counter()
    frames = list(ds._pool.map(lambda lab: ds._load_frame(lab, inputs), labels))
    t_frames = time.perf_counter() - t0
    # the device half, with the kernel bracketed by events on the dataset's stream
    ev = {}
    real = capture.ops.capture_crop_resize

    def timed(*a, **k):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = real(*a, **k)
        e.record()
        ev["k"] = (s, e)
        return out
    capture.ops.capture_crop_resize = timed
    try:
        ds._resize_on_device(frames, dev)  # warm-up (allocations, first launch)
        t0 = time.perf_counter()
        ds._resize_on_device(frames, dev)
        t_device = time.perf_counter() - t0
    finally:
        capture.ops.capture_crop_resize = real
    t_kernel = ev["k"][0].elapsed_time(ev["k"][1]) / 1e3
    planes = sum(fr[n].size for fr in frames for n in ("img", "mask", "skel") if fr[n] is not None)
    H, W = ds.height, ds.width
    rows = sum(fr["crop"][2] for fr in frames)  # scratch rows: about the crop height (the crop rows the vertical windows read)
    moved = planes + 2 * rows * W * 8 + len(frames) * 6 * H * W * 4
    # H2D of a pinned buffer of the staging size
    blob = torch.empty(planes, dtype=torch.uint8, pin_memory=True)
    dst = torch.empty(planes, dtype=torch.uint8, device=dev)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    dst.copy_(blob, non_blocking=True)
    e.record()
    e.synchronize()
    t_h2d = s.elapsed_time(e) / 1e3
    del blob, dst, frames
    t0 = time.perf_counter()
    ds.get_item(scene, spa, tem, inputs)
    t_get = time.perf_counter() - t0

    def pil(ps):  # decode + crop box + crop + resize, as the reference does per frame
        ims = [Image.open(p) for p in ps]
        m = np.asarray(ims[1])
        top, left, ch, cw = capture.crop_box(m)[:4]
        for im in ims:
            im.crop((left, top, left + cw, top + ch)).resize((W, H), Image.BICUBIC)
    t0 = time.perf_counter()
    list(ds._pool.map(pil, paths))
    t_pil = time.perf_counter() - t0
    return {"frames": len(labels), "decode_s": round(t_decode, 3), "host_prep_s": round(t_frames - t_decode, 3),
            "pack_s": round(t_device - t_kernel - t_h2d, 3), "h2d_s": round(t_h2d, 4), "h2d_gb_per_s": round(planes / t_h2d / 1e9, 1),
            "kernel_s": round(t_kernel, 4), "kernel_tb_per_s": round(moved / t_kernel / 1e12, 2),
            "kernel_frac_of_hbm": round(moved / t_kernel / 1e12 / HBM_TBPS, 3), "get_item_s": round(t_get, 3),
            "kernel_frac_of_get_item": round(t_kernel / t_get, 4), "pillow_decode_crop_resize_s": round(t_pil, 3)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--src", default="2448x2048", help="source W x H")
    ap.add_argument("--out", type=int, default=1024)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--dir", default=None, help="scene directory (default: a temporary one)")
    ap.add_argument("--plucker", default="host", choices=("host", "cameras"), help="the dataset's plucker mode")
    args = ap.parse_args(argv)
    W, H = (int(v) for v in args.src.split("x"))
    tmp = tempfile.TemporaryDirectory() if args.dir is None else None
    root = Path(args.dir or tmp.name)
    scene = root / "bench"
    inputs = ["01", "13", "25", "37"]
    t0 = time.perf_counter()
    write_scene(scene, W, H, 48, args.frames, temporal_cams=["03", "01"], threads=16)
    print(f"# scene {W}x{H} written in {time.perf_counter() - t0:.1f} s", flush=True)
    ds = capture.SpaTemDataset(data_dir=str(root), scene_label="bench", height=args.out, width=args.out,
                               decode_threads=args.threads, plucker=args.plucker)
    res = {"src": args.src, "out": args.out, "threads": args.threads, "plucker": args.plucker}
    res["spatial"] = bench_task(ds, [f"{c:02d}" for c in range(48)], ["000000"], inputs, args.threads)
    print(json.dumps(res["spatial"]), flush=True)
    res["temporal"] = bench_task(ds, ["03"], [f"{t:06d}" for t in range(args.frames)], inputs, args.threads)
    print(json.dumps(res["temporal"]), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
