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

With ``--skeleton-source kp2d --palette PATH`` the dataset draws the skeleton maps on the device from keypoint files (the scene gets a
``poses_2d`` file per frame either way) and the report gains
  read_kp2d        reading the task's keypoint files in the dataset's pool (wall)
  plan             plan_draw_calls of every frame, one thread (wall)
  draw_kernel      the dm4d_skeleton_draw_u8 launches (device events)
  box_mask_kernel  the dm4d_skeleton_box_mask_u8 launches, only with --no-gt-target (device events)
and decode counts the files that route still reads.  ``--no-gt-target`` builds the dataset with has_gt_target=False.  The drawing
reproduces a size only where s * 2048 / max(h, w) is an integer (a square source always): use such a --src with kp2d.

  python tools/capture_bench.py --src 2048x2048 --out 1024 --skeleton-source kp2d --palette tests/golden/skel_palette.json --no-gt-target
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
        # a 133-keypoint figure inside the mask's ellipse, deterministic: every link of a 133-keypoint palette gets drawn
        ang = np.arange(133) * 2.399963
        rad = 0.15 + 0.8 * ((np.arange(133) * 37) % 133) / 133
        kp = np.stack([cx + 0.2 * W * rad * np.cos(ang), cy + 0.4 * H * rad * np.sin(ang)], -1)
        kpath = root / "poses_2d" / f"{c:02d}" / f"{t:06d}.json"
        kpath.parent.mkdir(parents=True, exist_ok=True)
        kpath.write_text(json.dumps({"instance_info": [{"keypoints": kp.round(2).tolist(), "keypoint_scores": [1.0] * 133}]}))
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
    kp2d = ds.skeleton_source == "kp2d"
    # the files the route reads: no skeleton file with kp2d, and with has_gt_target=False only the skeleton file of a target
    target = [not ds.has_gt_target and lab[1] not in inputs for lab in labels]
    read = [[(p, m) for k, (p, m) in enumerate(zip(ps, modes)) if (k < 2 and not tg) or (k == 2 and not kp2d)] for ps, tg in zip(paths, target)]
    t0 = time.perf_counter()
    list(ds._pool.map(lambda pm: [capture._open(p, m) for p, m in pm], read))
    t_decode = time.perf_counter() - t0
    extra = {}
    if kp2d:
        from diffuman4d_amd.host import skeleton
        kpaths = [ds.get_file_path(ds.kp2d_path_pat, *lab) for lab in labels]
        t0 = time.perf_counter()
        insts = list(ds._pool.map(skeleton._read_instance, kpaths))
        extra["read_kp2d_s"] = round(time.perf_counter() - t0, 3)
        t0 = time.perf_counter()
        for lab, inst in zip(labels, insts):
            cam = ds.cameras[scene][lab[1]]
            hw = (cam["height"], cam["width"])
            skeleton.plan_draw_calls(inst, None, (ds.kp2d_canvas_shape or hw, hw), ds.palette)
        extra["plan_s"] = round(time.perf_counter() - t0, 3)
    load = ds._load_frame_kp2d if kp2d else ds._load_frame
    resize = ds._resize_on_device_kp2d if kp2d else ds._resize_on_device
    t0 = time.perf_counter()
    frames = list(ds._pool.map(lambda lab: load(lab, inputs), labels))
    t_frames = time.perf_counter() - t0
    # the device half, with the kernel bracketed by events on the dataset's stream
    ev = {}
    names = {"k": "capture_crop_resize", "draw": "skeleton_draw", "box": "skeleton_box_mask"}
    real = {key: getattr(capture.ops, name) for key, name in names.items()}

    def timed(key):
        def call(*a, **k):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out = real[key](*a, **k)
            e.record()
            ev.setdefault(key, []).append((s, e))
            return out
        return call
    for key, name in names.items():
        setattr(capture.ops, name, timed(key))
    try:
        resize(frames, dev)  # warm-up (allocations, first launch)
        ev.clear()
        t0 = time.perf_counter()
        resize(frames, dev)
        t_device = time.perf_counter() - t0
    finally:
        for key, name in names.items():
            setattr(capture.ops, name, real[key])
    seconds = lambda key: sum(s.elapsed_time(e) for s, e in ev.get(key, [])) / 1e3
    t_kernel = seconds("k")
    if kp2d:
        extra["draw_kernel_s"], extra["box_mask_kernel_s"] = round(seconds("draw"), 5), round(seconds("box"), 5)
    planes = sum(fr[n].size for fr in frames for n in ("img", "mask", "skel") if fr.get(n) is not None)
    if kp2d:  # the planes that exist on the device only are read by the kernel all the same, but never cross PCIe
        device_only = sum(fr["plan"].out_size[0] * fr["plan"].out_size[1] * (3 if fr["mask"] is not None else 4) for fr in frames)
    else:
        device_only = 0
    H, W = ds.height, ds.width
    rows = sum(fr["crop"][2] for fr in frames)  # scratch rows: about the crop height (the crop rows the vertical windows read)
    moved = planes + device_only + 2 * rows * W * 8 + len(frames) * 6 * H * W * 4
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
    return {"frames": len(labels), "skeleton_source": ds.skeleton_source, "has_gt_target": ds.has_gt_target, **extra,
            "decode_s": round(t_decode, 3), "host_prep_s": round(t_frames - t_decode, 3),
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
    ap.add_argument("--reuse-scene", action="store_true", help="with --dir: keep the scene a previous run wrote there instead of writing it again")
    ap.add_argument("--skeleton-source", default="files", choices=capture.SKELETON_SOURCES, help="the dataset's skeleton_source")
    ap.add_argument("--palette", default=None, help="palette file (skeleton.load_palette), required with --skeleton-source kp2d")
    ap.add_argument("--no-gt-target", action="store_true", help="has_gt_target=False: target cameras are skeleton-only")
    ap.add_argument("--compare-files", action="store_true",
                    help="with kp2d: also report the share of skeleton-tensor elements that differ from the file route on the scene's lossy files")
    args = ap.parse_args(argv)
    W, H = (int(v) for v in args.src.split("x"))
    tmp = tempfile.TemporaryDirectory() if args.dir is None else None
    root = Path(args.dir or tmp.name)
    scene = root / "bench"
    inputs = ["01", "13", "25", "37"]
    t0 = time.perf_counter()
    if args.reuse_scene and (scene / "transforms.json").exists():
        print(f"# scene {scene} reused", flush=True)
    else:
        write_scene(scene, W, H, 48, args.frames, temporal_cams=["03", "01"], threads=16)
        print(f"# scene {W}x{H} written in {time.perf_counter() - t0:.1f} s", flush=True)
    ds = capture.SpaTemDataset(data_dir=str(root), scene_label="bench", height=args.out, width=args.out,
                               decode_threads=args.threads, plucker=args.plucker, has_gt_target=not args.no_gt_target,
                               skeleton_source=args.skeleton_source, palette=args.palette)
    res = {"src": args.src, "out": args.out, "threads": args.threads, "plucker": args.plucker}
    if args.compare_files and args.skeleton_source == "kp2d":
        # skeletons_q85/*.webp: quality-85 encodings of the drawn maps (what draw_skeleton writes); the scene's skeletons/ stay as they are
        from diffuman4d_amd.host import skeleton
        t0 = time.perf_counter()
        skeleton.draw_skeleton(str(scene / "poses_2d"), str(scene / "skeletons_q85"), kp2d_canvas_shape=(H, W), out_kpmap_shape=(H, W),
                               palette=args.palette)
        files = capture.SpaTemDataset(data_dir=str(root), scene_label="bench", height=args.out, width=args.out, decode_threads=args.threads,
                                      plucker="cameras", skeleton_path_pat="{data_dir}/{scene_label}/skeletons_q85/{spa_label}/{tem_label}.webp")
        spa = [f"{c:02d}" for c in range(48)]
        drawn = capture.SpaTemDataset(data_dir=str(root), scene_label="bench", height=args.out, width=args.out, decode_threads=args.threads,
                                      plucker="cameras", skeleton_source="kp2d", palette=args.palette)
        a = files.get_item("bench", spa, ["000000"], inputs)["skeletons"]
        b = drawn.get_item("bench", spa, ["000000"], inputs)["skeletons"]
        res["lossy_files_vs_kp2d"] = {"elements": a.numel(), "differing_share": round(float((a != b).float().mean()), 6),
                                      "max_abs": round(float((a - b).abs().max()), 6), "seconds": round(time.perf_counter() - t0, 1)}
        print(json.dumps(res["lossy_files_vs_kp2d"]), flush=True)
    res["spatial"] = bench_task(ds, [f"{c:02d}" for c in range(48)], ["000000"], inputs, args.threads)
    print(json.dumps(res["spatial"]), flush=True)
    res["temporal"] = bench_task(ds, ["03"], [f"{t:06d}" for t in range(args.frames)], inputs, args.threads)
    print(json.dumps(res["temporal"]), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
