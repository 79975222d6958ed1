#!/usr/bin/env python
"""Time the device lossless-WebP encoder (diffuman4d_amd/host/webp.py, csrc/webp.hip) against Pillow on skeleton maps: 48 maps of
1024 x 1024 drawn on the device from a synthetic pose set (tools/skel_kp3d_bench.py's figure, one map per camera of its ring).

Measurements, written as JSON lines to --log (default profiles/webp_bench.log):
  encode    dm4d_webp_encode_u8 on maps already on the device (the five launches, workspace and blob from the warm caching allocator): HIP
            events around one call for all maps after a warm-up call, median of --reps -> time per map; the device seconds of each of
            the five launches from the profiler (one call, a run of its own); and Pillow's ``save(quality=85)`` and
            ``save(lossless=True)`` of the same maps into memory on one thread and through a pool of 16, wall clock
  sizes     bytes of the files of all three kinds, and bytes over PCIe per map: the files on the device route, the raw map on the
            Pillow route
  decode    Pillow's time to decode each kind of file to pixels (the dataset's file route reads them), one thread and 16
  equal     whether every device file decodes (Pillow) to exactly its map
  stage     ``draw_skeleton`` end to end over 48 x --scene-frames maps (tools/skel_kp3d_bench.py's scene), ``device_webp`` off and on
            alternately, from the poses_2d directory and from poses_3d; wall clock, medians of --rounds after a warm-up run of each

  python tools/webp_bench.py --palette tests/golden/skel_palette.json [--scene-frames 150 --rounds 5 --reps 5]
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
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch
from PIL import Image

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from bench_common import alternate, device_time, kernel_shares, pillow_decode, pillow_times  # noqa: E402
from capture_bench import write_scene  # noqa: E402
from diffuman4d_amd.host import lib as L  # noqa: E402
from diffuman4d_amd.host import ops, skeleton, triang, webp  # noqa: E402
from skel_kp3d_bench import CAMS, SIZE, figure, spread  # noqa: E402


def descriptors(n: int, h: int, w: int):
    """host int64 descriptors, total bound and workspace bytes of n tight h x w images back to back."""
    lib = L.load()
    desc = torch.zeros((n, L.WEBP_FIELDS), dtype=torch.int64)
    s = webp.n_stripes(h, w)
    for k in range(n):
        desc[k, :6] = torch.tensor([h, w, k * h * w * 3, 3 * w, k * h * w, k * s])
    return desc, n * int(lib.dm4d_webp_bound(h, w)), int(lib.dm4d_webp_ws_bytes(n * h * w, n * s, n))


def pillow_save(kw):
    def save(arr) -> bytes:
        buf = io.BytesIO()
        Image.fromarray(arr).save(buf, format="WEBP", **kw)
        return buf.getvalue()
    return save


def bench_encode(maps: torch.Tensor, reps: int):
    n, h, w, _ = maps.shape
    desc, bound, ws = descriptors(n, h, w)
    call = lambda: ops.webp_encode(maps.view(-1), desc, bound, ws)  # noqa: E731
    t = device_time(call, reps)
    blob, out = call()
    where = out.cpu().tolist()
    files = {"device": [bytes(blob[where[k]: where[k] + where[n + k]].cpu().numpy()) for k in range(n)]}
    enc = {"what": "encode", "maps": n, "map": [h, w],
           "timing": f"HIP events around one dm4d_webp_encode_u8 call for {n} maps, warm, median of {reps}; launches: profiler, one call",
           "device_seconds_per_map": t / n, "device_raw_bytes_per_second": n * h * w * 3 / t}
    shares = kernel_shares(call, r"webp_(tokens|image|offsets|emit|seam)_kernel")
    enc["device_launch_seconds_per_call"] = shares
    host = maps.cpu().numpy()
    arrays = [host[k] for k in range(n)]
    for kind, kw in (("q85", {"quality": 85}), ("lossless", {"lossless": True})):
        for threads, (seconds, got) in pillow_times(pillow_save(kw), arrays).items():
            enc[f"pillow_{kind}_seconds_per_map_{threads}_threads"] = seconds
        files[kind] = got
    sizes = {"what": "sizes", "raw_map_bytes": h * w * 3}
    dec = {"what": "decode", "timing": "Pillow: Image.open + np.asarray of the file's bytes in memory, wall clock per file"}
    for kind, fs in files.items():
        sizes[f"{kind}_file_bytes_mean"] = sum(len(f) for f in fs) / len(fs)
        sizes[f"{kind}_file_bytes_min_max"] = [min(len(f) for f in fs), max(len(f) for f in fs)]
        for threads, (seconds, _) in pillow_times(pillow_decode, fs).items():
            dec[f"{kind}_seconds_per_file_{threads}_threads"] = seconds
    sizes["device_over_q85"] = sizes["device_file_bytes_mean"] / sizes["q85_file_bytes_mean"]
    sizes["device_over_pillow_lossless"] = sizes["device_file_bytes_mean"] / sizes["lossless_file_bytes_mean"]
    sizes["device_route_bytes_down_per_map"] = sizes["device_file_bytes_mean"]
    sizes["pillow_route_bytes_down_per_map"] = h * w * 3
    equal = all(np.array_equal(np.asarray(Image.open(io.BytesIO(f))), a) for f, a in zip(files["device"], arrays))
    return [enc, sizes, dec, {"what": "equal", "device_files_decode_to_their_maps": bool(equal)}]


def bench_stage(scene: Path, tmp: Path, palette, n_frames: int, threads: int, rounds: int, pool, dev, emit) -> None:
    """Detections for every camera and frame (the figure's projection, score 0.9), triangulated once with poses_2d written; then
    draw_skeleton from poses_2d and from poses_3d, device_webp off and on alternately."""
    Ks, Ts = triang.scene_cameras(str(scene / "transforms.json"), CAMS)
    uv, _, _ = triang.project_points(np.stack([figure(t) for t in range(n_frames)]), Ks, Ts, device=dev)
    sap = tmp / "poses_sapiens"
    list(pool.map(lambda j: triang.write_kp2d(sap / CAMS[j[1]] / f"{j[0]:06d}.json", uv[j[0], j[1]], None, np.full(133, 0.9)),
                  [(t, c) for t in range(n_frames) for c in range(48)]))
    triang.triangulate_skeleton(str(scene / "transforms.json"), str(sap), str(tmp / "poses_3d"), num_workers=threads, device=dev,
                                out_kp2d_proj_dir=str(tmp / "poses_2d"))
    for route in ("poses_2d", "poses_3d"):
        last = {}

        def run(flag, r):
            out = tmp / f"skeletons_{route}_{int(flag)}"
            kw = dict(palette=palette, num_workers=threads, device=dev, device_webp=flag)
            t0 = time.perf_counter()
            if route == "poses_2d":
                res = skeleton.draw_skeleton(str(tmp / "poses_2d"), str(out), **kw)
            else:
                res = skeleton.draw_skeleton(None, str(out), kp3d_dir=str(tmp / "poses_3d"), camera_path=str(scene / "transforms.json"), **kw)
            dt = time.perf_counter() - t0
            assert res["files"] == 48 * n_frames
            last[flag] = {"seconds": res["seconds"], "bytes_written": sum(p.stat().st_size for p in out.rglob("*.webp"))}
            shutil.rmtree(out)
            return dt
        times = alternate(run, rounds)
        emit({"what": "stage", "route": route, "cameras": 48, "frames": n_frames, "maps": 48 * n_frames, "out": [SIZE, SIZE], "num_workers": threads,
              "rounds": rounds, "timing": "wall clock of draw_skeleton (read, plan or project, draw, encode, files written), device_webp off "
                                          "and on alternately; the first run of each is a warm-up",
              "pillow_q85": spread(times[False]), "device_webp": spread(times[True]),
              "speedup_of_medians": round(statistics.median(times[False]) / statistics.median(times[True]), 3),
              "pillow_q85_last_run": last[False], "device_webp_last_run": last[True]})


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--palette", required=True, help="JSON file with keypoint_colors, links and x_link_color (133 keypoints)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scene-frames", type=int, default=150, help="frames of the draw_skeleton measurement (0: skip it)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--log", default=str(ROOT / "profiles" / "webp_bench.log"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("webp_bench needs a HIP device: a time taken elsewhere says nothing")
    dev = torch.device("cuda", torch.cuda.current_device())
    palette = skeleton.load_palette(args.palette)
    import PIL.features
    lines = []
    Path(args.log).parent.mkdir(parents=True, exist_ok=True)
    log = open(args.log, "w")

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)
        log.write(json.dumps(line) + "\n")
        log.flush()
    shown = {k: v for k, v in vars(args).items() if k != "log"}  # where the log goes says nothing about the run
    emit({"what": "run", "device": torch.cuda.get_device_name(dev), "args": shown, "pillow": Image.__version__,
          "libwebp": PIL.features.version("webp"), "content": "133-keypoint figure projected into 48 ring cameras, drawn at 1024 x 1024"})
    tmp = Path(tempfile.mkdtemp(prefix="dm4d_webp_bench_"))
    try:
        scene = tmp / "data" / "bench"
        with ThreadPoolExecutor(args.threads) as pool:
            write_scene(scene, SIZE, SIZE, 48, 1, temporal_cams=[], threads=args.threads)  # for its transforms.json
            Ks, Ts = triang.scene_cameras(str(scene / "transforms.json"), CAMS)
            maps = torch.empty((48, SIZE, SIZE, 3), dtype=torch.uint8, device=dev)
            skeleton.draw_skeleton_maps_kp3d(figure(0)[None], Ks, Ts, [(0, c) for c in range(48)], ((SIZE, SIZE), (SIZE, SIZE)), palette, out=maps)
            for line in bench_encode(maps, args.reps):
                emit(line)
            del maps
            torch.cuda.empty_cache()
            if args.scene_frames > 0:
                bench_stage(scene, tmp / "scene", palette, args.scene_frames, args.threads, args.rounds, pool, dev, emit)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
        log.close()


if __name__ == "__main__":
    main()
