#!/usr/bin/env python
"""What drawing skeleton maps straight from ``poses_3d`` (``skeleton_source="kp3d"``, ``draw_skeleton(kp3d_dir=...)``) costs against
the route through a ``poses_2d`` directory, on one scene of 48 cameras and --frames frames with 1024 x 1024 maps.  JSON lines, written
to --log (default profiles/skel_kp3d_bench.log):

  maps       per map, for 48 x 1 and 2 x --frames maps: ``plan_draw_calls`` + ``pack_calls`` + upload + draw (``draw_plans_into`` on
             instances already read) against plan + draw from kp3d on the device (``draw_skeleton_maps_kp3d(out=...)`` on a scene already
             uploaded, its status read-back included), both into a buffer on the device, alternately, medians of --rounds after a warm-up;
             whether the two buffers hold the same bytes
  get_item   wall seconds of ``SpaTemDataset.get_item`` (has_gt_target=False) for skeleton_source="kp2d" against "kp3d", a spatial task of
             48 frames and a temporal one of 2 x --frames, alternately, medians of --rounds; whether the samples are equal
  scene      ``triangulate_skeleton`` + ``draw_skeleton`` for 48 x --scene-frames maps (WebP files): with ``out_kp2d_proj_dir`` and
             ``draw_skeleton(kp2d_dir)`` against without it and ``draw_skeleton(kp3d_dir=...)``; seconds per stage, files written, and
             whether the image files are the same bytes

  python tools/skel_kp3d_bench.py --palette tests/golden/skel_palette.json [--frames 150 --scene-frames 150 --rounds 5 --threads 16]
"""
from __future__ import annotations

import argparse
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

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from bench_common import alternate  # noqa: E402
from capture_bench import write_scene  # noqa: E402
from diffuman4d_amd.host import capture, skeleton, triang  # noqa: E402

INPUTS = ["01", "13", "25", "37"]
CAMS = [f"{c:02d}" for c in range(48)]
SIZE = 1024


def figure(t: int) -> np.ndarray:
    """A 133-keypoint figure around the origin that every camera of the ring sees whole, moving with the frame."""
    i = np.arange(133)
    ang, rad = i * 2.399963 + 0.02 * t, 0.1 + 0.5 * ((i * 37) % 133) / 133
    return np.stack([0.5 * rad * np.cos(ang), 0.9 * rad * np.sin(ang), 0.3 * rad * np.cos(3 * ang + 0.05 * t)], -1)


def spread(xs) -> dict:
    return {"seconds": [round(x, 4) for x in xs], "median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def write_poses(scene: Path, frames, cams_by_frame, pool, dev) -> None:
    """poses_3d/{frame}.json, and poses_2d/{cam}/{frame}.json for the named cameras as triangulate_skeleton writes them."""
    Ks, Ts = triang.scene_cameras(str(scene / "transforms.json"), CAMS)
    kp3d = np.stack([figure(t) for t in frames])
    uv, depth, _ = triang.project_points(kp3d, Ks, Ts, device=dev)
    jobs = [(triang.write_kp3d, (scene / "poses_3d" / f"{t:06d}.json", kp3d[f], np.zeros(133))) for f, t in enumerate(frames)]
    jobs += [(triang.write_kp2d, (scene / "poses_2d" / cam / f"{t:06d}.json", uv[f, CAMS.index(cam)], depth[f, CAMS.index(cam)]))
             for f, t in enumerate(frames) for cam in cams_by_frame(t)]
    list(pool.map(lambda j: j[0](*j[1]), jobs))


def bench_maps(scene: Path, palette, labels, rounds: int, dev) -> dict:
    """labels: [(cam, frame)]"""
    shapes = ((SIZE, SIZE), (SIZE, SIZE))
    instances = [skeleton._read_instance(scene / "poses_2d" / cam / f"{t:06d}.json") for cam, t in labels]
    frames = sorted({t for _, t in labels})
    Ks, Ts = triang.scene_cameras(str(scene / "transforms.json"), CAMS)
    dscene = skeleton.upload_scene(np.stack([skeleton.read_kp3d(scene / "poses_3d" / f"{t:06d}.json") for t in frames]), Ks, Ts, dev)
    jobs = [(frames.index(t), CAMS.index(cam)) for cam, t in labels]
    tables = skeleton.plan_tables(palette)
    out = {flag: torch.empty((len(labels), SIZE, SIZE, 3), dtype=torch.uint8, device=dev) for flag in (False, True)}
    phases = {}

    def run(flag, r):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if flag:
            skeleton.draw_skeleton_maps_kp3d(dscene, None, None, jobs, shapes, tables, out=out[True])
        else:
            plans = [skeleton.plan_draw_calls(inst, None, shapes, palette) for inst in instances]
            phases["host_plan_s"] = round(time.perf_counter() - t0, 4)
            skeleton.draw_plans_into(plans, out[False])
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    times = alternate(run, rounds)
    n = len(labels)
    return {"what": "maps", "maps": n, "out": [SIZE, SIZE], "rounds": rounds,
            "timing": "wall clock incl. a device synchronise; file route: plan_draw_calls + pack_calls + upload + draw of read instances; kp3d: "
                      "plan + draw on the device of an uploaded scene + the status read-back",
            "file_route": spread(times[False]), "kp3d": spread(times[True]), "host_plan_s_last_round": phases["host_plan_s"],
            "per_map_ms_file_route": round(1e3 * statistics.median(times[False]) / n, 4),
            "per_map_ms_kp3d": round(1e3 * statistics.median(times[True]) / n, 4),
            "speedup_of_medians": round(statistics.median(times[False]) / statistics.median(times[True]), 3),
            "equal": bool(torch.equal(out[False], out[True]))}


def bench_get_item(root: Path, palette, task: str, spa, tem, threads: int, rounds: int) -> dict:
    ds = {flag: capture.SpaTemDataset(data_dir=str(root), scene_label="bench", height=SIZE, width=SIZE, decode_threads=threads, plucker="cameras",
                                      has_gt_target=False, skeleton_source="kp3d" if flag else "kp2d", palette=palette) for flag in (False, True)}
    last = {}

    def run(flag, r):
        t0 = time.perf_counter()
        last[flag] = ds[flag].get_item("bench", spa, tem, INPUTS)
        return time.perf_counter() - t0
    times = alternate(run, rounds)
    a, b = last[False], last[True]
    return {"what": "get_item", "task": task, "frames": len(a["labels"]), "src": [SIZE, SIZE], "out": SIZE, "has_gt_target": False,
            "decode_threads": threads, "rounds": rounds, "timing": "wall clock of get_item, kp2d and kp3d alternately; the first round is a warm-up",
            "kp2d": spread(times[False]), "kp3d": spread(times[True]),
            "speedup_of_medians": round(statistics.median(times[False]) / statistics.median(times[True]), 3),
            "equal": bool(torch.equal(a["pixel_values"], b["pixel_values"]) and torch.equal(a["skeletons"], b["skeletons"]) and a["crops"] == b["crops"])}


def bench_scene(scene: Path, tmp: Path, palette, n_frames: int, threads: int, pool, dev) -> dict:
    """Detections for every camera and frame (the figure's projection, score 0.9), then the two routes from them to skeletons/*.webp."""
    Ks, Ts = triang.scene_cameras(str(scene / "transforms.json"), CAMS)
    uv, _, _ = triang.project_points(np.stack([figure(t) for t in range(n_frames)]), Ks, Ts, device=dev)
    sap = tmp / "poses_sapiens"
    list(pool.map(lambda j: triang.write_kp2d(sap / CAMS[j[1]] / f"{j[0]:06d}.json", uv[j[0], j[1]], None, np.full(133, 0.9)),
                  [(t, c) for t in range(n_frames) for c in range(48)]))
    out = {"what": "scene", "cameras": 48, "frames": n_frames, "maps": 48 * n_frames, "out": [SIZE, SIZE], "num_workers": threads,
           "timing": "wall clock of each stage, one run each, the poses_2d route first"}
    for name in ("poses_2d", "kp3d"):
        d = tmp / name
        t0 = time.perf_counter()
        tri = triang.triangulate_skeleton(str(scene / "transforms.json"), str(sap), str(d / "poses_3d"), num_workers=threads, device=dev,
                                          **({"out_kp2d_proj_dir": str(d / "poses_2d")} if name == "poses_2d" else {}))
        t1 = time.perf_counter()
        kw = dict(palette=palette, num_workers=threads, device=dev)
        if name == "poses_2d":
            drw = skeleton.draw_skeleton(str(d / "poses_2d"), str(d / "skeletons"), **kw)
        else:
            drw = skeleton.draw_skeleton(None, str(d / "skeletons"), kp3d_dir=str(d / "poses_3d"), camera_path=str(scene / "transforms.json"), **kw)
        t2 = time.perf_counter()
        out[name] = {"triangulate_skeleton_s": round(t1 - t0, 3), "draw_skeleton_s": round(t2 - t1, 3), "total_s": round(t2 - t0, 3),
                     "json_files_written": tri["files"], "triangulate_seconds": tri["seconds"], "draw_seconds": drw["seconds"], "maps": drw["files"]}
    files = {name: {p.relative_to(tmp / name / "skeletons").as_posix(): p.read_bytes() for p in sorted((tmp / name / "skeletons").rglob("*.webp"))}
             for name in ("poses_2d", "kp3d")}
    out["speedup_of_totals"] = round(out["poses_2d"]["total_s"] / out["kp3d"]["total_s"], 3)
    out["same_image_files"] = files["poses_2d"] == files["kp3d"] and len(files["kp3d"]) == 48 * n_frames
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--palette", required=True, help="JSON file with keypoint_colors, links and x_link_color (133 keypoints)")
    ap.add_argument("--frames", type=int, default=150, help="frames per camera of the temporal task")
    ap.add_argument("--scene-frames", type=int, default=150, help="frames of the whole-scene measurement (0: skip it)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--log", default=str(ROOT / "profiles" / "skel_kp3d_bench.log"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("skel_kp3d_bench: no HIP device (nothing here is measured without one)")
    dev = torch.device("cuda", torch.cuda.current_device())
    palette = skeleton.load_palette(args.palette)
    lines = [{"what": "run", "device": torch.cuda.get_device_name(dev), "args": vars(args)}]
    tmp = Path(tempfile.mkdtemp(prefix="dm4d_skel_kp3d_"))

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)
    try:
        scene = tmp / "data" / "bench"
        with ThreadPoolExecutor(args.threads) as pool:
            t0 = time.perf_counter()
            write_scene(scene, SIZE, SIZE, 48, args.frames, temporal_cams=["03", "01"], threads=args.threads)
            shutil.rmtree(scene / "poses_2d")  # the synthetic detections of capture_bench: replaced by the projection of poses_3d
            write_poses(scene, range(args.frames), lambda t: CAMS if t == 0 else ["03", "01"], pool, dev)
            print(f"# scene written in {time.perf_counter() - t0:.1f} s", flush=True)
            temporal = [(cam, t) for cam in ("01", "03") for t in range(args.frames)]
            for labels in ([(cam, 0) for cam in CAMS], temporal):
                emit(bench_maps(scene, palette, labels, args.rounds, dev))
            for task, spa, tem in (("spatial", CAMS, ["000000"]), ("temporal", ["03"], [f"{t:06d}" for t in range(args.frames)])):
                emit(bench_get_item(tmp / "data", palette, task, spa, tem, args.threads, args.rounds))
            if args.scene_frames > 0:
                emit(bench_scene(scene, tmp / "scene", palette, args.scene_frames, args.threads, pool, dev))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    Path(args.log).parent.mkdir(parents=True, exist_ok=True)
    with open(args.log, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
