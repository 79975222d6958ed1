#!/usr/bin/env python
"""What ``device_decode`` does to a captured-scene ``get_item`` (diffuman4d_amd/host/capture.py) and to ``predict_keypoints``
(diffuman4d_amd/host/pose.py): wall time and bytes over PCIe with the flag off and on, alternately in one process.

Per source size of --src (default 1024x1024 and 2448x2048) the scene of tools/capture_bench.py is written once (48 cameras; a spatial
task of 48 frames and a temporal task of 2 x --frames frames) and read as two scenes:
  fdvai          JPEG images and skeleton maps (quality 90, 4:2:0), PNG masks: every file may decode on the device
  dna_rendering  WebP images and skeleton maps, PNG masks: only the masks may; the WebP files stay with Pillow inside the same call
JSON lines, written to --log (default profiles/capture_decode_bench.log):
  get_item   per scene and task: wall seconds of ``get_item`` (it ends in a stream synchronise), the flag off and on alternately for
             --rounds rounds after one warm-up round -> every time, the median and the range; bytes over PCIe per call (flag off: the
             decoded planes of the staging buffer; flag on: ``decode_stats["bytes_uploaded"]``, file payloads + the planes Pillow
             decoded); the files each route decoded; whether the two calls returned equal tensors and crops
  pose       ``predict_keypoints`` over the 1024 x 1024 fdvai scene's first --pose-images images and masks with a stand-in network
             (an average pool), bbox_source="fmask", the flag off and on alternately; whether the JSON files are the same

  python tools/capture_decode_bench.py [--src 1024x1024,2448x2048 --frames 150 --rounds 5 --threads 16]
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

import torch
from PIL import Image

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from bench_common import alternate  # noqa: E402
from capture_bench import write_scene  # noqa: E402
from diffuman4d_amd.host import capture, pose  # noqa: E402

INPUTS = ["01", "13", "25", "37"]
SCENES = {"fdvai": ("images_jpg", "skeletons_jpg", ".jpg"), "dna_rendering": ("images", "skeletons", ".webp")}


def add_jpeg_files(scene: Path, threads: int) -> None:
    """images_jpg/ and skeletons_jpg/: the scene's WebP files re-saved as baseline JPEG (Pillow's default 4:2:0)."""
    def one(p: Path):
        q = scene / f"{p.parent.parent.name}_jpg" / p.parent.name / (p.stem + ".jpg")
        q.parent.mkdir(parents=True, exist_ok=True)
        Image.open(p).save(q, quality=90)
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(one, sorted((scene / "images").rglob("*.webp")) + sorted((scene / "skeletons").rglob("*.webp"))))


def spread(xs) -> dict:
    return {"seconds": [round(x, 4) for x in xs], "median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def bench_get_item(root: Path, name: str, task: str, spa, tem, out: int, threads: int, rounds: int, hw) -> dict:
    images, skeletons, ext = SCENES[name]
    pats = {"image_path_pat": "{data_dir}/{scene_label}/" + images + "/{spa_label}/{tem_label}" + ext,
            "skeleton_path_pat": "{data_dir}/{scene_label}/" + skeletons + "/{spa_label}/{tem_label}" + ext}
    ds = {flag: capture.SpaTemDataset(data_dir=str(root), scene_label="bench", height=out, width=out, decode_threads=threads, plucker="cameras",
                                      **pats, **({"device_decode": True} if flag else {})) for flag in (False, True)}
    last = {}

    def run(flag, r):
        t0 = time.perf_counter()
        last[flag] = ds[flag].get_item("bench", spa, tem, INPUTS)
        return time.perf_counter() - t0
    times = alternate(run, rounds)
    a, b = last[False], last[True]
    calls = rounds + 1
    frames = len(a["labels"])
    stats = ds[True].decode_stats
    return {"what": "get_item", "scene": name, "task": task, "frames": frames, "src": [hw[1], hw[0]], "out": out, "decode_threads": threads,
            "rounds": rounds, "timing": "wall clock of get_item, flag off and on alternately; the first round is a warm-up",
            "flag_off": spread(times[False]), "flag_on": spread(times[True]),
            "speedup_of_medians": round(statistics.median(times[False]) / statistics.median(times[True]), 3),
            "bytes_over_pcie_flag_off": frames * hw[0] * hw[1] * 7, "bytes_over_pcie_flag_on": stats["bytes_uploaded"] // calls,
            "files_device": stats["device"] // calls, "files_pillow": stats["pillow"] // calls,
            "equal": bool(torch.equal(a["pixel_values"], b["pixel_values"]) and torch.equal(a["skeletons"], b["skeletons"])
                          and a["crops"] == b["crops"] and torch.equal(a["Ks"], b["Ks"]))}


def bench_pose(scene: Path, tmp: Path, n: int, threads: int, rounds: int, dev: torch.device) -> dict:
    for sub, ext in (("images_jpg", ".jpg"), ("fmasks", ".png")):
        for p in sorted((scene / sub).glob(f"*/000000{ext}"))[:n]:
            q = tmp / "pose" / sub / p.parent.name / p.name
            q.parent.mkdir(parents=True, exist_ok=True)
            shutil.copyfile(p, q)
    net = lambda x: torch.nn.functional.avg_pool2d(x[:, :1] + x[:, 1:2] * 0.5 - x[:, 2:], 4).repeat(1, 17, 1, 1)  # noqa: E731
    trees = {}

    def run(flag, r):
        dst = tmp / "pose" / f"kp_{int(flag)}"
        shutil.rmtree(dst, ignore_errors=True)
        t0 = time.perf_counter()
        res = pose.predict_keypoints(str(tmp / "pose" / "images_jpg"), str(dst), str(tmp / "pose" / "fmasks"), pose_model=net, gpu_ids=[dev.index],
                                     num_workers=threads, batch_size=8, skip_exists=False, bbox_source="fmask", **({"device_decode": True} if flag else {}))
        dt = time.perf_counter() - t0
        assert res["written"] == n
        trees[flag] = {p.relative_to(dst).as_posix(): p.read_bytes() for p in sorted(dst.rglob("*.json"))}
        return dt
    times = alternate(run, rounds)
    return {"what": "pose", "images": n, "src": [1024, 1024], "network_input": [1024, 768], "batch_size": 8, "num_workers": threads, "rounds": rounds,
            "timing": "wall clock of predict_keypoints (files read, decoded, warped, a stand-in network, decoded heatmaps, JSON written)",
            "flag_off": spread(times[False]), "flag_on": spread(times[True]),
            "speedup_of_medians": round(statistics.median(times[False]) / statistics.median(times[True]), 3), "same_json_files": trees[False] == trees[True]}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--src", default="1024x1024,2448x2048", help="source sizes W x H, comma-separated")
    ap.add_argument("--out", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=150, help="frames per camera of the temporal task")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16, help="decode threads of the dataset, workers of the pose stage")
    ap.add_argument("--pose-images", type=int, default=48)
    ap.add_argument("--log", default=str(ROOT / "profiles" / "capture_decode_bench.log"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("capture_decode_bench: no HIP device (nothing here is measured without one)")
    dev = torch.device("cuda", torch.cuda.current_device())
    lines = [{"what": "run", "device": torch.cuda.get_device_name(dev), "args": vars(args)}]
    tmp = Path(tempfile.mkdtemp(prefix="dm4d_capture_decode_"))
    try:
        for k, src in enumerate(args.src.split(",")):
            W, H = (int(v) for v in src.split("x"))
            root = tmp / src
            t0 = time.perf_counter()
            write_scene(root / "bench", W, H, 48, args.frames, temporal_cams=["03", "01"], threads=args.threads)
            add_jpeg_files(root / "bench", args.threads)
            print(f"# scene {src} written in {time.perf_counter() - t0:.1f} s", flush=True)
            for name in SCENES:
                for task, spa, tem in (("spatial", [f"{c:02d}" for c in range(48)], ["000000"]),
                                       ("temporal", ["03"], [f"{t:06d}" for t in range(args.frames)])):
                    lines.append(bench_get_item(root, name, task, spa, tem, args.out, args.threads, args.rounds, (H, W)))
                    print(json.dumps(lines[-1]), flush=True)
            if (W, H) == (1024, 1024) and args.pose_images > 0:
                lines.append(bench_pose(root / "bench", tmp, args.pose_images, args.threads, args.rounds, dev))
                print(json.dumps(lines[-1]), flush=True)
            shutil.rmtree(root, ignore_errors=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    Path(args.log).parent.mkdir(parents=True, exist_ok=True)
    with open(args.log, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
