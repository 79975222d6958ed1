#!/usr/bin/env python
"""Time raw-capture rectification (diffuman4d_amd/host/rectify.py, csrc/rectify.hip) at the reference's sizes: --images frames of
--height x --width (2448 x 2048, DNA-Rendering's 5 MP cameras) to 1024 x 1024 by ``calc_unified_cameras``, in batches of --batch.

Measurements, written as JSON lines to --log (default profiles/rectify_bench.log):
  forms     which launch forms of the kernel exist and were measured
  device    dm4d_rectify_u8 on sources already staged on the device: HIP events around one pass over all batches (together larger than
            the 256 MB Infinity Cache, so every pass reads from HBM), after a warm-up pass, median of --reps passes -> time per image,
            and the bytes the pass must move (sources read once, results written) over that time
  host      the same four steps by the numpy / torch-CPU definition (tests/rectify_model.py) on this machine's CPU, --host_images
            images through a pool of 16 threads and on one thread, wall clock -> time per image.  The parent commit has no such stage,
            so this is the only baseline; it is the definition, not an optimised CPU implementation
  equal     whether the device's first image equals the definition's, byte for byte, at this size
  pcie      source bytes over PCIe per image with device_decode off (decoded pixels up) and on (file bytes up): ``bytes_uploaded`` of
            the counts ``extract_images`` returns; the results down, from the shapes
  stage     ``extract_images`` end to end over --images JPEG files, wall clock per image, for .webp and .jpg output with device_decode
            off and on alternately (the first run of each route is a warm-up), and Pillow's encoder alone on 12 threads for the same
            outputs; the .jpg run once more with all --images files in one batch, which gives the one-workgroup-per-image JPEG decoder
            six times as many files per call

  python tools/rectify_bench.py [--images 48 --batch 8 --reps 21]
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
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

import bench_common as bc  # noqa: E402
from diffuman4d_amd.host import ops, rectify, staging  # noqa: E402


def make_image(h: int, w: int, seed: int) -> np.ndarray:
    """A smooth figure on a noisy ground: cheap to make, not constant anywhere."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float32)
    blob = ((xs - w / 2) / (w * 0.22)) ** 2 + ((ys - h / 2) / (h * 0.4)) ** 2 < 1
    base = np.where(blob[..., None], np.array([200, 150, 120], dtype=np.float32), np.array([40, 60, 80], dtype=np.float32))
    return np.clip(base + 0.02 * xs[..., None] + rng.integers(-12, 13, (h, w, 3)), 0, 255).astype(np.uint8)


def camera(h: int, w: int, k: int, image_size: int) -> dict:
    """A camera like DNA-Rendering's 5 MP ones (f = 2496 at 2448 x 2048), a little different for every k."""
    f = 2496.0 * w / 2448.0
    K = [[f * (1 + 0.002 * k), 0, w / 2 + k], [0, f * (1 + 0.002 * k), h / 2 - k], [0, 0, 1]]
    Ku = [[f, 0, w / 2], [0, f, h / 2], [0, 0, 1]]
    cam = {"K": K, "D": [-0.08 - 0.002 * k, 0.05, 5e-4, -3e-4, 0.01], "ccm": [[1e-4, 0.97, 1.0], [-1e-4, 1.02, -1.5], [5e-5, 0.95, 2.0]],
           "K_undist": Ku, "H_undist": h, "W_undist": w, "H": h, "W": w}
    if image_size != 1024:  # a rehearsal size: the reference's target is 1024
        u = rectify.calc_unified_cameras({"00": {"K": np.array(Ku), "H": h, "W": w}}, image_size)["00"]
        cam["resized_wh"], cam["cropped_ltrb"] = list(u["resized_wh"]), list(u["cropped_ltrb"])
    return cam


class Batch:
    """One batch staged on the device: everything the launch needs, made once."""

    def __init__(self, arrays, rects, dev):
        self.n = len(arrays)
        planes, outs = staging.Layout(), staging.Layout()
        desc = np.zeros((self.n, rectify.FIELDS), dtype=np.int64)
        words, used = [], 0
        for k, (a, r) in enumerate(zip(arrays, rects)):
            h, w = a.shape[:2]
            desc[k, :17] = [planes.add(h * w * 3), h, w, r.uh, r.uw, r.rh, r.rw, r.top, r.left, r.ch, r.cw, used, r.hk, used + r.htab.size, r.vk,
                            used + r.htab.size + r.vtab.size, outs.add(r.out_bytes)]
            words.append(r.words)
            used += r.words.size
        host = staging.pinned(planes.total, dev)
        staging.fill(host.numpy(), [(int(desc[k, 0]), a) for k, a in enumerate(arrays)], None)
        self.blob = host.to(dev)
        self.lut = torch.from_numpy(np.stack([r.lut for r in rects])).to(dev)
        self.meta, self.meta_host, self.tab_off, self.tab_len, self.desc_off = staging.pack_meta(np.concatenate(words), desc, dev)
        self.out_bytes, self.out_at = outs.total, [int(v) for v in desc[:, 16]]
        self.moved = sum(a.nbytes for a in arrays) + sum(r.out_bytes for r in rects)
        torch.cuda.synchronize()

    def run(self):
        return ops.rectify(self.blob, self.meta, self.meta_host, self.n, self.desc_off, self.tab_off, self.tab_len, self.lut, self.out_bytes)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=48)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=2048)
    ap.add_argument("--width", type=int, default=2448)
    ap.add_argument("--image_size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--host_images", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--log", default=str(ROOT / "profiles" / "rectify_bench.log"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("rectify_bench needs a HIP device: nothing here is measured on the CPU alone")
    import rectify_model as rm
    dev = torch.device("cuda:0")
    h, w, n = args.height, args.width, args.images
    ncam = min(n, 6)
    cameras = {f"{k:02d}": camera(h, w, k, args.image_size) for k in range(ncam)}
    rects = rectify.load_cameras(cameras)
    labels = sorted(rects)
    arrays = [make_image(h, w, k) for k in range(n)]
    cam_of = [labels[k % ncam] for k in range(n)]
    lines = [{"what": "forms", "built": ["one launch: undistorted patch of a 32 x 8 output tile in LDS"], "measured": ["one launch"],
              "two_launch_form": "not built, not measured"}]
    shape = {"images": n, "batch": args.batch, "source": [h, w], "resized_wh": [rects[labels[0]].rw, rects[labels[0]].rh],
             "crop": [rects[labels[0]].ch, rects[labels[0]].cw], "device": torch.cuda.get_device_name(0)}

    # device
    batches = [Batch(arrays[i:i + args.batch], [rects[c] for c in cam_of[i:i + args.batch]], dev) for i in range(0, n, args.batch)]
    keep = []

    def one_pass():
        keep[:] = [b.run() for b in batches]
    t = bc.device_time(one_pass, args.reps)
    moved = sum(b.moved for b in batches)
    lines.append({"what": "device", **shape, "reps": args.reps, "seconds_per_pass": t, "us_per_image": t / n * 1e6, "bytes_moved_per_pass": moved,
                  "GB_per_s": moved / t / 1e9, "kernels": bc.kernel_shares(one_pass, r"rectify_kernel")})
    first = keep[0][batches[0].out_at[0]: batches[0].out_at[0] + rects[cam_of[0]].out_bytes].cpu().numpy()

    # host: the definition on this machine's CPU
    def model(k):
        c = cameras[cam_of[k]]
        r = rects[cam_of[k]]
        return rm.rectify(arrays[k], c["K"], c["D"], c["ccm"], c["K_undist"], (h, w), (r.rw, r.rh), (r.left, r.top, r.left + r.cw, r.top + r.ch))
    times = bc.pillow_times(model, list(range(min(args.host_images, n))))
    lines.append({"what": "host", "definition": "tests/rectify_model.py (numpy + torch CPU)", "images_16_threads": min(args.host_images, n),
                  "seconds_per_image_1_thread": times[1][0], "seconds_per_image_16_threads": times[16][0]})
    lines.append({"what": "equal", "device_equals_definition_first_image": bool(np.array_equal(first, times[16][1][0].reshape(-1)))})
    del batches, keep

    # the stage end to end
    tmp = Path(tempfile.mkdtemp(prefix="rectify_bench_"))
    try:
        files = []
        for k, a in enumerate(arrays):
            p = tmp / "raw" / cam_of[k] / f"{k:06d}.jpg"
            p.parent.mkdir(parents=True, exist_ok=True)
            Image.fromarray(a).save(p, quality=92)
            files.append((cam_of[k], f"{k:06d}", str(p)))
        file_bytes = sum(Path(f[2]).stat().st_size for f in files)
        out_bytes = sum(rects[c].out_bytes for c in cam_of)
        for ext, batch in ((".webp", args.batch), (".jpg", args.batch), (".jpg", n)):
            counts = {}

            def run(flag, r):
                out = tmp / f"out{ext[1:]}_{int(flag)}_{r}"
                t0 = time.perf_counter()
                counts[flag] = rectify.extract_images(files, cameras, str(out), ext, 85, False, 12, batch_size=batch, gpu_ids=[0], device_decode=flag)
                dt = time.perf_counter() - t0
                shutil.rmtree(out)
                return dt
            ts = bc.alternate(run, args.rounds)
            sample = [np.ascontiguousarray(first.reshape(rects[cam_of[0]].ch, rects[cam_of[0]].cw, 3))] * n

            def encode(a):
                buf = io.BytesIO()
                Image.fromarray(a).save(buf, format="WEBP" if ext == ".webp" else "JPEG", quality=85)
                return buf.tell()
            with ThreadPoolExecutor(max_workers=12) as pool:
                t0 = time.perf_counter()
                list(pool.map(encode, sample))
                enc = time.perf_counter() - t0
            if ext == ".webp":  # the stage's own counter of source bytes uploaded; the results come down as counted from the shapes
                lines.append({"what": "pcie", "up_per_image_device_decode_off": counts[False]["bytes_uploaded"] / n,
                              "up_per_image_device_decode_on": counts[True]["bytes_uploaded"] / n, "file_bytes_per_image": file_bytes / n,
                              "down_per_image": out_bytes / n, "note": "device_decode on: every file here is a baseline JPEG the decoder takes"})
            lines.append({"what": "stage", "image_ext": ext, "images": n, "batch_size": batch, "num_workers": 12,
                          "ms_per_image_device_decode_off": [x / n * 1e3 for x in ts[False]], "ms_per_image_device_decode_on": [x / n * 1e3 for x in ts[True]],
                          "median_off": statistics.median(ts[False]) / n * 1e3, "median_on": statistics.median(ts[True]) / n * 1e3,
                          "pillow_encode_alone_12_threads_ms_per_image": enc / n * 1e3, "counts_off": counts[False], "counts_on": counts[True]})
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    Path(args.log).parent.mkdir(parents=True, exist_ok=True)
    with open(args.log, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
            print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
