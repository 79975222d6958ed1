#!/usr/bin/env python
"""The `encode` figures of tools/png_bench.py and tools/webp_bench.py at the tools' default sizes and repetitions, for the package under
--pkg (a directory that holds diffuman4d_amd/ with its built library: this tree, or a copy of another commit's package), one JSON
line per tool, appended to --out.  The Pillow and stage parts of the tools, which run no encoder kernel, are left out, so that two
builds can be run alternately, a fresh process each, in a minute; the files' bytes are hashed so that the builds can be seen to agree.

  python tools/encoder_ab.py --pkg . --tag N1 --out profiles/encoder_shared_ab.log
"""
import argparse
import hashlib
import json
import sys
import tempfile
from pathlib import Path

ap = argparse.ArgumentParser()
ap.add_argument("--pkg", required=True)
ap.add_argument("--tag", required=True)
ap.add_argument("--only", default="png,webp")
ap.add_argument("--out", required=True)
args = ap.parse_args()
ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(Path(args.pkg).resolve()), str(ROOT / "tools"), str(ROOT / "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import diffuman4d_amd  # noqa: E402
from bench_common import device_time, kernel_shares  # noqa: E402
from diffuman4d_amd.host import ops, png, skeleton, triang  # noqa: E402

assert Path(diffuman4d_amd.__file__).resolve().parent.parent == Path(args.pkg).resolve(), diffuman4d_amd.__file__
dev = torch.device("cuda", 0)
out = open(args.out, "a")


def emit(line):
    line = {"tag": args.tag, **line}
    print(json.dumps(line), flush=True)
    out.write(json.dumps(line) + "\n")
    out.flush()


def digest(blob, where, n):
    total = where[n - 1] + where[2 * n - 1]
    return hashlib.sha256(blob[:total].cpu().numpy().tobytes() + repr(where).encode()).hexdigest()[:16]


if "png" in args.only:
    import png_bench
    import png_cases
    h, w, n, reps = 2448, 2048, 48, 7
    rgb0, mask0 = png_cases.result_like(h, w)
    pairs = [(np.ascontiguousarray(np.roll(rgb0, 37 * s, axis=1)), np.ascontiguousarray(np.roll(mask0, 37 * s, axis=1))) for s in range(4)]
    rgb = torch.from_numpy(np.stack([pairs[i % 4][0] for i in range(n)])).to(dev)
    masks = torch.from_numpy(np.stack([pairs[i % 4][1] for i in range(n)])).to(dev)
    plans = {"mask": png_bench.descriptors([(png.L, h, w, i * h * w, w) for i in range(n)]),
             "rgba": png_bench.descriptors([(png.RGBA, h, w, i * h * w * 3, 3 * w, i * h * w, w) for i in range(n)])}
    enc = {"what": "encode", "tool": "png_bench", "images": n, "image": [h, w], "reps": reps}
    for kind, (desc, bound, ws) in plans.items():
        call = lambda: ops.png_encode(masks.view(-1), rgb.view(-1) if kind == "rgba" else None, desc, bound, ws)  # noqa: E731
        t = device_time(call, reps)
        blob, o = call()
        enc[f"device_{kind}_seconds_per_file"] = t / n
        enc[f"device_{kind}_sha"] = digest(blob, o.cpu().tolist(), n)
        enc[f"device_{kind}_launch_seconds_per_call"] = kernel_shares(call, r"png_(filter|stripe|scan|offsets|emit)_kernel")
    emit(enc)
    del rgb, masks, blob
    torch.cuda.empty_cache()

if "webp" in args.only:
    import webp_bench
    from capture_bench import write_scene
    from skel_kp3d_bench import CAMS, SIZE, figure
    palette = skeleton.load_palette(str(ROOT / "tests" / "golden" / "skel_palette.json"))
    with tempfile.TemporaryDirectory(prefix="ab_webp_") as tmp:
        scene = Path(tmp) / "data" / "bench"
        write_scene(scene, SIZE, SIZE, 48, 1, temporal_cams=[], threads=16)  # for its transforms.json
        Ks, Ts = triang.scene_cameras(str(scene / "transforms.json"), CAMS)
    maps = torch.empty((48, SIZE, SIZE, 3), dtype=torch.uint8, device=dev)
    skeleton.draw_skeleton_maps_kp3d(figure(0)[None], Ks, Ts, [(0, c) for c in range(48)], ((SIZE, SIZE), (SIZE, SIZE)), palette, out=maps)
    n, reps = 48, 5
    desc, bound, ws = webp_bench.descriptors(n, SIZE, SIZE)
    call = lambda: ops.webp_encode(maps.view(-1), desc, bound, ws)  # noqa: E731
    t = device_time(call, reps)
    blob, o = call()
    emit({"what": "encode", "tool": "webp_bench", "maps": n, "map": [SIZE, SIZE], "reps": reps, "device_seconds_per_map": t / n,
          "device_sha": digest(blob, o.cpu().tolist(), n),
          "device_launch_seconds_per_call": kernel_shares(call, r"webp_(tokens|image|offsets|emit|seam)_kernel")})
