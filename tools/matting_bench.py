#!/usr/bin/env python
"""Time the foreground-mask stage's own arithmetic (diffuman4d_amd/host/matting.py, csrc/matting.hip) at the reference's sizes: --images
captured images of --height x --width (2448 x 2048, DNA-Rendering) to the network's 1024 x 1024 and the masks back, in batches of
--batch.  The matting network itself is the caller's and is not timed: an identity-cost stand-in (``lambda x: x[:, :1]``) makes the logits.

Measurements, written as JSON lines to --log (default profiles/matting_bench.log):
  device    dm4d_matting_input_u8 (fp16) and dm4d_matting_mask_f16_u8 on images already staged on the device: HIP events around one
            pass over all batches (together larger than the 256 MB Infinity Cache, so every pass reads from HBM), after a warm-up
            pass, median of --reps passes -> time per image of each stage
  host      the same two stages the reference's way on this machine's CPU: Pillow's resize + ToTensor + Normalize + .half(), and
            to_pil_image of an fp16 sigmoid map + Pillow's resize back, on --host_images images, one thread and a pool of 16 threads,
            wall clock -> time per image
  pcie      bytes over PCIe per image for each route, counted from the shapes: uint8 image up and uint8 mask down here; the fp32
            network input up and the fp16 sigmoid map down in the reference
  equal     whether the device's input and mask of the first image equal the host route's, byte for byte
and to --parity_log (default profiles/matting_parity.log): on how many fp16 bit patterns the quantiser's definition (a table) differs
from this device's own fp16 ``sigmoid().mul(255).byte()``, next to the same count for torch CPU.

  python tools/matting_bench.py [--images 48 --batch 8 --reps 21]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch
from PIL import Image

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from diffuman4d_amd.host import matting, ops, staging  # noqa: E402

NET = (1024, 1024)


def make_image(h: int, w: int, seed: int) -> np.ndarray:
    """A smooth figure on a noisy ground: cheap to make, not constant anywhere."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float32)
    blob = ((xs - w / 2) / (w * 0.22)) ** 2 + ((ys - h / 2) / (h * 0.4)) ** 2 < 1
    base = np.where(blob[..., None], np.array([200, 150, 120], dtype=np.float32), np.array([40, 60, 80], dtype=np.float32))
    return np.clip(base + rng.integers(-30, 31, (h, w, 3)), 0, 255).astype(np.uint8)


class Batch:
    """One batch staged on the device: everything the two launches need, made once."""

    def __init__(self, arrays, dev):
        self.sizes = [a.shape[:2] for a in arrays]
        self.n = len(arrays)
        desc, tab, plane_bytes, scratch_bytes = matting._plan(self.sizes, NET, 0, True)
        host = staging.pinned(plane_bytes, dev)
        staging.fill(host.numpy(), [(int(desc[k, 0]), a) for k, a in enumerate(arrays)], None)
        self.blob = host.to(dev)
        self.in_meta, self.in_meta_host, _, self.in_tab_len, self.in_desc_off = staging.pack_meta(tab, desc, dev)
        self.in_scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=dev)
        desc, tab, self.blob_bytes, scratch_bytes = matting._plan(self.sizes, NET, 0, False)
        self.out_desc = desc
        self.out_meta, self.out_meta_host, _, self.out_tab_len, self.out_desc_off = staging.pack_meta(tab, desc, dev)
        self.out_scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=dev)
        self.lut, self.qtab = matting._on_device(torch.float16, dev), matting._on_device("q", dev)
        torch.cuda.synchronize()
        self.logits = None

    def inputs(self):
        return ops.matting_input(self.blob, self.in_meta, self.in_meta_host, self.n, self.in_desc_off, 0, self.in_tab_len, self.lut, self.in_scratch,
                                 NET[0], NET[1], 0)

    def masks(self):
        return ops.matting_mask(self.logits, self.out_meta, self.out_meta_host, self.n, self.out_desc_off, 0, self.out_tab_len, self.qtab,
                                self.out_scratch, self.blob_bytes, 0)


def device_time(fn, reps: int) -> float:
    """Median over `reps` passes of the HIP-event time of one pass, in seconds, after one warm-up pass."""
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / 1e3)
    return statistics.median(times)


def host_input(a: np.ndarray) -> torch.Tensor:
    import matting_model as M
    return M.matting_input(a, NET, 0, torch.float16)


def host_mask(sig: torch.Tensor, hw) -> np.ndarray:
    """to_pil_image of an fp16 sigmoid map [S_h, S_w] (.mul(255).byte()) and Pillow's default resize to the image's size."""
    return np.asarray(Image.fromarray(sig.mul(255).byte().numpy()).resize((hw[1], hw[0])))


def wall(fn, items, threads: int) -> float:
    t0 = time.perf_counter()
    if threads == 1:
        for it in items:
            fn(it)
    else:
        with ThreadPoolExecutor(max_workers=threads) as pool:
            list(pool.map(fn, items))
    return (time.perf_counter() - t0) / len(items)


def parity(dev) -> dict:
    import matting_model as M
    patterns = torch.from_numpy(np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16).copy())
    finite = ~torch.isnan(patterns)
    q = M.quantise(patterns)
    on_device = patterns.to(dev).sigmoid().mul(255).byte().cpu()
    on_cpu = patterns.sigmoid().mul(255).byte()
    table = torch.from_numpy(matting.quantiser_table())
    return {"what": "parity", "device": torch.cuda.get_device_name(dev), "non_nan_patterns": int(finite.sum()),
            "definition_vs_device_fp16_sigmoid_mul255_byte": int((q[finite] != on_device[finite]).sum()),
            "definition_vs_torch_cpu_fp16_sigmoid_mul255_byte": int((q[finite] != on_cpu[finite]).sum()),
            "host_table_vs_definition": int((table != q).sum())}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=48)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=2448)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--host_images", type=int, default=16, help="images the host route is timed on")
    ap.add_argument("--log", default=str(ROOT / "profiles" / "matting_bench.log"))
    ap.add_argument("--parity_log", default=str(ROOT / "profiles" / "matting_parity.log"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("matting_bench needs a HIP device: a time taken elsewhere says nothing")
    dev = torch.device("cuda", torch.cuda.current_device())
    h, w = args.height, args.width
    lines = [{"what": "setup", "device": torch.cuda.get_device_name(dev), "images": args.images, "batch": args.batch, "image": [h, w],
              "network": list(NET), "reps": args.reps, "network_stand_in": "lambda x: x[:, :1]"}]

    distinct = [make_image(h, w, s) for s in range(min(args.batch, args.images))]  # the batches hold copies at their own addresses
    batches = [Batch([distinct[(i + j) % len(distinct)] for j in range(min(args.batch, args.images - i))], dev) for i in range(0, args.images, args.batch)]
    for b in batches:
        b.logits = b.inputs()[:, :1].contiguous()
    torch.cuda.synchronize()
    staged = sum(b.blob.numel() for b in batches)
    t_in = device_time(lambda: [b.inputs() for b in batches], args.reps)
    t_out = device_time(lambda: [b.masks() for b in batches], args.reps)
    lines.append({"what": "device", "input_seconds_per_image": t_in / args.images, "mask_seconds_per_image": t_out / args.images,
                  "both_seconds_per_image": (t_in + t_out) / args.images, "staged_image_bytes_per_pass": staged,
                  "input_source_bytes_per_second": staged / t_in, "mask_bytes_per_second": h * w * args.images / t_out,
                  "timing": f"HIP events around one pass over {len(batches)} batches, warm, median of {args.reps}"})

    # the host route, and equality on the first image
    b0 = batches[0]
    x0 = b0.inputs()
    m0 = b0.masks().cpu().numpy()
    want_x = host_input(distinct[0])
    sig = b0.logits[0, 0].sigmoid().cpu()   # the reference's map: the device's own fp16 sigmoid, copied back
    got_mask = m0[int(b0.out_desc[0, 0]): int(b0.out_desc[0, 0]) + h * w].reshape(h, w)
    import matting_model as M
    lines.append({"what": "equal", "input_bit_equal_to_pillow_torch_cpu": bool(torch.equal(x0[0].cpu(), want_x)),
                  "mask_byte_equal_to_definition_pillow": bool(np.array_equal(got_mask, M.matting_mask(b0.logits[0].cpu(), (h, w)))),
                  "mask_bytes_differing_from_device_sigmoid_route": int((got_mask != host_mask(sig, (h, w))).sum())})
    torch.set_num_threads(1)  # the pool below is the parallelism: 16 threads in all
    items = [distinct[i % len(distinct)] for i in range(args.host_images)]
    sigs = [sig] * args.host_images
    host = {"what": "host", "images": args.host_images}
    for threads in (1, 16):
        host[f"input_seconds_per_image_{threads}_threads"] = wall(host_input, items, threads)
        host[f"mask_seconds_per_image_{threads}_threads"] = wall(lambda s: host_mask(s, (h, w)), sigs, threads)
    lines.append(host)
    lines.append({"what": "pcie", "native_bytes_up_per_image": h * w * 3, "native_bytes_down_per_image": h * w,
                  "reference_bytes_up_per_image": 3 * NET[0] * NET[1] * 4, "reference_bytes_down_per_image": NET[0] * NET[1] * 2,
                  "note": "native: the uint8 image up, the uint8 mask down; reference: the fp32 network input up, the fp16 sigmoid map down"})
    for path, rows in ((args.log, lines), (args.parity_log, [parity(dev)])):
        Path(path).parent.mkdir(parents=True, exist_ok=True)
        with open(path, "w") as f:
            for line in rows:
                print(json.dumps(line))
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
