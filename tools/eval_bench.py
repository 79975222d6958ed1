#!/usr/bin/env python
"""What result evaluation costs (diffuman4d_amd/host/metrics.py, csrc/metrics.hip).

Writes a seeded result directory (predicted .jpg, captured .webp, mask .png at ``--src WxH``) and reports:
  kernel      the launches of dm4d_eval_psnr_ssim_f64 for one batch of ``--batch`` pairs already on the device (device events, best of
              ``--reps``), per pair, at ``--src`` resized to the canvas (2448x2048 -> 1224x1024)
  decode      Pillow decode of the batch's 3 files per pair in the evaluator's thread pool (wall)
  evaluate    evaluate_results over the whole directory, decode included (wall) -> pairs/s
  torch cpu   the fp32 torch-CPU model of the same steps (tests/eval_model.py) on ``--cpu-threads`` threads, per pair, on files already
              decoded -- for scale: it is the arithmetic torchmetrics runs
  lpips       with ``--lpips VGG16 LIN`` (torchvision's VGG-16 checkpoint and the LPIPS linear layers; ``python tests/lpips_model.py DIR``
              writes a seeded full-width pair of such files when the real ones are not at hand -- the cost does not depend on the values):
              ``evaluate_batch`` over ``--lpips-pairs`` pairs without and with ``LpipsVGG`` (wall, decode included, best of ``--reps``) and
              the span of one LpipsVGG call (device events around its ~45 launches, their host-side gaps and the final read-back), per pair

  python tools/eval_bench.py --src 2448x2048 --canvas 1024 --batch 64 --pairs 128 --threads 16 [--lpips vgg16-397923af.pth vgg.pth]
"""
from __future__ import annotations

import argparse
import json
import math
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from diffuman4d_amd.host import metrics  # noqa: E402


def write_results(root: Path, W: int, H: int, n_cams: int, n_frames: int, threads: int) -> None:
    from PIL import Image
    yy, xx = np.mgrid[:H, :W]

    def one(job):
        c, t = job
        rng = np.random.default_rng(1000 * c + t)
        cx, cy = W / 2 + 0.1 * W * math.sin(c + t / 10), H / 2 + 0.05 * H * math.cos(c)
        inside = ((xx - cx) / (0.22 * W)) ** 2 + ((yy - cy) / (0.42 * H)) ** 2 < 1
        img = np.stack([(xx // 3 + 20 * c) % 256, (yy // 3 + t) % 256, ((xx + yy) // 5) % 256], -1).astype(np.uint8)
        pred = np.clip(img.astype(np.int16) + rng.integers(-8, 9, img.shape), 0, 255).astype(np.uint8)
        for sub, arr, ext in (("gt", img, "webp"), ("pred/images", pred, "jpg"), ("fmasks", np.where(inside, 255, 0).astype(np.uint8), "png")):
            p = root / sub / f"{c:02d}" / f"{t:06d}.{ext}"
            p.parent.mkdir(parents=True, exist_ok=True)
            Image.fromarray(arr).save(p) if ext == "png" else Image.fromarray(arr).save(p, quality=90)

    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(one, [(c, t) for c in range(n_cams) for t in range(n_frames)]))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--src", default="2448x2048", help="source W x H")
    ap.add_argument("--canvas", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--pairs", type=int, default=128, help="pairs in the directory (8 cameras x pairs / 8 frames)")
    ap.add_argument("--threads", type=int, default=16, help="decode threads")
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--cpu-pairs", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lpips", nargs=2, metavar=("VGG16", "LIN"), default=None, help="the two LPIPS weight files: also time LPIPS")
    ap.add_argument("--lpips-pairs", type=int, default=8)
    args = ap.parse_args(argv)
    W, H = (int(v) for v in args.src.split("x"))
    cams, frames = 8, max(1, args.pairs // 8)
    with tempfile.TemporaryDirectory() as tmp:
        root = Path(tmp)
        t0 = time.perf_counter()
        write_results(root, W, H, cams, frames, 16)
        print(f"# {cams * frames} pairs {W}x{H} written in {time.perf_counter() - t0:.1f} s", flush=True)
        dirs = dict(pred_images_dir=str(root / "pred/images"), gt_images_dir=str(root / "gt"), fmasks_dir=str(root / "fmasks"),
                    pred_image_ext=".jpg", gt_image_ext=".webp", fmask_ext=".png", background_color="white")
        keys = metrics.evaluation_keys(dirs["pred_images_dir"])
        dev = torch.device("cuda", torch.cuda.current_device())
        ev = metrics.ImageEvaluator(dev, decode_threads=args.threads)
        batch = keys[: args.batch]
        pairs = [dict(pred=f"{dirs['pred_images_dir']}/{k}.jpg", gt=f"{dirs['gt_images_dir']}/{k}.webp", pred_fmask=f"{dirs['fmasks_dir']}/{k}.png",
                      gt_fmask=f"{dirs['fmasks_dir']}/{k}.png", canvas_size=args.canvas, crop_with_fmask=True, background_color="white")
                 for k in batch]
        t0 = time.perf_counter()
        items = list(ev._pool.map(lambda kw: ev._prepare(**kw), pairs))
        t_decode = time.perf_counter() - t0
        # the library call alone, on a batch that is already on the device
        times = []
        real = metrics.ops.eval_psnr_ssim

        def timed(*a, **k):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out = real(*a, **k)
            e.record()
            times.append((s, e))
            return out
        metrics.ops.eval_psnr_ssim = timed
        try:
            t_run = []
            for _ in range(args.reps + 1):  # the first call warms up (allocations, first launch)
                t0 = time.perf_counter()
                out, boxes, _ = ev._run(items, debug=False)
                t_run.append(time.perf_counter() - t0)
        finally:
            metrics.ops.eval_psnr_ssim = real
        torch.cuda.synchronize()
        t_kernel = min(s.elapsed_time(e) for s, e in times[1:]) / 1e3
        box = boxes[0].tolist()
        res = {"src": args.src, "canvas": args.canvas, "resized": list(metrics.resized_size(H, W, args.canvas)), "batch": len(batch),
               "crop_of_pair_0": box, "decode_s": round(t_decode, 3), "upload_and_kernel_s": round(min(t_run[1:]), 4),
               "kernel_s": round(t_kernel, 5), "kernel_us_per_pair": round(t_kernel / len(batch) * 1e6, 1)}
        print(json.dumps(res), flush=True)
        del items
        t0 = time.perf_counter()
        m = metrics.evaluate_results(gpu_ids=[dev.index], batch_size=args.batch, decode_threads=args.threads, canvas_size=args.canvas, **dirs)
        t_eval = time.perf_counter() - t0
        res.update({"evaluate_results_pairs": len(keys), "evaluate_results_s": round(t_eval, 3), "pairs_per_s": round(len(keys) / t_eval, 1),
                    "mean": m["mean"]})
        print(json.dumps({k: res[k] for k in ("evaluate_results_pairs", "evaluate_results_s", "pairs_per_s", "mean")}), flush=True)
        # the fp32 torch-CPU model, for scale
        import eval_model as em
        from PIL import Image
        torch.set_num_threads(args.cpu_threads)
        loaded = [{k: np.asarray(Image.open(v)) if k in ("pred", "gt", "pred_fmask", "gt_fmask") else v for k, v in kw.items()} for kw in pairs[: args.cpu_pairs]]
        t0 = time.perf_counter()
        cpu = [em.evaluate(dtype=torch.float32, **kw)[:2] for kw in loaded]
        t_cpu = (time.perf_counter() - t0) / len(loaded)
        res.update({"torch_cpu_fp32_threads": args.cpu_threads, "torch_cpu_fp32_s_per_pair": round(t_cpu, 3),
                    "torch_cpu_over_kernel": round(t_cpu / (t_kernel / len(batch)), 1),
                    "native_minus_cpu_pair_0": [float(out[0, 0]) - cpu[0][0], float(out[0, 1]) - cpu[0][1]]})
        print(json.dumps(res), flush=True)
        if args.lpips:
            print(json.dumps(lpips_report(dev, pairs[: args.lpips_pairs], args)))


def lpips_report(dev, pairs, args) -> dict:
    """Time per pair of evaluate_batch without and with LPIPS on the same pairs, and the event span of the LpipsVGG call alone (it
    contains the host-side gaps between its launches: an upper bound of the kernel time, not the kernel time)."""
    from diffuman4d_amd.host.lpips import LpipsVGG
    lp = LpipsVGG(dev, *args.lpips)
    events = []

    def timed_lp(gt, pred):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        v = lp(gt, pred)
        e.record()
        events.append((s, e, tuple(gt.shape[2:])))
        return v

    def wall(ev):
        best = float("inf")
        for _ in range(args.reps + 1):  # the first call warms up
            t0 = time.perf_counter()
            out = ev.evaluate_batch(pairs)
            best = min(best, time.perf_counter() - t0)
        return best / len(pairs), out

    t_plain, _ = wall(metrics.ImageEvaluator(dev, decode_threads=args.threads))
    t_lpips, out = wall(metrics.ImageEvaluator(dev, lpips=timed_lp, decode_threads=args.threads))
    torch.cuda.synchronize()
    per_pair = [min(s.elapsed_time(e) for s, e, _ in events[i + len(pairs):: len(pairs)]) for i in range(len(pairs))]  # without the warm-up round
    return {"lpips_pairs": len(pairs), "canvas": args.canvas, "crop_of_pair_0": list(events[0][2]),
            "psnr_ssim_only_ms_per_pair": round(t_plain * 1e3, 2), "with_lpips_ms_per_pair": round(t_lpips * 1e3, 2),
            "lpips_call_span_ms_per_pair": round(sum(per_pair) / len(per_pair), 2), "lpips_of_pair_0": out[0][2]}


if __name__ == "__main__":
    main()
