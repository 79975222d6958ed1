"""Micro-benchmark of the self-attention kernels by head dimension: ms and TFLOP/s (4 B H Lq Lk d per launch) for the SD-1.x layout's
head dimensions 40 / 80 / 160 (attention_hd.hip, 8 heads over 320 / 640 / 1280 channels) beside the SD-2.1 layout's head dimension 64
(attention.hip, 5 / 10 / 20 heads over the same channels) at the same token counts, in the three precisions.

    python tools/attn_hd_bench.py [--iters 20] [--batch 2]

Token counts per sequence are those of the judged window calls' 3-D attention (F = 16 / 24 frames at a 72 x 40 latent): 11 520 / 17 280
at 320 channels, 2 880 / 4 320 at 640, 720 / 1 080 at 1 280; `--batch` sequences per launch (2 = the CFG pair)."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

LEVELS = [(320, (11520, 17280)), (640, (2880, 4320)), (1280, (720, 1080))]


def _time(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def bench(C, L, heads, precision, batch, iters):
    from diffuman4d_amd.host import ops
    d = C // heads
    g = torch.Generator(device="cuda").manual_seed(0)
    M = batch * L
    if precision == "parity":
        qkv = (torch.randn(M, 6 * C, device="cuda", generator=g) * 0.5).to(torch.bfloat16)
        fn = lambda: ops.attention_split(qkv, batch, heads, L)  # noqa: E731
        flop = 3 * 4.0 * batch * heads * L * L * d
    else:
        dt = torch.float16 if precision == "fp16" else torch.bfloat16
        qkv = (torch.randn(M, 3 * C, device="cuda", generator=g) * 0.5).to(dt)
        out = torch.empty(M, C, dtype=dt, device="cuda")
        fn = lambda: ops.attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], batch, heads, L, out=out, q_scaled=True)  # noqa: E731
        flop = 4.0 * batch * heads * L * L * d
    ms = _time(fn, iters)
    return ms, flop / ms * 1e-9  # TFLOP/s (algorithmic: one MFMA term per product)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--json", default=None, help="also write the rows as JSON")
    a = ap.parse_args()
    rows = []
    print(f"{'C':>5} {'L':>6} {'layout':>7} {'heads':>5} {'d':>4} {'precision':>9} {'ms':>9} {'TFLOP/s':>8} {'x SD-2.1':>8}")
    for C, Ls in LEVELS:
        for L in Ls:
            for precision in ("fast", "fp16", "parity"):
                base = None
                for layout, heads in (("sd21", C // 64), ("sd1x", 8)):
                    ms, tf = bench(C, L, heads, precision, a.batch, a.iters)
                    base = ms if layout == "sd21" else base
                    rows.append(dict(C=C, L=L, layout=layout, heads=heads, d=C // heads, precision=precision, ms=ms, tflops=tf))
                    print(f"{C:>5} {L:>6} {layout:>7} {heads:>5} {C // heads:>4} {precision:>9} {ms:>9.3f} {tf:>8.1f} {ms / base:>8.2f}", flush=True)
    if a.json:
        Path(a.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
