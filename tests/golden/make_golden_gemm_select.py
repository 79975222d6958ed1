#!/usr/bin/env python
"""Input grid of the tile-selection table (tests/golden/gemm_select_table.txt, read by tests/test_gemm_select_cpu.py).

    python tests/golden/make_golden_gemm_select.py            prints the input lines
    python tests/golden/make_golden_gemm_select.py --write    rewrites the table: inputs from here, the expected column from
                                                              tests/gemm_select_probe.cpp (compiled with the host compiler)

This script builds the INPUTS only.  The expected column of the committed table was first produced by the selection code as it stood
before csrc/gemm_select.h existed (a host harness around the functions of gemm.hip), so the table pins the heuristic and not the
header's reading of it.  `--write` is for a later, intentional retune: the change then shows up as a diff of the table.

Line formats (every number an integer):
    g M N K K1 geglu                 a Linear layer; K1 > 0 = split A (skip concat): A holds K1 columns, A2 the other K - K1
    c B H W Cin Cout stride up       a 3x3 convolution, pad 1; up = fused nearest-x2 upsample
    u B H W Cin Cout                 the phase-decomposed x2 upsampling convolution
"""
from __future__ import annotations

import subprocess
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
TABLE = HERE / "gemm_select_table.txt"
PROBE_SRC = ROOT / "tests" / "gemm_select_probe.cpp"

LATENTS = [(72, 40), (128, 72), (16, 8)]
CHANNELS = [320, 640, 1280, 1280]
BATCHES = [1, 2, 4, 8, 16, 24, 32, 48, 64, 96]
# tools/gemm_tune.py vae(): the SD VAE's stride-1 convolutions (H, W, Cin, Cout)
VAE = [(576, 320, 128, 128), (288, 160, 128, 256), (288, 160, 256, 256), (144, 80, 256, 512), (144, 80, 512, 512), (72, 40, 512, 512),
       (576, 320, 256, 128), (288, 160, 512, 256)]


def inputs() -> list[str]:
    out: list[str] = []

    def g(M, N, K, K1=0, geglu=0):
        out.append(f"g {M} {N} {K} {K1} {geglu}")

    def c(B, H, W, Cin, Cout, stride=1, up=0):
        out.append(f"c {B} {H} {W} {Cin} {Cout} {stride} {up}")

    def u(B, H, W, Cin, Cout):
        out.append(f"u {B} {H} {W} {Cin} {Cout}")

    # UNet levels
    for (h0, w0) in LATENTS:
        for lvl, ch in enumerate(CHANNELS):
            h, w = max(h0 >> lvl, 1), max(w0 >> lvl, 1)
            prev = CHANNELS[max(lvl - 1, 0)]
            for B in BATCHES:
                M = B * h * w
                g(M, ch, ch)                    # proj_in / attention output / proj_out
                g(M, 3 * ch, ch)                # fused QKV
                g(M, 4 * ch, ch, geglu=1)       # GEGLU ff1
                g(M, ch, 4 * ch)                # ff2
                g(M, ch, 1024)                  # cross-attention projection of the K = 1024 context, per pixel row
                g(B * 77, 2 * ch, 1024)         # fused K / V projection of the context tokens
                g(M, ch, ch + prev, K1=ch)      # split-A skip concat
                for cin in (ch, ch + ch // 2, 2 * ch, 3 * ch):
                    c(B, h, w, cin, ch)
                c(B, h, w, prev, ch)            # first convolution of a down level
                c(B, h, w, ch, ch, stride=2)    # Downsample2D
                c(B, h, w, ch, ch, up=1)        # Upsample2D, gather form
                u(B, h, w, ch, ch)              # Upsample2D, phase form
    # VAE
    for (h, w, ci, co) in VAE:
        for B in (1, 2, 4, 8):
            c(B, h, w, ci, co)
        c(8, h, w, ci, co, up=1)
        u(8, h, w, ci, co)
    # lattice of small and odd Linear shapes (K = 32, 96, 160: no K-slab of 64)
    for K in (32, 96, 160, 320):
        for N in (32, 64, 96, 320, 512, 1280, 2560):
            for M in (1, 17, 128, 1000, 4096, 20000, 65536, 200000):
                g(M, N, K)
                g(M, N, K, geglu=1)
    # lattice of small and odd convolutions (Cin = 32, 96: no K-slab of 64)
    for cin in (32, 64, 96, 320):
        for cout in (32, 64, 96, 320, 512, 1280):
            for (B, h, w) in ((1, 8, 8), (1, 9, 5), (2, 33, 17), (4, 64, 64), (16, 128, 72)):
                c(B, h, w, cin, cout)
                c(B, h, w, cin, cout, stride=2)
                c(B, h, w, cin, cout, up=1)
    for cout in (8, 64, 72, 200, 384):
        for B in (1, 16, 96):
            u(B, 36, 20, 64, cout)
    # the split rows away from the UNet's own channel counts: H * W <= 64 and Cin >= 512, and their neighbours
    for (h, w) in ((8, 8), (9, 7), (13, 5)):
        for cin in (448, 512, 1024):
            for cout in (512, 516, 1280):
                c(4, h, w, cin, cout)
    # wide, tall problems: 256x256 pipe tiles of the gather kernels, 64-wide tiles on many rows
    for B in (32, 96):
        c(B, 72, 40, 256, 512, stride=2)
        c(B, 128, 72, 256, 512, stride=2)
        c(B, 36, 20, 1280, 1280, up=1)
        c(B, 72, 40, 640, 640, up=1)
        c(B, 72, 40, 320, 192)
        c(B, 72, 40, 320, 192, stride=2)
        g(B * 2880, 192, 320)
        g(B * 2880, 960, 320)
    # operands of 4 GiB or more: the 32-bit-offset kernels (second form, strips) must not be chosen
    for N, geglu in ((320, 0), (1280, 0), (640, 0), (1280, 1)):
        g(8000000, N, 320, geglu=geglu)
        g(8000000, N, 1280, geglu=geglu)
        g(8000000, N, 2560, geglu=geglu)
    g(8000000, 320, 640, K1=320)
    g(4000000, 320, 960, K1=320)
    g(4096, 65536, 16384)
    g(4096, 65536, 16384, geglu=1)
    for cout in (128, 256, 320, 640):
        c(96, 576, 320, 256, cout)
        c(96, 576, 320, 256, cout, up=1)
        u(96, 576, 320, 256, cout)
    c(1, 8, 8, 65536, 8192)
    return list(dict.fromkeys(out))  # levels share some shapes (context projections, the two 1280-channel levels): one line each


def run_probe(lines: list[str], exe: Path | None = None) -> list[str]:
    """Compile tests/gemm_select_probe.cpp with the host compiler (unless `exe` is given) and run it over `lines`."""
    with tempfile.TemporaryDirectory() as tmp:
        if exe is None:
            exe = Path(tmp) / "gemm_select_probe"
            subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{ROOT / 'include'}", f"-I{ROOT / 'diffuman4d_amd' / 'csrc'}",
                            str(PROBE_SRC), "-o", str(exe)], check=True)
        res = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    return res.stdout.splitlines()


HEADER = """\
# Tile selection of csrc/gemm_select.h over the grid of tests/golden/make_golden_gemm_select.py: `input | expected`.
# g M N K K1 geglu           | fast par f16                        (id/splits; par: `unsupported` where the precision has no kernel)
# c B H W Cin Cout stride up | fast fast_ws ws_bytes par_ws f16 f16_ws   (_ws: with the workspace of ws_bytes, else without one)
# u B H W Cin Cout           | tile
"""


if __name__ == "__main__":
    if "--write" in sys.argv:
        TABLE.write_text(HEADER + "\n".join(run_probe(inputs())) + "\n")
        print(TABLE)
    else:
        print("\n".join(inputs()))
