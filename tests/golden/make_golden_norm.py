#!/usr/bin/env python
"""The bit-exactness fixture of tests/test_norm_bits_gpu.py: tests/golden/norm_bits.json.  Needs the GPU.

  python tests/golden/make_golden_norm.py      runs every case of CASES on the device and records, per case, the sha256 of the
                                               input bytes and of every output tensor's bytes

Every kernel of csrc/norm.hip -- GroupNorm (single-launch, two-launch, fp64 general), LayerNorm (register rows, general) and the
three row softmaxes -- in every instantiation and on both sides of every size at which the code takes another path, on seeded CPU
inputs, through host/ops.py (the two *_general entries that a multiple-of-8 channel count cannot reach: through lib.call).  The
opcheck cases compare these kernels with fp64 references to bounds that would not notice a changed summation order; this file pins
the bits, so a refactor of norm.hip can be held to "nothing changed".  Record it with the library built from the commit BEFORE the
change.  A change that really alters the order of a sum regenerates the file and says so.
The file in the tree was recorded with the library built from commit 97f62cf, the parent of the commit that moved the family into
one file (norm.hip 704 lines, parity.hip 781), before any kernel source was touched, and has not been regenerated since.

Fast GroupNorm: a case is one shape, run in four forms (outputs `bf16`, `f32_f16`, `f32_f16_raw` + `raw`, `f16_f16`: bf16 in and
out; fp32 in, fp16 out; the same with the second, un-normalised output; fp16 in and out).  The single-launch kernel has one case per
register bucket (C = 640, 32 groups: slabs of 5 vectors x 51 pixels, HW = 45 / 180 / 360 / 720 -> 1 / 4 / 8 / 15 pixels per thread),
B % 8 == 0 (the XCD map) and not, and a two-source shape whose slabs straddle C1 and whose vectors span two groups.  The two-launch
pair is forced with dm4d_tune_set_groupnorm_resident(0) on that shape, on one with 320 vectors (one pixel per pass), on groups
of 2 and 6 channels (more than one group per vector), and runs by itself at HW = 821 (17 pixels per thread: past the resident limit;
an odd count for the unrolled loops' tails).  One shape has its mean 200 standard deviations out, so the shift enters the bits.
fp64 GroupNorm: four and one channel per thread, one and two sources, both outputs (`split`, `f16`).
"""
from __future__ import annotations

import hashlib
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
OUT = Path(__file__).resolve().parent / "norm_bits.json"
BF, F16 = torch.bfloat16, torch.float16

# name -> (family, keyword arguments)
CASES = {
    # single-launch kernel: NV buckets 2, 4, 8, 16
    "gn_res_nv2_b8": ("gn", dict(B=8, HW=45, C1=640, silu=True, eps=1e-5, seed=1)),
    "gn_res_nv4_b3": ("gn", dict(B=3, HW=180, C1=640, silu=False, eps=1e-6, seed=2)),
    "gn_res_nv8_b2": ("gn", dict(B=2, HW=360, C1=640, silu=True, eps=1e-6, seed=3)),
    "gn_res_nv16_b8": ("gn", dict(B=8, HW=720, C1=640, silu=False, eps=1e-5, seed=4)),
    "gn_res_straddle": ("gn", dict(B=3, HW=180, C1=1280, C2=640, silu=True, eps=1e-5, seed=5)),
    "gn_res_mean_200sigma": ("gn", dict(B=2, HW=512, C1=64, groups=8, silu=False, eps=1e-5, offset=400.0, seed=6)),
    # statistics + apply pair
    "gn_two_straddle": ("gn", dict(B=3, HW=180, C1=1280, C2=640, silu=True, eps=1e-5, seed=5, resident=0)),
    "gn_two_cv320": ("gn", dict(B=2, HW=45, C1=1280, C2=1280, silu=False, eps=1e-6, seed=7, resident=0)),
    "gn_two_gs2": ("gn", dict(B=5, HW=100, C1=64, silu=True, eps=1e-6, seed=8, resident=0)),
    "gn_two_gs6_two_sources": ("gn", dict(B=5, HW=50, C1=128, C2=64, silu=False, eps=1e-5, seed=9, resident=0)),
    "gn_two_natural_hw821": ("gn", dict(B=3, HW=821, C1=320, silu=True, eps=1e-5, seed=10)),
    "gn_two_mean_200sigma": ("gn", dict(B=2, HW=512, C1=64, groups=8, silu=True, eps=1e-5, offset=400.0, seed=6, resident=0)),
    # fp64 statistics: W = 4 (one source; two sources, Q >= 256; through the fp16 entry's fall-back), W = 1 (one and two sources)
    "gn32_w4": ("gn32", dict(B=3, HW=720, C1=320, silu=True, eps=1e-5, seed=11)),
    "gn32_w4_two_sources": ("gn32", dict(B=2, HW=45, C1=1280, C2=640, silu=False, eps=1e-6, seed=12)),
    "gn32_w4_c132": ("gn32", dict(B=2, HW=77, C1=132, groups=6, silu=True, eps=1e-5, seed=13)),
    "gn32_w4_c68_c28": ("gn32", dict(B=2, HW=77, C1=68, C2=28, groups=6, silu=False, eps=1e-5, seed=14)),
    "gn32_w1": ("gn32", dict(B=2, HW=77, C1=66, groups=6, silu=True, eps=1e-5, seed=15)),
    "gn32_w1_two_sources": ("gn32", dict(B=2, HW=77, C1=66, C2=30, groups=6, silu=False, eps=1e-6, seed=16)),
    # LayerNorm: ln_kernel<NV = 1, 1, 2, 3, 4, 4, 8> in bf16 and fp32 -> fp16, M % 4 != 0; a strided view; the general kernel
    **{f"ln_c{c}": ("ln", dict(M=37, C=c, seed=20 + i)) for i, c in enumerate((64, 320, 640, 1280, 1600, 2048, 2560))},
    "ln_c320_strided": ("ln", dict(M=37, C=320, seed=30, strided=True)),
    "ln32_c320": ("ln32", dict(M=37, C=320, seed=31)),
    "ln32_c100": ("ln32", dict(M=37, C=100, seed=32)),
    # row softmax
    "softmax_bf16": ("softmax", dict(M=5, N=300, seed=40)),
    "softmax_f32_n301": ("softmax_f32", dict(M=5, N=301, Np=320, seed=41)),
    "softmax_f32_n256": ("softmax_f32", dict(M=5, N=256, Np=256, seed=42)),
    "softmax32_split": ("softmax32", dict(M=5, N=301, Np=320, seed=43)),
}


def sha(*tensors) -> str:
    """sha256 over the bytes of the tensors (None: one zero byte), each as a contiguous host copy."""
    h = hashlib.sha256()
    for t in tensors:
        h.update(b"\0" if t is None else t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _dev(t, dt=None):
    return None if t is None else (t if dt is None else t.to(dt)).to("cuda")


def _gn_inputs(B, HW, C1, C2, seed, offset):
    g = torch.Generator().manual_seed(seed)
    x1 = torch.randn(B, HW, C1, generator=g) * 2 + offset
    x2 = torch.randn(B, HW, C2, generator=g) - 0.25 if C2 else None
    gam, bet = 1.0 + 0.1 * torch.randn(C1 + C2, generator=g), 0.1 * torch.randn(C1 + C2, generator=g)
    return x1, x2, gam, bet


def run_gn(B, HW, C1, silu, eps, seed, C2=0, groups=32, offset=0.5, resident=1):
    """the fast GroupNorm kernels in their four input / output forms; resident=0 forces the statistics + apply pair"""
    from diffuman4d_amd.host import lib, ops
    x1, x2, gam, bet = _gn_inputs(B, HW, C1, C2, seed, offset)
    outs = {}
    lib.load().dm4d_tune_set_groupnorm_resident(resident)
    try:
        for name, xdt, pdt, raw in (("bf16", BF, BF, False), ("f32_f16", None, F16, False), ("f32_f16_raw", None, F16, True),
                                    ("f16_f16", F16, F16, False)):
            y = ops.groupnorm(_dev(x1, xdt), _dev(gam, pdt), _dev(bet, pdt), groups, eps, x2=_dev(x2, xdt), silu=silu, raw_out=raw)
            if raw:
                y, outs["raw"] = y
            outs[name] = y
    finally:
        lib.load().dm4d_tune_set_groupnorm_resident(1)
    return sha(x1, x2, gam, bet), outs


def run_gn32(B, HW, C1, silu, eps, seed, C2=0, groups=32):
    """the fp64-statistics GroupNorm: the parity operand out (`split`) and one fp16 plane out (`f16`; channel counts that are
    multiples of 8 would take the fast kernels in ops.groupnorm: those call dm4d_groupnorm_f32_f16_general themselves)"""
    from diffuman4d_amd.host import lib, ops
    x1, x2, gam, bet = _gn_inputs(B, HW, C1, C2, seed, 0.5)
    d1, d2 = _dev(x1), _dev(x2)
    outs = {"split": ops.groupnorm(d1, _dev(gam, BF), _dev(bet, BF), groups, eps, x2=d2, silu=silu)}
    gh, bh = _dev(gam, F16), _dev(bet, F16)
    if C1 % 8 or C2 % 8:
        outs["f16"] = ops.groupnorm(d1, gh, bh, groups, eps, x2=d2, silu=silu)
    else:
        y = torch.empty((B, HW, C1 + C2), dtype=F16, device="cuda")
        ws = torch.empty(lib.load().dm4d_groupnorm_f32_ws_bytes(B, HW, groups) // 8, dtype=torch.float64, device="cuda")
        lib.call("dm4d_groupnorm_f32_f16_general", torch.cuda.current_stream().cuda_stream, d1.data_ptr(), C1,
                 None if d2 is None else d2.data_ptr(), C2, B, HW, groups, eps, gh.data_ptr(), bh.data_ptr(), y.data_ptr(), 1 if silu else 0,
                 ws.data_ptr())
        outs["f16"] = y
    assert outs["split"].shape[-1] == 2 * (C1 + C2) and outs["f16"].shape[-1] == C1 + C2
    return sha(x1, x2, gam, bet), outs


def _ln_inputs(M, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, C, generator=g) * 3 + 0.5
    return x, 1.0 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)


def run_ln(M, C, seed, strided=False):
    """ln_kernel: bf16 rows, and fp32 rows -> one fp16 plane; strided: the rows are a column slice of a wider tensor"""
    from diffuman4d_amd.host import ops
    x, gam, bet = _ln_inputs(M, C, seed)
    xb, xf = _dev(x, BF), _dev(x)
    if strided:
        xb, xf = torch.cat([xb, xb], dim=1)[:, C:], torch.cat([xf, xf], dim=1)[:, C:]
        assert xb.stride(0) == 2 * C
    outs = {"bf16": ops.layernorm(xb, _dev(gam, BF), _dev(bet, BF), 1e-5), "f32_f16": ops.layernorm(xf, _dev(gam, F16), _dev(bet, F16), 1e-5)}
    return sha(x, gam, bet), outs


def run_ln32(M, C, seed):
    """ln32_kernel: the parity operand out and, where C % 8 != 0 sends the fp16 entry there, one fp16 plane out"""
    from diffuman4d_amd.host import ops
    x, gam, bet = _ln_inputs(M, C, seed)
    outs = {"split": ops.layernorm(_dev(x), _dev(gam, BF), _dev(bet, BF), 1e-5)}
    if C % 8:
        outs["f16"] = ops.layernorm(_dev(x), _dev(gam, F16), _dev(bet, F16), 1e-5)
    return sha(x, gam, bet), outs


def _logits(M, Np, seed):
    return torch.randn(M, Np, generator=torch.Generator().manual_seed(seed)) * 40


def run_softmax(M, N, seed):
    from diffuman4d_amd.host import ops
    s = _logits(M, N, seed).to(BF)
    return sha(s), {"p": ops.softmax_rows(_dev(s), 0.05)}


def run_softmax_f32(M, N, Np, seed):
    """softmax_rows_f32_kernel over the first N of Np columns; the columns behind N keep the caller's zeros"""
    from diffuman4d_amd.host import ops
    s = _logits(M, Np, seed)
    p = ops.softmax_rows(_dev(s), 0.05, n=N, out=torch.zeros((M, Np), dtype=BF, device="cuda"))
    return sha(s), {"p": p}


def run_softmax32(M, N, Np, seed):
    """softmax32_split_kernel both ways: three planes [hi | lo | hi], and one fp16 plane; padded columns included"""
    from diffuman4d_amd.host import ops
    s = _logits(M, Np, seed)
    return sha(s), {"split": ops.softmax_rows_split(_dev(s), 0.05, n=N), "f16": ops.softmax_rows_split(_dev(s), 0.05, n=N, h16=True)}


RUN = {"gn": run_gn, "gn32": run_gn32, "ln": run_ln, "ln32": run_ln32, "softmax": run_softmax, "softmax_f32": run_softmax_f32,
       "softmax32": run_softmax32}


def run_case(name):
    """-> {"inputs": sha256, "outputs": {tensor name: sha256}}"""
    family, kw = CASES[name]
    inputs, outs = RUN[family](**kw)
    torch.cuda.synchronize()
    return {"inputs": inputs, "outputs": {k: sha(v) for k, v in outs.items()}}


def main() -> None:
    rec = {}
    for name in CASES:
        rec[name] = run_case(name)
        print(name, rec[name]["outputs"])
    OUT.write_text(json.dumps({"device": torch.cuda.get_device_name(0), "cases": rec}, indent=1) + "\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
