#!/usr/bin/env python
"""The bit-exactness fixture of tests/test_ff_fused_bits_gpu.py: tests/golden/ff_fused_bits.json.  Needs the GPU.

  python tests/golden/make_golden_ff_fused.py      runs every case of CASES on the device and records, per case, the sha256 of the
                                                   input bytes and of every output tensor's bytes

The four launches of csrc/ff_fused.hip -- ff_fused_kernel, ff_proj_fused_kernel, ff_proj_fused_h16_kernel, l0_head_kernel -- with
their switches forced on, on seeded CPU inputs built the way tests/opcheck.py case_ff_fused / case_ff_proj_fused /
case_h16_ff_proj_fused and tests/test_l0_linear_fused.py::_head_inputs build theirs.  The other tests of these kernels compare them
with the launches they replace, to bounds (1.5e-3) that would not notice a changed summation order; this file pins the bits, so a
refactor of ff_fused.hip can be held to "nothing changed".  Record it with the library built from the commit BEFORE the change.
A change that really alters the order of a sum regenerates the file and says so.

Shapes (block tail and ff_fused_kernel): M = 300, hidden = 1280, biases -- two full 128-row tiles and a 44-row one whose clamped rows
m > M - 1 are fetched; M = 257, hidden = 64, no biases -- two hidden steps: the steady loop runs zero times, null bias pointers;
M = 129, hidden = 96 on row-strided views.  Head: M = 300 with bias, M = 257 without, M = 384 on a strided n and a strided qkv view
(the columns outside the view must stay untouched: asserted here, since a hash of the view cannot see them).
"""
from __future__ import annotations

import hashlib
import json
import math
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
OUT = Path(__file__).resolve().parent / "ff_fused_bits.json"
BF, F16 = torch.bfloat16, torch.float16
C = 320

SHAPES = {"m300_h1280": dict(M=300, hidden=1280, bias=True, strided=False, seed=11),
          "m257_h64_nobias": dict(M=257, hidden=64, bias=False, strided=False, seed=12),
          "m129_h96_strided": dict(M=129, hidden=96, bias=True, strided=True, seed=13)}
HEADS = {"m300": dict(M=300, bias=True, strided=False, seed=21), "m257_nobias": dict(M=257, bias=False, strided=False, seed=22),
         "m384_strided": dict(M=384, bias=True, strided=True, seed=23)}
# name -> (family, keyword arguments)
CASES = {}
for _s, _kw in SHAPES.items():
    CASES[f"ff_fused_{_s}"] = ("ff", dict(_kw, ln=False))
    CASES[f"ff_fused_ln_{_s}"] = ("ff", dict(_kw, ln=True))
    CASES[f"tail_bf16_{_s}"] = ("tail", _kw)
    CASES[f"tail_f16_{_s}"] = ("tail_f16", dict(_kw, out_f32=False))
    CASES[f"tail_f16_f32out_{_s}"] = ("tail_f16", dict(_kw, out_f32=True))
for _s, _kw in HEADS.items():
    CASES[f"head_{_s}"] = ("head", _kw)


def sha(*tensors) -> str:
    """sha256 over the bytes of the tensors (None: one zero byte), each as a contiguous host copy."""
    h = hashlib.sha256()
    for t in tensors:
        h.update(b"\0" if t is None else t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _rnd(shape, g, scale=1.0, dt=BF):
    return (torch.randn(shape, generator=g) * scale).to(dt)


def _dev(t):
    return None if t is None else t.to("cuda")


def _strided(nd, xd):
    """row-strided views (column slices of wider tensors), as the *_strided cases of tests/opcheck.py pass them"""
    return torch.cat([nd, nd], dim=1)[:, :C], torch.cat([xd, xd], dim=1)[:, C:]


class _Forced:
    """every switch of the fused launches on, ops.PROFILE a fresh list: `.launches` after the block"""

    def __enter__(self):
        from diffuman4d_amd.host import ops
        self.ops = ops
        self.old = {k: getattr(ops, k) for k in ("FF_FUSED", "FF_PROJ_FUSED", "L0_HEAD_FUSED", "PROFILE", "TRACE")}
        ops.FF_FUSED = ops.FF_PROJ_FUSED = ops.L0_HEAD_FUSED = True
        ops.PROFILE, ops.TRACE = [], None
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self.launches = len(self.ops.PROFILE)
        for k, v in self.old.items():
            setattr(self.ops, k, v)
        return False


def run_ff(M, hidden, bias, strided, seed, ln):
    """ops.FeedForward.__call__ (ff_fused_kernel), inputs as tests/opcheck.py case_ff_fused"""
    from diffuman4d_amd.host import ops
    g = torch.Generator().manual_seed(seed)
    n, x = _rnd((M, C), g), _rnd((M, C), g)
    w1, w2 = _rnd((2 * hidden, C), g, 1.0 / math.sqrt(C)), _rnd((C, hidden), g, 1.0 / math.sqrt(hidden))
    b1, b2 = (_rnd((2 * hidden,), g, 0.5), _rnd((C,), g, 0.5)) if bias else (None, None)
    gam, bet = (1.0 + 0.1 * torch.randn(C, generator=g)).to(BF), (0.1 * torch.randn(C, generator=g)).to(BF)
    ff = ops.FeedForward(_dev(w1), _dev(b1), _dev(w2), _dev(b2))
    assert ff.packed is not None, "fused feed-forward not built for this shape"
    nd, xd = _dev(n), _dev(x)
    if strided:
        nd, xd = _strided(nd, xd)
    with _Forced() as f:
        out = ff(nd, xd, ln=(_dev(gam), _dev(bet), 1e-5) if ln else None)
    return sha(n, x, w1, w2, b1, b2, gam, bet), {"out": out}, f.launches


def _tail_inputs(M, hidden, bias, seed, dt):
    g = torch.Generator().manual_seed(seed)
    a = _rnd((M, C), g, dt=dt)
    x = _rnd((M, C), g) if dt == BF else torch.randn(M, C, generator=g) * 2  # precision "fp16": the fp32 residual stream
    wo = _rnd((C, C), g, 1.0 / math.sqrt(C), dt)
    w1, w2 = _rnd((2 * hidden, C), g, 1.0 / math.sqrt(C), dt), _rnd((C, hidden), g, 1.0 / math.sqrt(hidden), dt)
    bo, b1, b2 = (_rnd((C,), g, 0.5, dt), _rnd((2 * hidden,), g, 0.5, dt), _rnd((C,), g, 0.5, dt)) if bias else (None, None, None)
    gam, bet = (1.0 + 0.1 * torch.randn(C, generator=g)).to(dt), (0.1 * torch.randn(C, generator=g)).to(dt)
    return a, x, wo, w1, w2, bo, b1, b2, gam, bet


def run_tail(M, hidden, bias, strided, seed, out_f32=None):
    """FeedForward.after_attention (ff_proj_fused_kernel) or, with out_f32 given, after_attention_f16 (ff_proj_fused_h16_kernel);
    inputs as tests/opcheck.py case_ff_proj_fused / case_h16_ff_proj_fused"""
    from diffuman4d_amd.host import ops
    h16 = out_f32 is not None
    inp = _tail_inputs(M, hidden, bias, seed, F16 if h16 else BF)
    a, x, wo, w1, w2, bo, b1, b2, gam, bet = inp
    ff = ops.FeedForward(_dev(w1), _dev(b1), _dev(w2), _dev(b2))
    assert ff.packed is not None, "fused feed-forward not built for this shape"
    ad, xd = _dev(a), _dev(x)
    if strided:
        ad, xd = _strided(ad, xd)
    lnp = (_dev(gam), _dev(bet), 1e-5)
    with _Forced() as f:
        if h16:
            out = ff.after_attention_f16(ad, _dev(wo), _dev(bo), xd, lnp, out_f32)
        else:
            out = ff.after_attention(ad, _dev(wo), _dev(bo), xd, lnp)
    assert out.dtype == ((torch.float32 if out_f32 else F16) if h16 else BF) and out.shape == (M, C)
    return sha(*inp), {"out": out}, f.launches


def run_head(M, bias, strided, seed):
    """ops.proj_in_ln_qkv (l0_head_kernel), inputs as tests/test_l0_linear_fused.py::_head_inputs"""
    from diffuman4d_amd.host import ops
    g = torch.Generator().manual_seed(seed)
    n = _rnd((M, C), g)
    wpi, wqkv = _rnd((C, C), g, 1.0 / math.sqrt(C)), _rnd((3 * C, C), g, 1.0 / math.sqrt(C))
    bpi = _rnd((C,), g, 0.5) if bias else None
    gam, bet = (1.0 + 0.1 * torch.randn(C, generator=g)).to(BF), (0.1 * torch.randn(C, generator=g)).to(BF)
    nd, view, wide_q = _dev(n), None, None
    if strided:  # column views of wider tensors
        wide = torch.full((M, C + 16), 7.0, dtype=BF, device="cuda")
        wide[:, 8:8 + C] = nd
        nd = wide[:, 8:8 + C]
        wide_q = torch.full((M, 3 * C + 16), 5.0, dtype=BF, device="cuda")
        view = wide_q[:, 8:8 + 3 * C]
    with _Forced() as f:
        h, qkv = ops.proj_in_ln_qkv(nd, _dev(wpi), _dev(bpi), (_dev(gam), _dev(bet), 1e-5), _dev(wqkv), qkv=view)
    if strided:
        assert qkv.data_ptr() == view.data_ptr()
        assert bool((wide_q[:, :8] == 5.0).all()) and bool((wide_q[:, 8 + 3 * C:] == 5.0).all()), "columns outside the qkv view were written"
    return sha(n, wpi, wqkv, bpi, gam, bet), {"h": h, "qkv": qkv}, f.launches


RUN = {"ff": run_ff, "tail": run_tail, "tail_f16": run_tail, "head": run_head}


def run_case(name):
    """-> {"inputs": sha256, "outputs": {tensor name: sha256}}, number of launches the call took"""
    family, kw = CASES[name]
    inputs, outs, launches = RUN[family](**kw)
    return {"inputs": inputs, "outputs": {k: sha(v) for k, v in outs.items()}}, launches


def main() -> None:
    rec = {}
    for name in CASES:
        rec[name], launches = run_case(name)
        assert launches == 1, f"{name}: {launches} launches -- the fused kernel was not used"
        print(name, rec[name]["outputs"])
    OUT.write_text(json.dumps({"device": torch.cuda.get_device_name(0), "cases": rec}, indent=1) + "\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
