"""Tensor-level wrappers over the C ABI (torch is only the allocator / stream provider here).

Every function requires tensors resident on a HIP device and launches on torch's current
stream.  Nothing here computes with torch: a tensor on the CPU is an error, not a fallback.

Three arithmetics share these wrappers (include/dm4d.h, "Parity precision" / "fp16 precision"):
  * fast (default): bf16 tensors between kernels, bf16 MFMA operands, fp32 accumulation;
  * parity (``precision="parity"`` on the model objects): fp32 tensors between kernels; every activation that feeds the
    matrix unit is a two-term OPERAND ``[hi(C) | lo(C)]`` (bf16, 2 C columns) against weights duplicated along K
    (``dup_k``);
  * fp16 (``precision="fp16"``): fp32 tensors between kernels; every activation that feeds the matrix unit is ONE fp16 plane
    against fp16 weights (one MFMA per product, as in the fast precision).
Functions that exist in several forms dispatch on the dtypes they are given: an fp32 activation means a wide (parity / fp16)
precision, and fp16 weights / norm parameters / operands mean the fp16 one.
"""
from __future__ import annotations

import os

from typing import Optional, Tuple

import torch

from . import lib as _l
from .codec import workspace as _workspace
from .lib import (CAPTURE_CELL_FIELDS, CAPTURE_FIELDS, EVAL_BG_SHIFT, EVAL_CROP_MASKS, EVAL_FIELDS, EVAL_IMAGE_F32, EVAL_MASK_F32, EVAL_OUT,  # noqa: F401
                  LOG2E, LPIPS_IN_COLS, LPIPS_TAPS, ROWS_MOVE_MAX_JOBS, SKEL_CIRCLE, SKEL_COORD_MAX, SKEL_COORD_MIN, SKEL_FIELDS, SKEL_LINE, SKEL_LINK_FIELDS,
                  SKEL_MAX_KPTS, SKEL_MAX_PRIMS, SKEL_MAX_SIZE, SKEL_ST_LINK_SHIFT, SKEL_ST_NOCOLOR, SKEL_ST_NONFINITE,
                  TRIANG_MAX_VIEWS, VHULL_BLOCK, VHULL_MAX_CHUNK)

BF16 = torch.bfloat16
F16 = torch.float16
F32 = torch.float32


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


# tests/modelcheck.py (the *_opreplay cases) sets this to a list: every fast-precision launch then appends (operator name, its
# inputs as a dict of tensors / scalars, its output tensor), so that each launch of a real model call can be recomputed on the CPU
# from the very tensors the device was given (oracle/replay.py).  None = no tracing.  The tensors are kept alive by the list.
TRACE = None


def _trace(name: str, out, **inputs) -> None:
    if TRACE is not None:
        TRACE.append((name, inputs, out))


def _req(t: torch.Tensor, name: str, dtype=BF16):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _l.Dm4dError(f"{name}: expected a tensor on a HIP device (no CPU fallback in diffuman4d_amd)")
    if t.dtype != dtype:
        raise _l.Dm4dError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if t.stride(-1) != 1 and t.shape[-1] != 1:  # the stride of a dimension of size 1 says nothing
        raise _l.Dm4dError(f"{name}: last dim must be contiguous")
    return t


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _check_meta(meta: torch.Tensor, meta_host: torch.Tensor, fields: int, rows: int, desc_off: int, tab_off: Optional[int] = None,
                tab_len: Optional[int] = None, what: str = "meta") -> None:
    """`meta_host` is the host copy of the device bytes `meta` (named `what` in the refusals), and the `rows` int64 descriptors of
    `fields` fields at byte `desc_off` -- with `tab_off`, also the `tab_len` int32 table entries at that byte -- lie inside it, aligned."""
    if meta_host.device.type != "cpu" or meta_host.dtype != torch.uint8 or meta_host.numel() != meta.numel() or \
            not meta_host.is_contiguous() or not meta.is_contiguous():
        raise _l.Dm4dError(f"{what}: expected a contiguous uint8 tensor and its contiguous host copy")
    if rows < 1 or desc_off < 0 or desc_off % 8 or desc_off + rows * fields * 8 > meta.numel():
        raise _l.Dm4dError(f"desc_off: the descriptors lie outside {what}, or are not aligned")
    if tab_off is not None and (tab_off < 0 or tab_off % 4 or tab_len < 1 or tab_off + tab_len * 4 > meta.numel()):
        raise _l.Dm4dError(f"tab_off: the tables lie outside {what}, or are not aligned")


def gemm(a: torch.Tensor, w: torch.Tensor, *, a2: Optional[torch.Tensor] = None, bias=None, rowbias=None,
         rows_per_rowbias: int = 1, residual=None, geglu: bool = False, silu: bool = False, out_scale: float = 1.0,
         out: Optional[torch.Tensor] = None, out_f32: bool = False, split_out: bool = False, scale_cols: int = 0,
         col_scale: float = 1.0) -> torch.Tensor:
    """out[M,N] = epi([a | a2] @ w^T); a [M,K1], a2 [M,K-K1], w [N,K] (GEGLU: [2N,K]).
    out_f32: the result is stored unrounded in an fp32 tensor (attention logits of the VAE mid block; wide precisions).
    split_out (wide precisions): the result leaves as the OPERAND of the next contraction -- parity: bf16 [M, 2N] = [hi | lo];
    fp16 (w is fp16): one fp16 plane [M, N].
    rowbias / residual may be fp32 tensors (wide precisions: both must then be fp32).
    scale_cols / col_scale (fp16 precision): output columns [0, scale_cols) are multiplied by col_scale before the one rounding."""
    h16 = isinstance(w, torch.Tensor) and w.dtype == F16  # precision "fp16": fp16 a / a2 / w / bias, fp16 (or fp32) result
    dt = F16 if h16 else BF16
    assert h16 or scale_cols == 0
    _req(a, "a", dt), _req(w, "w", dt)
    M, K1 = a.shape
    K = w.shape[1]
    N = w.shape[0] // 2 if geglu else w.shape[0]
    if a2 is not None:
        _req(a2, "a2", dt)
        assert a2.shape[0] == M and K1 + a2.shape[1] == K
    else:
        assert K1 == K, (K1, K)
    if bias is not None:
        _req(bias, "bias", dt)
    side = [t for t in (rowbias, residual) if t is not None]
    f32_side = bool(side) and side[0].dtype == F32
    for t, n in ((rowbias, "rowbias"), (residual, "residual")):
        if t is not None:
            _req(t, n, F32 if f32_side else dt)
    split_out = split_out and not h16  # the fp16 operand is the one plane this entry stores anyway
    assert not (out_f32 and split_out)
    odt, ocols = (F32 if out_f32 else dt), (2 * N if split_out else N)
    if out is None:
        out = torch.empty((M, ocols), dtype=odt, device=a.device)
    _req(out, "out", odt)
    assert out.shape[1] >= ocols or out.stride(0) >= ocols
    flags = ((_l.EPI_GEGLU if geglu else 0) | (_l.EPI_SILU if silu else 0) | (_l.EPI_F32OUT if out_f32 else 0)
             | (_l.EPI_F32SIDE if f32_side else 0) | (_l.EPI_SPLITOUT if split_out else 0))
    args = (_stream(), _p(a), a.stride(0), _p(a2), a2.stride(0) if a2 is not None else 0, K1 if a2 is not None else 0, _p(w), w.stride(0),
            _p(out), out.stride(0), M, N, K, _p(bias), _p(rowbias), rowbias.stride(0) if rowbias is not None else 0, rows_per_rowbias,
            _p(residual), residual.stride(0) if residual is not None else 0, flags, out_scale)
    with _Prof("linear", 2.0 * M * w.shape[0] * K, "flop", M):
        if h16:
            _l.call("dm4d_gemm_f16", *args, int(scale_cols), float(col_scale))
        else:
            _l.call("dm4d_gemm_bf16", *args)
    if not h16:
        _trace("gemm", out, a=a, w=w, a2=a2, bias=bias, rowbias=rowbias, rows_per_rowbias=rows_per_rowbias, residual=residual, geglu=geglu,
               silu=silu, out_scale=out_scale, out_f32=out_f32, split_out=split_out)
    return out


def conv_out_hw(h: int, w: int, stride: int, pad: int, upsample: bool, pad_hi: Optional[int] = None) -> Tuple[int, int]:
    if upsample:
        return 2 * h, 2 * w
    ph = pad if pad_hi is None else pad_hi
    return (h + pad + ph - 3) // stride + 1, (w + pad + ph - 3) // stride + 1


def conv3x3(x: torch.Tensor, wt: torch.Tensor, *, bias=None, rowbias=None, residual=None, stride: int = 1,
            pad: int = 1, pad_hi: Optional[int] = None, upsample: bool = False, out_scale: float = 1.0,
            out_f32: bool = False) -> torch.Tensor:
    """x [B,H,W,Cin] NHWC, wt [Cout, 9*Cin] ((ky,kx,ci) order) -> [B,Ho,Wo,Cout].
    out_f32 (wide precisions): fp32 output; rowbias / residual must then be fp32 as well (in the parity precision x is usually a two-term
    operand and wt duplicated along Cin, which this function does not need to know).
    fp16 x / wt / bias (precision "fp16"): rowbias / residual fp32 or fp16; an fp16 result may take an fp32 row bias (conv1 of a resnet,
    whose fp32 sum is rounded once for norm2)."""
    lib = _l.load()
    h16 = isinstance(wt, torch.Tensor) and wt.dtype == F16
    dt = F16 if h16 else BF16
    _req(x, "x", dt), _req(wt, "wt", dt)
    assert x.is_contiguous() and wt.is_contiguous()
    B, H, W, Cin = x.shape
    Cout = wt.shape[0]
    assert wt.shape[1] == 9 * Cin, (wt.shape, Cin)
    Ho, Wo = conv_out_hw(H, W, stride, pad, upsample, pad_hi)
    y = torch.empty((B, Ho, Wo, Cout), dtype=F32 if out_f32 else dt, device=x.device)
    sides = [t for t in (rowbias, residual) if t is not None]
    side = F32 if (out_f32 or (h16 and sides and sides[0].dtype == F32)) else dt
    if h16 and bias is not None:  # (a bf16 bias has always been taken as it comes)
        _req(bias, "bias", F16)
    if residual is not None:
        _req(residual, "residual", side)
        assert residual.numel() == y.numel() and residual.is_contiguous()
    if rowbias is not None:
        _req(rowbias, "rowbias", side)
        assert rowbias.shape[0] == B
    up = 1 if upsample else 0
    args = (_stream(), _p(x), B, H, W, Cin, _p(wt), _p(y), Ho, Wo, Cout, stride, pad, up, _p(bias), _p(rowbias),
            rowbias.stride(0) if rowbias is not None else 0, _p(residual), Cout if residual is not None else 0, out_scale)
    flags = (_l.EPI_F32OUT if out_f32 else 0) | (_l.EPI_F32SIDE if side == F32 else 0)
    ws = ws_bytes = None
    if h16 or not out_f32:
        # small images with a deep K (the 9x5 level) run split over the three kernel rows and need an fp32 workspace
        ws_bytes = lib.dm4d_conv3x3_ws_bytes(B, H, W, Cin, Ho, Wo, Cout, stride, pad, up)
        ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=x.device) if ws_bytes else None
    with _Prof("conv3x3", 2.0 * B * Ho * Wo * 9 * Cin * Cout, "flop", B * Ho * Wo):
        if h16:
            _l.call("dm4d_conv3x3_nhwc_f16", *args, flags, _p(ws), ws_bytes)
        elif out_f32:
            _l.call("dm4d_conv3x3_nhwc_bf16_flags", *args, flags)
        else:
            _l.call("dm4d_conv3x3_nhwc_bf16_ws", *args, _p(ws), ws_bytes)
    if not h16:
        _trace("conv3x3", y, x=x, wt=wt, bias=bias, rowbias=rowbias, residual=residual, stride=stride, pad=pad, pad_hi=pad_hi,
               upsample=upsample, out_scale=out_scale, out_f32=bool(out_f32))
    return y


# ---- wide precisions: operands -------------------------------------------------------------------------------------------
def dup_k(w: torch.Tensor, taps: int = 1, times: int = 2) -> torch.Tensor:
    """Weights for a two-term operand: [N, taps * C] -> [N, taps * times * C] with every tap's C columns repeated `times` times
    ([W | W] per tap), so that  [hi | lo] [W | W]^T = (hi + lo) W^T.  Host / load-time helper (any device)."""
    n, k = w.shape
    c = k // taps
    return w.reshape(n, taps, 1, c).expand(n, taps, times, c).reshape(n, taps * times * c).contiguous()


def split(x: torch.Tensor, x2: Optional[torch.Tensor] = None, *, cpad: Optional[int] = None, silu: bool = False,
          scale: float = 1.0, pattern: int = 0, transposed: bool = False, h16: bool = False) -> torch.Tensor:
    """fp32 [..., C] (channel concat with x2) -> the OPERAND of a contraction.  Parity precision: two-term bf16 [..., 2 cpad] =
    [hi | lo] (pattern 1: [hi | lo | hi], 2: [hi | hi | lo], three planes); h16 (precision "fp16"): one fp16 plane [..., cpad].
    transposed: x is a 2-D view [K, M] read as its transpose (result [M, planes * K])."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != F32:
        raise _l.Dm4dError("split: expected an fp32 tensor on a HIP device")
    planes = 1 if h16 else (2 if pattern == 0 else 3)
    if transposed:
        assert x.ndim == 2 and x2 is None and x.stride(1) == 1
        C1, M = x.shape
        rs1, cs1, lead = 1, x.stride(0), (M,)
    else:
        assert x.stride(-1) == 1
        C1 = x.shape[-1]
        x2d = x.reshape(-1, C1) if x.is_contiguous() else x
        assert x2d.ndim == 2
        M, rs1, cs1, lead = x2d.shape[0], x2d.stride(0), 1, tuple(x.shape[:-1])
        x = x2d
    C2, rs2 = 0, 0
    if x2 is not None:
        _req(x2, "x2", F32)
        x2 = x2.reshape(-1, x2.shape[-1])
        assert x2.shape[0] == M
        C2, rs2 = x2.shape[1], x2.stride(0)
    Cp = cpad or (C1 + C2)
    y = torch.empty(lead + (planes * Cp,), dtype=F16 if h16 else BF16, device=x.device)
    with _Prof("split", 4.0 * M * (C1 + C2) + 2.0 * M * planes * Cp, "byte", M):  # fp32 in, 16-bit planes out
        if h16:
            _l.call("dm4d_to_f16_f32", _stream(), _p(x), rs1, cs1, C1, _p(x2), rs2, C2, _p(y), Cp, M, Cp, 1 if silu else 0, scale)
        else:
            _l.call("dm4d_split_f32", _stream(), _p(x), rs1, cs1, C1, _p(x2), rs2, C2, _p(y), planes * Cp, M, Cp, 1 if silu else 0,
                    scale, pattern)
    return y


UP2X_PHASE = os.environ.get("DM4D_UP2X_PHASE", "1") != "0"  # Upsample2D as four 2x2 phase convolutions; off = the gather kernel (A/B, tests)
FF_FUSED = os.environ.get("DM4D_FF_FUSED", "1") != "0"  # level-0 feed-forward (C = 320) as one launch; off = the two-GEMM form (A/B, tests)
# the attention output projection + residual as a prologue of that launch (FeedForward.after_attention); off = its own GEMM (A/B, tests)
FF_PROJ_FUSED = os.environ.get("DM4D_FF_PROJ_FUSED", "1") != "0"


class FeedForward:
    """ff(n) + residual of a transformer block (attention.py:129-149): GEGLU projection then output projection.  Where the fused
    kernel is built for the shape (dm4d_ff_geglu_supported: C = 320) the per-step packed weights are made here, at load time
    (the stream is drained before the object is handed out, as in Upsampler), and the call is ONE launch whose hidden tensor
    never leaves the chip; other shapes -- and FF_FUSED = False -- run gemm(GEGLU) + gemm(residual).  Both forms are
    bit-identical (tests/opcheck.py ff_fused_*)."""

    def __init__(self, w1: torch.Tensor, b1: Optional[torch.Tensor], w2: torch.Tensor, b2: Optional[torch.Tensor]):
        self.w1, self.b1, self.w2, self.b2 = w1, b1, w2, b2
        self.C, self.hidden = w2.shape[0], w2.shape[1]
        assert w1.shape == (2 * self.hidden, self.C)
        self.packed = None
        if w1.is_cuda and _l.load().dm4d_ff_geglu_supported(self.C, self.hidden):
            _req(w1, "w1", w1.dtype), _req(w2, "w2", w1.dtype)  # bf16, or fp16 (precision "fp16": the packing permutes 16-bit words)
            with torch.cuda.device(w1.device):
                w1p, b1p, w2p = torch.empty_like(w1), torch.empty(2 * self.hidden, dtype=w1.dtype, device=w1.device), torch.empty_like(w2)
                _l.call("dm4d_ff_geglu_prepare_bf16", _stream(), _p(w1.contiguous()), _p(b1), _p(w2.contiguous()), _p(w1p), _p(b1p),
                        _p(w2p), self.C, self.hidden)
                torch.cuda.current_stream(w1.device).synchronize()
            self.packed = (w1p, b1p, w2p)

    def _one_launch(self, dma: torch.Tensor, *others) -> bool:
        """The guards every one-launch form shares: packed weights, the FF_FUSED switch, `dma` (the input the kernel fetches by DMA) below
        4 GiB, and 16-byte-aligned starts and rows of `dma` and `others` (None passes).  Any other view takes the separate launches,
        which accept 8-element-aligned strides."""
        return (self.packed is not None and FF_FUSED and dma.shape[0] * dma.stride(0) * 2 < (1 << 32)
                and all(t is None or (t.data_ptr() % 16 == 0 and (t.ndim < 2 or t.stride(0) * t.element_size() % 16 == 0))
                        for t in (dma,) + others))

    def _proj_one_launch(self, a: torch.Tensor, wo: torch.Tensor, *others) -> bool:
        """_one_launch for the forms that start at the attention output projection: they also want a contiguous square weight."""
        return FF_PROJ_FUSED and wo.shape == (self.C, self.C) and wo.is_contiguous() and self._one_launch(a, wo, *others)

    def _launch(self, name: str, like: torch.Tensor, odt, cols: int, front, mid=(), flags=()) -> torch.Tensor:
        """One launch of the entry `name`: (stream, *front, packed weights, b2, *mid, out, ldo, *flags, M, C, hidden) -> out [M, C] of
        dtype odt next to `like`; cols = the weight rows the launch multiplies by, for the profile."""
        M = like.shape[0]
        out = torch.empty((M, self.C), dtype=odt, device=like.device)
        w1p, b1p, w2p = self.packed
        with _Prof("linear", 2.0 * M * cols * self.C, "flop", M):
            _l.call(name, _stream(), *front, _p(w1p), _p(b1p), _p(w2p), _p(self.b2), *mid, _p(out), out.stride(0), *flags, M, self.C,
                    self.hidden)
        return out

    def __call__(self, n: torch.Tensor, residual: torch.Tensor, ln=None) -> torch.Tensor:
        """ln = (gamma, beta, eps): `n` is the un-normalised input and the LayerNorm in front of the feed-forward (norm3) is applied
        here -- inside the fused launch, or as its own launch in the two-GEMM form."""
        if not self._one_launch(n, residual, *(ln[:2] if ln is not None else ())):
            if ln is not None:
                n = layernorm(n, ln[0], ln[1], ln[2])
            f = gemm(n, self.w1, bias=self.b1, geglu=True)
            return gemm(f, self.w2, bias=self.b2, residual=residual)
        _req(n, "n"), _req(residual, "residual")
        if ln is not None:
            _req(ln[0], "gamma"), _req(ln[1], "beta")
        gamma, beta, eps = (_p(ln[0]), _p(ln[1]), float(ln[2])) if ln is not None else (None, None, 0.0)
        out = self._launch("dm4d_ff_geglu_fused_bf16", n, BF16, 3 * self.hidden, (_p(n), n.stride(0), gamma, beta, eps),
                           mid=(_p(residual), residual.stride(0)))
        _trace("ff_fused", out, n=n, residual=residual, ln=ln, w1=self.w1, b1=self.b1, w2=self.w2, b2=self.b2)
        return out

    def after_attention(self, a: torch.Tensor, wo: torch.Tensor, bo: Optional[torch.Tensor], x: torch.Tensor, ln) -> torch.Tensor:
        """The tail of a transformer block: h = a wo^T + bo + x (attention output projection + residual), then ff(LayerNorm(h)) + h.
        One launch where the fused kernel is built for the shape (FF_PROJ_FUSED), gemm + __call__ otherwise: the same products and bf16
        rounding points either way (since round 6 the one-launch form adds its fp32 terms in another order: one-ulp differences on isolated
        elements, tests/opcheck.py ff_proj_fused_*).  A column view of a wider tensor as `a` or `x` takes the separate launches."""
        if ln is None or not self._proj_one_launch(a, wo, x):
            h = gemm(a, wo, bias=bo, residual=x)
            return self(h, h, ln=ln)
        _req(a, "a"), _req(wo, "wo"), _req(x, "x"), _req(ln[0], "gamma"), _req(ln[1], "beta")
        out = self._launch("dm4d_attn_out_ff_geglu_fused_bf16", a, BF16, 3 * self.hidden + self.C,
                           (_p(a), a.stride(0), _p(wo), _p(bo), _p(x), x.stride(0), _p(ln[0]), _p(ln[1]), float(ln[2])))
        _trace("attn_out_ff_fused", out, a=a, wo=wo, bo=bo, x=x, ln=ln, w1=self.w1, b1=self.b1, w2=self.w2, b2=self.b2)
        return out

    def after_attention_f16(self, a: torch.Tensor, wo: torch.Tensor, bo: Optional[torch.Tensor], x: torch.Tensor, ln, out_f32: bool) -> torch.Tensor:
        """The same tail in precision "fp16": a fp16 [M, C], x the fp32 residual stream; the result is fp32 (out_f32) or the fp16 operand
        of the next contraction.  One launch (dm4d_attn_out_ff_geglu_fused_f16: h stays in the accumulators, never stored) where the kernel
        is built for the shape, otherwise gemm -> fp32 h, layernorm, gemm(GEGLU), gemm(+ h); the two forms agree to fp32 rounding."""
        if not self._proj_one_launch(a, wo, x, ln[0], ln[1]):
            h = gemm(a, wo, bias=bo, residual=x, out_f32=True)
            f = gemm(layernorm(h, ln[0], ln[1], ln[2]), self.w1, bias=self.b1, geglu=True)
            return gemm(f, self.w2, bias=self.b2, residual=h, out_f32=out_f32)
        _req(a, "a", F16), _req(wo, "wo", F16), _req(x, "x", F32), _req(ln[0], "gamma", F16), _req(ln[1], "beta", F16)
        return self._launch("dm4d_attn_out_ff_geglu_fused_f16", a, F32 if out_f32 else F16, 3 * self.hidden + self.C,
                            (_p(a), a.stride(0), _p(wo), _p(bo), _p(x), x.stride(0), _p(ln[0]), _p(ln[1]), float(ln[2])),
                            flags=(1 if out_f32 else 0,))


# proj_in + norm1 + QKV projection of a level-0 transformer (C = 320) as one launch (proj_in_ln_qkv); off = gemm, layernorm, gemm (A/B, tests)
L0_HEAD_FUSED = os.environ.get("DM4D_L0_HEAD_FUSED", "1") != "0"


def _on_device(t: torch.Tensor) -> bool:
    return t.is_cuda


def _rows16(*ts) -> bool:
    """2-D views whose rows start on 16-byte boundaries (row strides in multiples of 8 elements, contiguous columns)."""
    return all(t.ndim == 2 and t.data_ptr() % 16 == 0 and t.stride(0) % 8 == 0 and t.stride(1) == 1 for t in ts)


def _l0_fusable(C: int, rows, weights, vectors) -> bool:
    """The guards of FeedForward.after_attention for the level-0 head launch: bf16 device tensors, 16-byte-aligned rows, M * stride * 2 <
    2^32 for the DMA-fetched input (rows[0]), contiguous 16-byte-aligned weights and vectors, and a channel count the kernels are built for."""
    ts = tuple(rows) + tuple(weights) + tuple(v for v in vectors if v is not None)
    return (all(isinstance(t, torch.Tensor) and t.dtype == BF16 and _on_device(t) for t in ts) and _rows16(*rows)
            and all(t.shape[1] == C and t.stride(0) < (1 << 24) for t in rows)
            and rows[0].shape[0] * rows[0].stride(0) * 2 < (1 << 32)
            and all(w.is_contiguous() and w.data_ptr() % 16 == 0 for w in weights)
            and all(v is None or (v.is_contiguous() and v.data_ptr() % 16 == 0) for v in vectors)
            and bool(_l.load().dm4d_l0_linear_fused_supported(C)))


def _launch_l0_head(n, wpi, bpi, ln, wqkv, h, qkv, n1) -> None:
    M, C = n.shape
    with _Prof("linear", 2.0 * M * (C + 3 * C) * C, "flop", M):
        _l.call("dm4d_proj_in_ln_qkv_fused_bf16", _stream(), _p(n), n.stride(0), _p(wpi), _p(bpi), _p(ln[0]), _p(ln[1]), float(ln[2]),
                _p(wqkv), _p(h), h.stride(0), _p(qkv), qkv.stride(0), _p(n1), n1.stride(0) if n1 is not None else 0, M, C)


def proj_in_ln_qkv(n: torch.Tensor, wpi: torch.Tensor, bpi: Optional[torch.Tensor], ln, wqkv: torch.Tensor,
                   qkv: Optional[torch.Tensor] = None):
    """The head of a transformer whose first block follows proj_in (transformer_multiview.py:160, attention.py:73-78):
    h = n wpi^T + bpi, qkv = LayerNorm(h) wqkv^T with ln = (gamma, beta, eps); returns (h, qkv).  One launch at C = 320 (L0_HEAD_FUSED:
    LayerNorm(h) never leaves the chip), otherwise gemm, layernorm, gemm: the same products and bf16 rounding points, h bit-identical, the
    LayerNorm's fp32 row sums in another order (one-ulp differences on isolated elements of qkv).  `qkv`: a [M, 3C] view to write into."""
    M, C = n.shape[0], wpi.shape[0]
    fused = (L0_HEAD_FUSED and wpi.shape == (C, C) and wqkv.shape == (3 * C, C) and n.shape[1] == C
             and (qkv is None or (qkv.shape == (M, 3 * C) and _rows16(qkv) and qkv.dtype == BF16 and qkv.stride(0) < (1 << 24)))
             and _l0_fusable(C, (n,), (wpi, wqkv), (bpi, ln[0], ln[1])))
    if not fused:
        h = gemm(n, wpi, bias=bpi)
        return h, gemm(layernorm(h, ln[0], ln[1], ln[2]), wqkv, out=qkv)
    h = torch.empty((M, C), dtype=BF16, device=n.device)
    if qkv is None:
        qkv = torch.empty((M, 3 * C), dtype=BF16, device=n.device)
    # operator trace: the launch also stores LayerNorm(h), and is recorded part by part under the names of the separate launches
    n1 = torch.empty((M, C), dtype=BF16, device=n.device) if TRACE is not None else None
    _launch_l0_head(n, wpi, bpi, ln, wqkv, h, qkv, n1)
    if TRACE is not None:
        _trace("gemm", h, a=n, w=wpi, a2=None, bias=bpi, rowbias=None, rows_per_rowbias=1, residual=None, geglu=False, silu=False,
               out_scale=1.0, out_f32=False, split_out=False)
        _trace("layernorm", n1, x=h, gamma=ln[0], beta=ln[1], eps=ln[2])
        _trace("gemm", qkv, a=n1, w=wqkv, a2=None, bias=None, rowbias=None, rows_per_rowbias=1, residual=None, geglu=False, silu=False,
               out_scale=1.0, out_f32=False, split_out=False)
    return h, qkv


def conv_up2x_prepare(wt: torch.Tensor) -> torch.Tensor:
    """3x3 weights [Cout, 9*Cin] ((ky,kx,ci) order) -> the four 2x2 phase kernels [4, Cout, 4*Cin] of conv_up2x (once per
    layer: sums of the taps that read the same low-resolution pixel, fp32, rounded to bf16 once)."""
    h16 = wt.dtype == F16  # precision "fp16": fp16 taps in, fp16 phase kernels out
    _req(wt, "wt", F16 if h16 else BF16)
    assert wt.is_contiguous() and wt.shape[1] % 9 == 0
    Cout, Cin = wt.shape[0], wt.shape[1] // 9
    wp = torch.empty((4, Cout, 4 * Cin), dtype=wt.dtype, device=wt.device)
    _l.call("dm4d_conv_up2x_prepare_f16" if h16 else "dm4d_conv_up2x_prepare_bf16", _stream(), _p(wt), _p(wp), Cout, Cin)
    return wp


def conv_up2x_supported(Cin: int, Cout: int) -> bool:
    return Cin % 64 == 0 and Cout % 8 == 0


class Upsampler:
    """Upsample2D of the UNet / VAE decoder: nearest x2 + 3x3 convolution.  Runs as four 2x2 phase convolutions of the
    low-resolution input (conv_up2x) when the channel counts allow, else as the gather kernel that reads the upsampled
    image through index arithmetic.  The phase kernels are made from the checkpoint's 3x3 weights HERE, at load time, and the
    stream is drained before the object is handed out: the runner's task streams (one worker thread and HIP stream each,
    sharing one pipeline) must never see a published `wp` whose prepare kernel is still queued on another stream."""

    def __init__(self, wt: torch.Tensor, bias: Optional[torch.Tensor], parity: bool = False, h16: bool = False):
        """parity (precision "parity"): wt is duplicated along Cin, the input fp32; the phase kernels -- whose weights are SUMS of taps
        rounded to bf16 once more, a deviation from the checkpoint's arithmetic -- are not used: the gather kernel reads the upsampled
        image of the two-term operand through index arithmetic and multiplies by the checkpoint's own weights."""
        # h16 (precision "fp16"; implies `parity` = fp32 tensors): fp16 weights, one fp16 operand plane; the phase kernels ARE used (their
        # extra weight rounding is 2^-12 relative in fp16, inside the precision's budget -- in bf16 it would be 2^-9)
        self.wt, self.bias, self.wp, self.parity, self.h16 = wt, bias, None, parity or h16, h16
        self.phase = (h16 or not self.parity) and conv_up2x_supported(wt.shape[1] // 9, wt.shape[0]) and UP2X_PHASE
        if self.phase and wt.is_cuda:
            with torch.cuda.device(wt.device):
                self.wp = conv_up2x_prepare(wt)
                torch.cuda.current_stream(wt.device).synchronize()

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        if self.h16 and self.phase and x.numel() * 2 < (1 << 32):
            if self.wp is None or self.wp.device != x.device:
                raise _l.Dm4dError("Upsampler: phase kernels were not prepared on the input's device")
            return conv_up2x(split(x, h16=True), self.wp, bias=self.bias, out_f32=True)
        if self.parity:
            return conv3x3(split(x, h16=self.h16), self.wt, bias=self.bias, upsample=True, out_f32=True)
        # the phase kernel addresses its input with 32-bit byte offsets: inputs of 4 GiB or more take the gather kernel
        if not self.phase or x.numel() * 2 >= (1 << 32):
            return conv3x3(x, self.wt, bias=self.bias, upsample=True)
        if self.wp is None or self.wp.device != x.device:
            raise _l.Dm4dError(f"Upsampler: phase kernels live on {None if self.wp is None else self.wp.device}, input on {x.device} "
                            "(reload the pipeline on the new device: host/loader.py does)")
        return conv_up2x(x, self.wp, bias=self.bias)


def conv_up2x(x: torch.Tensor, wp: torch.Tensor, *, bias=None, out_f32: bool = False) -> torch.Tensor:
    """conv3x3(nearest_upsample_x2(x)) from the phase kernels of conv_up2x_prepare: x [B,H,W,Cin] -> [B,2H,2W,Cout].
    fp16 x / wp / bias (precision "fp16"): fp32 (out_f32) or fp16 result."""
    h16 = wp.dtype == F16
    dt = F16 if h16 else BF16
    _req(x, "x", dt), _req(wp, "wp", dt)
    assert x.is_contiguous() and wp.is_contiguous() and (h16 or not out_f32)
    B, H, W, Cin = x.shape
    Cout = wp.shape[1]
    assert wp.shape == (4, Cout, 4 * Cin), (wp.shape, Cin)
    y = torch.empty((B, 2 * H, 2 * W, Cout), dtype=F32 if out_f32 else dt, device=x.device)
    # credited with the multiply-adds it executes (4 taps per output pixel), not the 9 of the op it replaces
    with _Prof("conv3x3", 2.0 * B * 4 * H * W * 4 * Cin * Cout, "flop", B * 4 * H * W):
        if h16:
            _l.call("dm4d_conv_up2x_nhwc_f16", _stream(), _p(x), B, H, W, Cin, _p(wp), _p(y), Cout, _p(bias), _l.EPI_F32OUT if out_f32 else 0)
        else:
            _l.call("dm4d_conv_up2x_nhwc_bf16", _stream(), _p(x), B, H, W, Cin, _p(wp), _p(y), Cout, _p(bias))
    if not h16:
        _trace("conv_up2x", y, x=x, wp=wp, bias=bias)
    return y


def conv2d_direct(x: torch.Tensor, wt: torch.Tensor, *, ksize: int, bias=None, stride: int = 1, pad: int = 1,
                  silu: bool = False) -> torch.Tensor:
    """Thin-layer convolution (PoseEncoder): x [B,H,W,Cin] NHWC, wt [Cout, ksize*ksize*Cin] ((ky,kx,ci) order).  bf16 tensors, or
    (parity precision) x, wt, bias and the result all fp32."""
    dt = F32 if x.dtype == F32 else BF16
    _req(x, "x", dt), _req(wt, "wt", dt)
    if bias is not None:
        _req(bias, "bias", dt)
    assert x.is_contiguous() and wt.is_contiguous()
    B, H, W, Cin = x.shape
    Cout = wt.shape[0]
    assert wt.shape[1] == ksize * ksize * Cin, (wt.shape, ksize, Cin)
    Ho, Wo = (H + 2 * pad - ksize) // stride + 1, (W + 2 * pad - ksize) // stride + 1
    y = torch.empty((B, Ho, Wo, Cout), dtype=dt, device=x.device)
    _l.call("dm4d_conv2d_direct_nhwc_f32" if dt == F32 else "dm4d_conv2d_direct_nhwc_bf16",
            _stream(), _p(x), B, H, W, Cin, _p(wt), _p(bias), _p(y), Ho, Wo, Cout, ksize, stride, pad, 1 if silu else 0)
    return y


def groupnorm(x1: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int, eps: float, *,
              x2: Optional[torch.Tensor] = None, silu: bool = False, raw_out: bool = False):
    """GroupNorm(+SiLU) over the channel concat [x1 | x2]; x [B, HW, C] (any leading spatial shape).
    fp32 input (wide precisions): the result leaves as an operand -- parity: fp64 statistics, two-term [..., 2 C]; fp16 (fp16 gamma / beta):
    one fp16 plane.  fp16 input (precision "fp16": an activation its producer left in fp16, conv1's output in front of norm2) -> one fp16
    plane.  raw_out (fp16 precision, fp32 input): also returns fp16 of the un-normalised concat [x1 | x2] (the shortcut convolution's
    operand) -> (y, raw)."""
    lib = _l.load()
    xdt = x1.dtype if isinstance(x1, torch.Tensor) and x1.dtype in (F32, F16) else BF16
    wide = xdt == F32
    h16 = xdt == F16 or (wide and gamma.dtype == F16)  # precision "fp16": fp16 parameters, one fp16 plane out
    pdt, planes = (F16 if h16 else BF16), (2 if wide and not h16 else 1)
    assert wide or not raw_out
    _req(x1, "x1", xdt), _req(gamma, "gamma", pdt), _req(beta, "beta", pdt)
    assert x1.is_contiguous()
    B, C1 = x1.shape[0], x1.shape[-1]
    HW = x1.numel() // (B * C1)
    C2 = 0
    if x2 is not None:
        _req(x2, "x2", xdt)
        assert x2.is_contiguous() and x2.shape[0] == B
        C2 = x2.shape[-1]
    y = torch.empty(x1.shape[:-1] + (planes * (C1 + C2),), dtype=pdt, device=x1.device)
    if wide:
        ws = torch.empty(lib.dm4d_groupnorm_f32_ws_bytes(B, HW, groups) // 8, dtype=torch.float64, device=x1.device)
    else:
        ws = torch.empty(lib.dm4d_groupnorm_ws_bytes(B, HW, groups) // 4, dtype=torch.float32, device=x1.device)
    # ALGORITHMIC bytes per element: read once + write once (the operand out: one 16-bit plane, or hi + lo); the statistics
    # pass re-reads the input (mostly from L2 / Infinity Cache), so the device moves up to 1.5x this
    bpe = (4.0 if wide else 2.0) + 2.0 * planes
    n_in = x1.numel() + (x2.numel() if x2 is not None else 0)
    if raw_out:
        if not h16:
            raise _l.Dm4dError("groupnorm: raw_out is a feature of the fp16 precision")
        fused = C1 % 8 == 0 and C2 % 8 == 0 and all(t is None or t.data_ptr() % 16 == 0 for t in (x1, x2))
        if not fused:  # shapes the vectorised kernels do not take: the operand from its own pass
            M = B * HW
            return (groupnorm(x1, gamma, beta, groups, eps, x2=x2, silu=silu),
                    split(x1.reshape(M, C1), x2.reshape(M, C2) if x2 is not None else None, h16=True).view(y.shape))
        raw = torch.empty_like(y)
        with _Prof("groupnorm", (bpe + 2.0) * n_in, "byte", B * HW):
            _l.call("dm4d_groupnorm_nhwc_f32_f16_raw", _stream(), _p(x1), C1, _p(x2), C2, B, HW, groups, eps, _p(gamma), _p(beta), _p(y),
                    _p(raw), 1 if silu else 0, _p(ws))
        return y, raw
    if wide:
        name = "dm4d_groupnorm_nhwc_f32_f16" if h16 else "dm4d_groupnorm_nhwc_f32_split"
    else:
        name = "dm4d_groupnorm_nhwc_f16_f16" if h16 else "dm4d_groupnorm_nhwc_bf16"
    with _Prof("groupnorm", bpe * n_in, "byte", B * HW):
        _l.call(name, _stream(), _p(x1), C1, _p(x2), C2, B, HW, groups, eps, _p(gamma), _p(beta), _p(y), 1 if silu else 0, _p(ws))
    if xdt == BF16:
        _trace("groupnorm", y, x1=x1, x2=x2, gamma=gamma, beta=beta, groups=groups, eps=eps, silu=silu)
    return y


class groupnorm_as_in_batch:
    """with groupnorm_as_in_batch(B): the GroupNorm launches of this thread on fewer than B samples chunk their statistics as a launch
    on B samples does, so a sample gets the bits it has inside the batch of B (dm4d.h: dm4d_groupnorm_plan_batch)."""

    def __init__(self, batch: int):
        self.batch = int(batch)

    def __enter__(self):
        _l.call("dm4d_groupnorm_plan_batch", self.batch)

    def __exit__(self, *exc):
        _l.call("dm4d_groupnorm_plan_batch", 0)
        return False


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    """fp32 input (wide precisions): the result leaves as an operand -- parity: two-term [..., 2 C]; fp16 (fp16 gamma / beta): one fp16
    plane."""
    wide = isinstance(x, torch.Tensor) and x.dtype == F32
    h16 = wide and gamma.dtype == F16
    pdt, planes = (F16 if h16 else BF16), (2 if wide and not h16 else 1)
    _req(x, "x", F32 if wide else BF16), _req(gamma, "gamma", pdt), _req(beta, "beta", pdt)
    x2 = x.reshape(-1, x.shape[-1])
    M, C = x2.shape
    y = torch.empty((M, planes * C), dtype=pdt, device=x.device)
    if wide:
        name = "dm4d_layernorm_f32_f16" if h16 else "dm4d_layernorm_f32_split"
    else:
        name = "dm4d_layernorm_bf16"
    with _Prof("layernorm", ((4.0 if wide else 2.0) + 2.0 * planes) * x2.numel(), "byte", M):
        _l.call(name, _stream(), _p(x2), x2.stride(0), _p(gamma), _p(beta), _p(y), y.stride(0), M, C, eps)
    if not wide:
        _trace("layernorm", y, x=x2, gamma=gamma, beta=beta, eps=eps)
    return y.view(x.shape[:-1] + (planes * C,))


HEAD_DIMS_HD = (40, 80, 160)  # head dimensions of the attention_hd.hip kernels (SD-1.x layout); 64 has attention.hip's own


def _head_dim(width: int, heads: int, what: str) -> int:
    """Head dimension of an operand `width` channels wide over `heads` heads: 64 or one of HEAD_DIMS_HD, else Dm4dError."""
    d = width // heads if heads > 0 else 0
    if heads <= 0 or d * heads != width or (d != 64 and d not in HEAD_DIMS_HD):
        raise _l.Dm4dError(f"{what}: {width} channels over {heads} heads; supported head dimensions are 64, "
                           + ", ".join(str(x) for x in HEAD_DIMS_HD))
    return d


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, batch: int, heads: int, seq: int,
              scale: Optional[float] = None, out: Optional[torch.Tensor] = None,
              kv_seq: Optional[int] = None, q_scaled: bool = False) -> torch.Tensor:
    """q/k/v: [batch*seq, >=heads*d] row-strided views (e.g. column slices of the fused QKV output), d = q.shape[1] // heads:
    64 (attention.hip) or 40 / 80 / 160 (attention_hd.hip; pre-scaled Q only).
    kv_seq: keys per batch when K/V hold more tokens than Q (frame-sharded 3-D attention); default = seq.
    q_scaled: q already carries scale * LOG2E (folded into the to_q weights, unet._TransformerBlock)."""
    h16 = isinstance(q, torch.Tensor) and q.dtype == F16  # precision "fp16": fp16 Q (pre-scaled) / K / V -> fp16 O
    dt = F16 if h16 else BF16
    _req(q, "q", dt), _req(k, "k", dt), _req(v, "v", dt)
    d = _head_dim(q.shape[1], heads, "attention")
    assert q.shape[0] == batch * seq and q.shape[1] == heads * d, (q.shape, batch, seq, heads)
    kv_seq = seq if kv_seq is None else kv_seq
    assert k.shape[0] == batch * kv_seq and v.shape[0] == batch * kv_seq, (k.shape, batch, kv_seq)
    if out is None:
        out = torch.empty((batch * seq, heads * d), dtype=dt, device=q.device)
    if h16 and not q_scaled:
        raise _l.Dm4dError("attention: fp16 operands need a pre-scaled Q (gemm(..., scale_cols=C, col_scale=scale * LOG2E))")
    if d != 64 and not q_scaled:
        raise _l.Dm4dError(f"attention: head dimension {d} needs a pre-scaled Q (gemm(..., scale_cols=C, col_scale=scale * LOG2E))")
    if scale is None:
        scale = d ** -0.5
    prof = KERNEL_TIMER
    if prof is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    with _Prof("attention", 4.0 * batch * heads * seq * kv_seq * d, "flop", batch * seq):
        args = (_stream(), _p(q), _p(k), _p(v), _p(out), q.stride(0), k.stride(0), v.stride(0), out.stride(0), batch, heads)
        if d != 64:
            _l.call("dm4d_attention_hd_qscaled_kv_f16" if h16 else "dm4d_attention_hd_qscaled_kv_bf16", *args, d, seq, kv_seq)
        elif h16:
            _l.call("dm4d_attention_qscaled_kv_f16", *args, seq, kv_seq)
        elif q_scaled:
            _l.call("dm4d_attention_qscaled_kv_bf16", *args, seq, kv_seq)
        else:
            _l.call("dm4d_attention_kv_bf16", *args, seq, kv_seq, scale)
    if prof is not None:
        e1.record()
        prof.append(("attn_kernel" if d == 64 else "attn_hd_kernel", 4.0 * batch * heads * seq * kv_seq * d, e0, e1))
    if h16 or d != 64:  # oracle/replay.py recomputes the head_dim 64 launches only
        return out
    _trace("attention", out, q=q, k=k, v=v, batch=batch, heads=heads, seq=seq, kv_seq=kv_seq, scale=scale, q_scaled=q_scaled)
    return out


def attention_split(qkv: Optional[torch.Tensor], batch: int, heads: int, seq: int, scale: Optional[float] = None, *,
                    q: Optional[torch.Tensor] = None, kv: Optional[torch.Tensor] = None, kv_seq: Optional[int] = None) -> torch.Tensor:
    """Parity precision: qkv [batch*seq, 6 C] = the planes gemm(split_out=True) leaves for a fused QKV projection
    ([q_hi | k_hi | v_hi | q_lo | k_lo | v_lo], C = heads * d) -> attention output as a two-term operand [batch*seq, 2 C].
    Frame-sharded form (qkv = None): q [batch*seq, 2 C] = [q_hi | q_lo] of the local queries, kv [batch*kv_seq, 4 C] =
    [k_hi | v_hi | k_lo | v_lo] of the all-gathered keys (the planes of gemm(n, w_kv, split_out=True)).
    Three MFMAs per product, exact running-max softmax in fp32 (dm4d_attention_split_bf16; head dimensions 40 / 80 / 160:
    dm4d_attention_hd_split_bf16).  d comes from the operand widths: qkv.shape[1] // (6 heads), or q.shape[1] // (2 heads)."""
    if qkv is not None:
        d = _head_dim(qkv.shape[1] // 6 if qkv.shape[1] % 6 == 0 else -1, heads, "attention_split")
    else:
        d = _head_dim(q.shape[1] // 2 if q.shape[1] % 2 == 0 else -1, heads, "attention_split")
    C = heads * d
    if qkv is not None:
        _req(qkv, "qkv")
        assert qkv.shape == (batch * seq, 6 * C), (qkv.shape, batch, seq, heads)
        qp, kp, vp = qkv.data_ptr(), qkv.data_ptr() + 2 * C, qkv.data_ptr() + 4 * C
        ldq = ldk = ldv = qkv.stride(0)
        q_lo = k_lo = v_lo = 3 * C
        kv_seq, dev = seq, qkv.device
    else:
        _req(q, "q"), _req(kv, "kv")
        kv_seq = seq if kv_seq is None else kv_seq
        assert q.shape == (batch * seq, 2 * C) and kv.shape == (batch * kv_seq, 4 * C), (q.shape, kv.shape, batch, seq, kv_seq, heads)
        qp, kp, vp = q.data_ptr(), kv.data_ptr(), kv.data_ptr() + 2 * C
        ldq, ldk, ldv = q.stride(0), kv.stride(0), kv.stride(0)
        q_lo, k_lo, v_lo = C, 2 * C, 2 * C
        dev = q.device
    out = torch.empty((batch * seq, 2 * C), dtype=BF16, device=dev)
    scale = d ** -0.5 if scale is None else scale
    with _Prof("attention", 3 * 4.0 * batch * heads * seq * kv_seq * d, "flop", batch * seq):  # three MFMA terms per product
        args = (_stream(), qp, kp, vp, _p(out), ldq, ldk, ldv, out.stride(0), q_lo, k_lo, v_lo, C, batch, heads, seq, kv_seq, scale)
        if d == 64:
            _l.call("dm4d_attention_split_bf16", *args)
        else:
            _l.call("dm4d_attention_hd_split_bf16", *args, d)
    return out


def softmax_rows_split(s: torch.Tensor, scale: float, n: Optional[int] = None, h16: bool = False) -> torch.Tensor:
    """Wide precisions: P = softmax(s * scale) over the first n columns of fp32 logits s [M, Np] -> parity: three planes
    [p_hi | p_lo | p_hi], bf16 [M, 3 Np]; h16 (precision "fp16"): one fp16 plane [M, Np] (columns n .. Np-1 of every plane zero)."""
    _req(s, "s", F32)
    M, Np = s.shape
    n = Np if n is None else int(n)
    p = torch.empty((M, Np if h16 else 3 * Np), dtype=F16 if h16 else BF16, device=s.device)
    _l.call("dm4d_softmax_rows_f32_f16" if h16 else "dm4d_softmax_rows_f32_split", _stream(), _p(s), s.stride(0), _p(p), p.stride(0), M, n,
            Np, scale)
    return p


# bench.py sets this to a list to time individual launches with HIP events on the launch stream:
# entries are (kernel, algorithmic flops, start_event, end_event).  None = no instrumentation.
KERNEL_TIMER = None
# Same idea for every kernel family (bench.py's untimed breakdown pass): entries are (family, work, unit, start, end, rows)
# with unit "flop" or "byte" and rows = output rows of the launch.  None = no instrumentation.
PROFILE = None


class _Prof:
    """with _Prof(family, work, unit): <one launch>   -- records two events when ops.PROFILE is a list."""

    def __init__(self, family: str, work: float, unit: str, rows: int = 0):
        self.args = (family, work, unit)
        self.rows = int(rows)  # output rows (tokens / pixels) of the launch: bench.py derives the UNet level from it
        self.on = PROFILE is not None

    def __enter__(self):
        if self.on:
            self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if self.on:
            self.e1.record()
            PROFILE.append(self.args + (self.e0, self.e1, self.rows))
        return False


def softmax_rows(s: torch.Tensor, scale: float, n: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """P = softmax(s * scale) per row, bf16; s bf16 or fp32 (logits from gemm(out_f32=True)).
    n (fp32 logits only): softmax over the first n columns of every row -- a key axis padded to the GEMM's K granularity; `out`
    (same shape as s) then keeps whatever it holds behind column n (the caller's zeros)."""
    f32 = s.dtype == torch.float32
    _req(s, "s", torch.float32 if f32 else BF16)
    if n is not None and not f32:
        raise _l.Dm4dError("softmax_rows: a column count below the row length needs fp32 logits")
    p = torch.empty(s.shape, dtype=BF16, device=s.device) if out is None else out
    _req(p, "out", BF16)
    if p.shape != s.shape:
        raise _l.Dm4dError(f"softmax_rows: out has shape {tuple(p.shape)}, the logits {tuple(s.shape)}")
    _l.call("dm4d_softmax_rows_f32in_bf16" if f32 else "dm4d_softmax_rows_bf16", _stream(), _p(s), s.stride(0), _p(p), p.stride(0),
            s.shape[0], s.shape[1] if n is None else int(n), scale)
    _trace("softmax_rows", p, s=s, scale=scale, n=n)
    return p


def timestep_embedding(t: torch.Tensor, dim: int, flip_sin_to_cos: bool = True, freq_shift: float = 0.0,
                       out_f32: bool = False) -> torch.Tensor:
    _req(t, "t", torch.float32)
    out = torch.empty((t.shape[0], dim), dtype=F32 if out_f32 else BF16, device=t.device)
    _l.call("dm4d_timestep_embedding_f32" if out_f32 else "dm4d_timestep_embedding_bf16", _stream(), _p(t), _p(out), t.shape[0], dim,
            1 if flip_sin_to_cos else 0, freq_shift)
    return out


def silu(x: torch.Tensor) -> torch.Tensor:
    _req(x, "x")
    assert x.is_contiguous()
    y = torch.empty_like(x)
    _l.call("dm4d_silu_bf16", _stream(), _p(x), _p(y), x.numel())
    _trace("silu", y, x=x)
    return y


def pack_model_input(latents, pv_lat, plucker, skel, mask, is_cond, cpad: int, use_cfg: bool,
                     frame_idx: Optional[torch.Tensor] = None, h16: bool = False, out_row: Optional[torch.Tensor] = None,
                     rows: int = 0) -> torch.Tensor:
    """Inputs NHWC [N, HW, c] (task level); is_cond int32 [F]; frame_idx int32 [F] selects the window's frames
    (None: F = N, identity).  Mutates the cond rows of `latents` (reference aliasing).
    fp32 task tensors (wide precisions): the result is conv_in's operand -- [hi | lo] bf16, or (h16) one fp16 plane.
    out_row (int32 [F], with `rows`): only the frames with out_row[f] >= 0 are written, frame f to row out_row[f] of a compact result of
    `rows` rows per CFG half (dm4d.h: dm4d_pack_model_input_rows_bf16); the aliasing still covers every cond frame."""
    dt = F32 if latents.dtype == F32 else BF16  # fp32 task tensors = parity precision: the result is conv_in's two-term operand
    for t, n in ((latents, "latents"), (pv_lat, "pv_lat"), (plucker, "plucker"), (mask, "mask")):
        _req(t, n, dt)
        assert t.is_contiguous()
    if skel is not None:
        _req(skel, "skel", dt)
    _req(is_cond, "is_cond", torch.int32)
    F, HW = is_cond.shape[0], latents.shape[1]
    if frame_idx is not None:
        _req(frame_idx, "frame_idx", torch.int32)
        assert frame_idx.shape[0] == F
    else:
        assert latents.shape[0] == F
    assert not h16 or dt == F32
    Fo = F
    if out_row is not None:
        _req(out_row, "out_row", torch.int32)
        if out_row.shape[0] != F or not 1 <= rows <= F:
            raise _l.Dm4dError("pack_model_input: out_row needs one entry per window frame and 1 <= rows <= F")
        Fo = int(rows)
    out = torch.empty(((2 if use_cfg else 1) * Fo, HW, 2 * cpad if (dt == F32 and not h16) else cpad), dtype=F16 if h16 else BF16,
                      device=latents.device)
    suffix = ("f32_f16" if h16 else "f32_split") if dt == F32 else "bf16"
    front = (_stream(), _p(latents), _p(pv_lat), _p(plucker), _p(skel), _p(mask), _p(is_cond), _p(frame_idx))
    if out_row is None:
        _l.call("dm4d_pack_model_input_" + suffix, *front, _p(out), F, HW, cpad, 1 if use_cfg else 0)
    else:
        _l.call("dm4d_pack_model_input_rows_" + suffix, *front, _p(out_row), _p(out), F, Fo, HW, cpad, 1 if use_cfg else 0)
    return out


def rows_move(jobs) -> None:
    """One launch: dst[dst_idx[r]] = src[src_idx[r]] for every job (src, dst, src_idx, dst_idx) of `jobs` (dm4d.h: dm4d_rows_move; at most
    ROWS_MOVE_MAX_JOBS).  src / dst: contiguous device tensors of one dtype whose rows (dim 0) have the same byte size, a multiple of 16;
    src_idx / dst_idx: int32 device vectors of one length (0: the job is skipped).  The caller vouches for the indices -- they are not
    read here (no host sync) -- and for distinct dst rows."""
    if not jobs:
        return
    if len(jobs) > _l.ROWS_MOVE_MAX_JOBS:
        raise _l.Dm4dError(f"rows_move: {len(jobs)} jobs, one launch takes {_l.ROWS_MOVE_MAX_JOBS}")
    tab = (_l.RowsMoveJob * len(jobs))()
    moved = 0
    for t, (src, dst, si, di) in zip(tab, jobs):
        _req(src, "src", src.dtype), _req(dst, "dst", src.dtype), _req(si, "src_idx", torch.int32), _req(di, "dst_idx", torch.int32)
        if not (src.is_contiguous() and dst.is_contiguous() and si.is_contiguous() and di.is_contiguous()):
            raise _l.Dm4dError("rows_move: tensors and index vectors must be contiguous")
        rb = src[0].numel() * src.element_size() if src.shape[0] else 0
        if si.ndim != 1 or si.shape != di.shape or (si.shape[0] and (rb == 0 or dst.shape[0] == 0 or dst[0].numel() * dst.element_size() != rb)):
            raise _l.Dm4dError("rows_move: src and dst rows differ in size, or the index vectors in length")
        t.src, t.dst, t.src_row_idx, t.dst_row_idx, t.n_rows, t.row_bytes = _p(src), _p(dst), _p(si), _p(di), si.shape[0], max(rb, 16)
        moved += si.shape[0] * rb
    import ctypes
    with _Prof("rows_move", 2.0 * moved, "byte", 0):
        _l.call("dm4d_rows_move", _stream(), ctypes.cast(tab, ctypes.c_void_p), len(jobs))


def _cfg_step_inputs(latents, noise_pred, coef, is_cond, frame_idx):
    """What the three cfg_*_step wrappers ask of their common inputs -> (the tensors' dtype: fp32 in the wide precisions, F, HW)."""
    dt = F32 if latents.dtype == F32 else BF16
    _req(latents, "latents", dt), _req(noise_pred, "noise_pred", dt), _req(coef, "coef", torch.float32)
    _req(is_cond, "is_cond", torch.int32)
    if frame_idx is not None:
        _req(frame_idx, "frame_idx", torch.int32)
    return dt, is_cond.shape[0], latents.shape[1]


def cfg_ddim_step(latents, noise_pred, coef, is_cond, use_cfg: bool, guidance_scale: float, v_prediction: bool,
                  frame_idx: Optional[torch.Tensor] = None):
    """In-place DDIM update of rows frame_idx of `latents` [N,HW,4] from noise_pred [cfg*F, HW, ldn]."""
    dt, F, HW = _cfg_step_inputs(latents, noise_pred, coef, is_cond, frame_idx)
    _l.call("dm4d_cfg_ddim_step_f32" if dt == F32 else "dm4d_cfg_ddim_step_bf16", _stream(), _p(latents), _p(noise_pred),
            noise_pred.stride(-2), _p(coef), _p(is_cond), _p(frame_idx), F, HW, 1 if use_cfg else 0, guidance_scale,
            1 if v_prediction else 0)
    return latents


def cfg_linear_step(latents, x0_prev, noise_pred, coef, is_cond, use_cfg: bool, guidance_scale: float,
                    frame_idx: Optional[torch.Tensor] = None):
    """In-place linear multistep update (x' = a x + b m + c p; p' = d x + e m) of rows frame_idx of `latents` and `x0_prev`
    [N,HW,4] from noise_pred [cfg*F, HW, ldn]; coef [F,8] fp32 rows from scheduler.step_rows."""
    dt, F, HW = _cfg_step_inputs(latents, noise_pred, coef, is_cond, frame_idx)
    _req(x0_prev, "x0_prev", dt)
    assert x0_prev.shape == latents.shape and coef.shape[-1] == 8 and coef.is_contiguous()
    _l.call("dm4d_cfg_linear_step_f32" if dt == F32 else "dm4d_cfg_linear_step_bf16", _stream(), _p(latents), _p(x0_prev), _p(noise_pred),
            noise_pred.stride(-2), _p(coef), _p(is_cond), _p(frame_idx), F, HW, 1 if use_cfg else 0, guidance_scale)
    return latents


def cfg_multistep_step(latents, states, noise_pred, coef, is_cond, use_cfg: bool, guidance_scale: float,
                       frame_idx: Optional[torch.Tensor] = None):
    """In-place general linear multistep update (UniPC with its corrector, DEIS; dm4d.h: dm4d_cfg_multistep_step_bf16) of rows frame_idx
    of `latents` and of the stored tensors `states` (a list of 1-3 tensors shaped like latents, zero at the start of a call) from
    noise_pred [cfg*F, HW, ldn]; coef [F,16] fp32 rows from scheduler.step_rows."""
    dt, F, HW = _cfg_step_inputs(latents, noise_pred, coef, is_cond, frame_idx)
    assert 1 <= len(states) <= 3 and coef.shape[-1] == 16 and coef.is_contiguous()
    for t in states:
        _req(t, "state", dt)
        assert t.shape == latents.shape and t.is_contiguous()
    st = list(states) + [None] * (3 - len(states))
    _l.call("dm4d_cfg_multistep_step_f32" if dt == F32 else "dm4d_cfg_multistep_step_bf16", _stream(), _p(latents), _p(st[0]), _p(st[1]),
            _p(st[2]), _p(noise_pred), noise_pred.stride(-2), _p(coef), _p(is_cond), _p(frame_idx), F, HW, 1 if use_cfg else 0,
            guidance_scale)
    return latents


def nchw_to_nhwc(x: torch.Tensor, cpad: Optional[int] = None) -> torch.Tensor:
    _req(x, "x")
    assert x.is_contiguous()
    B, C, H, W = x.shape
    cpad = cpad or C
    y = torch.empty((B, H, W, cpad), dtype=BF16, device=x.device)
    _l.call("dm4d_nchw_to_nhwc_bf16", _stream(), _p(x), _p(y), B, C, H * W, cpad)
    return y


def nhwc_to_nchw(x: torch.Tensor, C: Optional[int] = None) -> torch.Tensor:
    dt = F32 if x.dtype == F32 else BF16
    _req(x, "x", dt)
    assert x.is_contiguous()
    B, H, W, ld = x.shape
    C = C or ld
    y = torch.empty((B, C, H, W), dtype=dt, device=x.device)
    _l.call("dm4d_nhwc_to_nchw_f32" if dt == F32 else "dm4d_nhwc_to_nchw_bf16", _stream(), _p(x), _p(y), B, C, H * W, ld)
    return y


def vae_sample(moments: torch.Tensor, noise: torch.Tensor, channels: int, scale: float) -> torch.Tensor:
    """moments [..., >=2C] (mean | logvar), noise [..., C] -> (mean + std * noise) * scale, [..., C]."""
    dt = F32 if moments.dtype == F32 else BF16
    _req(moments, "moments", dt), _req(noise, "noise", dt)
    assert noise.is_contiguous() and noise.shape[-1] == channels
    M = noise.numel() // channels
    out = torch.empty_like(noise)
    _l.call("dm4d_vae_sample_f32" if dt == F32 else "dm4d_vae_sample_bf16", _stream(), _p(moments), moments.stride(-2), _p(noise), _p(out),
            M, channels, scale)
    return out


def scale_pad(x: torch.Tensor, cpad: int, scale: float) -> torch.Tensor:
    _req(x, "x")
    C = x.shape[-1]
    M = x.numel() // C
    assert x.is_contiguous()
    y = torch.empty(x.shape[:-1] + (cpad,), dtype=BF16, device=x.device)
    _l.call("dm4d_scale_pad_bf16", _stream(), _p(x), C, _p(y), cpad, M, C, scale)
    return y


def resize_to_nhwc(x: torch.Tensor, size: Tuple[int, int], mode: str, out_f32: bool = False) -> torch.Tensor:
    """x fp32 NCHW on the device -> bf16 (out_f32: fp32) NHWC [B,h,w,C]; mode 'bilinear' | 'nearest' (F.interpolate semantics)."""
    _req(x, "x", torch.float32)
    assert x.is_contiguous() and mode in ("bilinear", "nearest")
    B, C, H, W = x.shape
    h, w = size
    y = torch.empty((B, h, w, C), dtype=F32 if out_f32 else BF16, device=x.device)
    _l.call("dm4d_resize_nchw_f32_to_nhwc_f32" if out_f32 else "dm4d_resize_nchw_f32_to_nhwc_bf16", _stream(), _p(x), _p(y), B, C, H, W,
            h, w, 1 if mode == "bilinear" else 0)
    return y


def resize_aa(x: torch.Tensor, size: Tuple[int, int]) -> torch.Tensor:
    """F.interpolate(x, size=size, mode="bilinear", antialias=True) for fp32 NCHW on the device (the result writer's mosaic)."""
    _req(x, "x", F32)
    assert x.is_contiguous() and x.ndim == 4
    N, C, H, W = x.shape
    h, w = size
    y = torch.empty((N, C, h, w), dtype=F32, device=x.device)
    _l.call("dm4d_resize_aa_nchw_f32", _stream(), _p(x), _p(y), N * C, H, W, h, w)
    return y


def camera_rows(Ks: torch.Tensor, poses: torch.Tensor) -> torch.Tensor:
    """Per-frame camera constants of dm4d_plucker_latent_bf16, on the host in fp32 as the reference prepares them
    (ray_utils.py:56-59,101-105): [K^-1 | R | T | -R^T T] with [R | T] = inverse(pose)[:3].  -> [N, 24] fp32 (CPU)."""
    Ks, poses = Ks.detach().float().cpu(), poses.detach().float().cpu()
    ext = torch.inverse(poses)
    R, T = ext[:, :3, :3], ext[:, :3, 3:]
    o = -R.mT @ T
    return torch.cat([torch.inverse(Ks).reshape(-1, 9), R.reshape(-1, 9), T.reshape(-1, 3), o.reshape(-1, 3)], dim=1).contiguous()


def plucker_latents(Ks: torch.Tensor, poses: torch.Tensor, image_size: Tuple[int, int], latent_size: Tuple[int, int],
                    device, out_f32: bool = False) -> torch.Tensor:
    """Pluecker maps at latent resolution from the cameras -> bf16 (out_f32: fp32) NHWC [N, h, w, 6] on `device` (see dm4d.h)."""
    cams = camera_rows(Ks, poses).to(device)
    (H, W), (h, w) = image_size, latent_size
    y = torch.empty((cams.shape[0], h, w, 6), dtype=F32 if out_f32 else BF16, device=device)
    _l.call("dm4d_plucker_latent_f32" if out_f32 else "dm4d_plucker_latent_bf16", _stream(), _p(cams), _p(y), cams.shape[0], H, W, h, w)
    return y


def postprocess_images(x: torch.Tensor, channels: int = 3) -> torch.Tensor:
    """NHWC [B,H,W,ld] -> NCHW [B,channels,H,W] with (x/2+0.5).clamp(0,1)."""
    dt = F32 if x.dtype == F32 else BF16
    _req(x, "x", dt)
    assert x.is_contiguous()
    B, H, W, ld = x.shape
    y = torch.empty((B, channels, H, W), dtype=dt, device=x.device)
    _l.call("dm4d_postprocess_images_f32" if dt == F32 else "dm4d_postprocess_images_bf16", _stream(), _p(x), _p(y), B, channels, H * W, ld)
    return y


def _capture_resize_args(blob: torch.Tensor, blob_host: torch.Tensor, n_frames: int, desc_off: int, tab_off: int, tab_len: int, W: int,
                         meta: Optional[torch.Tensor]):
    """The checks of capture_crop_resize / capture_crop_resize_packed and the arguments their entries share, up to scratch_bytes ->
    (the arguments, the tensors that must outlive the call's launches)."""
    _req(blob, "blob", torch.uint8)
    where = blob if meta is None else _req(meta, "meta", torch.uint8)
    _check_meta(where, blob_host, CAPTURE_FIELDS, n_frames, desc_off, tab_off, tab_len, what="blob" if meta is None else "meta")
    if where.device != blob.device or not blob.is_contiguous():
        raise _l.Dm4dError("meta: expected a contiguous tensor on blob's device")
    desc = blob_host[desc_off: desc_off + n_frames * CAPTURE_FIELDS * 8].view(torch.int64).reshape(n_frames, CAPTURE_FIELDS)
    tab = blob_host[tab_off: tab_off + tab_len * 4].view(torch.int32)
    scratch_bytes = int((desc[:, 13] + desc[:, 15] * W * 8).max())
    scratch = torch.empty(max(scratch_bytes, 16), dtype=torch.uint8, device=blob.device)
    base = where.data_ptr()
    return (_stream(), blob.data_ptr(), blob.numel(), desc.data_ptr(), base + desc_off, n_frames, tab.data_ptr(), base + tab_off, tab_len,
            _p(scratch), scratch.numel()), (scratch, desc, tab)


def capture_crop_resize(blob: torch.Tensor, blob_host: torch.Tensor, n_frames: int, desc_off: int, tab_off: int, tab_len: int,
                        H: int, W: int, meta: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Crop + Pillow-exact bicubic resize + the dataset's fp32 epilogue of `n_frames` captured frames (host/capture.py) ->
    (pixel_values, skeletons), fp32 [n_frames, 3, H, W] on blob's device.  `blob`: the device copy of the staging buffer
    `blob_host` (uint8: frame planes | int32 tables at byte `tab_off` | int64 descriptors at byte `desc_off`); the library checks
    every descriptor and table on the host copy before it launches.  With `meta` (uint8, on blob's device) the tables and the
    descriptors are read from it instead, at the same two offsets, `blob_host` is the host copy of `meta`, and `blob` holds
    planes only, some of which may never have been on the host."""
    args, _keep = _capture_resize_args(blob, blob_host, n_frames, desc_off, tab_off, tab_len, W, meta)
    pix = torch.empty((n_frames, 3, H, W), dtype=F32, device=blob.device)
    skel = torch.empty((n_frames, 3, H, W), dtype=F32, device=blob.device)
    _l.call("dm4d_capture_crop_resize_f32", *args, _p(pix), _p(skel), H, W)
    return pix, skel


def _capture_cells(cells_host: torch.Tensor, cells: torch.Tensor, n: int) -> None:
    """`cells_host` is the host int64 [n, CAPTURE_CELL_FIELDS] copy of the device tensor `cells`."""
    _req(cells, "cells", torch.int64)
    if not isinstance(cells_host, torch.Tensor) or cells_host.device.type != "cpu" or cells_host.dtype != torch.int64 or \
            tuple(cells_host.shape) != (n, CAPTURE_CELL_FIELDS) or tuple(cells.shape) != (n, CAPTURE_CELL_FIELDS) or \
            not cells_host.is_contiguous() or not cells.is_contiguous():
        raise _l.Dm4dError(f"cells: expected contiguous int64 [{n}, {CAPTURE_CELL_FIELDS}] descriptors on the device and their host copy")


def capture_crop_resize_packed(blob: torch.Tensor, blob_host: torch.Tensor, n_frames: int, desc_off: int, tab_off: int, tab_len: int,
                               H: int, W: int, cells_host: torch.Tensor, cells: torch.Tensor, meta: Optional[torch.Tensor] = None) -> None:
    """capture_crop_resize up to the epilogue: frame f's resized uint8 pixels {i0 i1 i2 m s0 s1 s2 0} go into the cell that row f of
    the int64 [n_frames, CAPTURE_CELL_FIELDS] descriptors `cells` = {slab address, slab bytes, byte offset of the cell, (unused)}
    names (include/dm4d.h; host/capture_cache.py).  `cells_host`: their host copy, checked by the library before it launches.  The
    slabs are device memory of blob's device that the caller keeps alive.  blob / blob_host / meta as for capture_crop_resize."""
    args, _keep = _capture_resize_args(blob, blob_host, n_frames, desc_off, tab_off, tab_len, W, meta)
    _capture_cells(cells_host, cells, n_frames)
    if cells.device != blob.device:
        raise _l.Dm4dError("cells: expected a tensor on blob's device")
    _l.call("dm4d_capture_crop_resize_packed_u8", *args, cells_host.data_ptr(), _p(cells), H, W)


def capture_unpack_cells(cells_host: torch.Tensor, cells: torch.Tensor, n_out_rows: int, H: int, W: int,
                         out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The dataset's fp32 epilogue of cells that capture_crop_resize_packed wrote -> (pixel_values, skeletons), fp32 [n_out_rows, 3, H, W]
    on cells' device: row `cells[r, 3]` of both is cell r's sample, bit for bit what capture_crop_resize gives for the frame.  One
    launch on the current stream.  `out`: the two tensors to write into; rows that no descriptor names keep what they hold (without
    `out` they are uninitialised)."""
    n = int(cells_host.shape[0]) if isinstance(cells_host, torch.Tensor) and cells_host.ndim == 2 else 0
    _capture_cells(cells_host, cells, n)
    if out is None:
        out = tuple(torch.empty((n_out_rows, 3, H, W), dtype=F32, device=cells.device) for _ in range(2))
    pix, skel = out
    for t, name in ((pix, "pixel_values"), (skel, "skeletons")):
        _req(t, name, F32)
        if tuple(t.shape) != (n_out_rows, 3, H, W) or not t.is_contiguous() or t.device != cells.device:
            raise _l.Dm4dError(f"{name}: expected a contiguous [{n_out_rows}, 3, {H}, {W}] tensor on cells' device")
    _l.call("dm4d_capture_unpack_cells_f32", _stream(), cells_host.data_ptr(), _p(cells), n, _p(pix), _p(skel), n_out_rows, H, W)
    return pix, skel


def _capture_planes(blob: torch.Tensor, meta: torch.Tensor, meta_host: torch.Tensor, fields: int, n: int, desc_off: int) -> torch.Tensor:
    """The checks that capture_plane_stats and capture_fill_rects share -> the host int64 [n, fields] view of the descriptors."""
    _req(blob, "blob", torch.uint8), _req(meta, "meta", torch.uint8)
    _check_meta(meta, meta_host, fields, n, desc_off)
    if meta.device != blob.device or not blob.is_contiguous() or blob.numel() == 0:
        raise _l.Dm4dError("blob / meta: expected contiguous non-empty tensors on one device")
    return meta_host[desc_off: desc_off + n * fields * 8].view(torch.int64).reshape(n, fields)


def capture_plane_stats(blob: torch.Tensor, meta: torch.Tensor, meta_host: torch.Tensor, n: int, desc_off: int) -> torch.Tensor:
    """{first column, first row, last column, last row, sum} of the `n` uint8 planes of `blob` that the int64 CAPTURE_PLANE_FIELDS
    descriptors {byte offset (16-byte aligned), h, w, channels 1 or 3} at byte `desc_off` of `meta` name (host/capture.py) -> int64
    [n, 5] on blob's device; {w, h, -1, -1} for a plane without a non-zero pixel.  `meta_host`: the host copy of `meta`, on which the
    library checks every descriptor before it launches.  Two launches on the current stream; nothing is read back."""
    lib = _l.load()
    desc = _capture_planes(blob, meta, meta_host, _l.CAPTURE_PLANE_FIELDS, n, desc_off)
    nbytes = int(lib.dm4d_capture_plane_stats_ws_bytes(n, int((desc[:, 1] * desc[:, 2] * desc[:, 3]).max())))
    ws = torch.empty(max(nbytes, 8) // 8, dtype=torch.int64, device=blob.device)  # 0: out of range, which the call itself refuses
    out = torch.empty((n, 5), dtype=torch.int64, device=blob.device)
    _l.call("dm4d_capture_plane_stats_u8", _stream(), _p(blob), blob.numel(), desc.data_ptr(), meta.data_ptr() + desc_off, n, _p(out), _p(ws),
            ws.numel() * 8)
    return out


def capture_fill_rects(blob: torch.Tensor, meta: torch.Tensor, meta_host: torch.Tensor, n: int, desc_off: int) -> None:
    """Write the `n` [h, w] uint8 mask planes of `blob` that the int64 CAPTURE_RECT_FIELDS descriptors {byte offset, h, w, c0, r0, c1,
    r1} at byte `desc_off` of `meta` name: 255 on rows r0 .. r1 - 1 and columns c0 .. c1 - 1, 0 elsewhere.  meta / meta_host as for
    capture_plane_stats.  One launch on the current stream."""
    desc = _capture_planes(blob, meta, meta_host, _l.CAPTURE_RECT_FIELDS, n, desc_off)
    _l.call("dm4d_capture_fill_rects_u8", _stream(), _p(blob), blob.numel(), desc.data_ptr(), meta.data_ptr() + desc_off, n)


def eval_psnr_ssim(blob: torch.Tensor, desc: torch.Tensor, desc_off: Optional[int] = None, debug: bool = False):
    """PSNR / SSIM of a batch of image pairs (host/metrics.py; the reference's ImageEvaluator.__call__) -> (out [n, EVAL_OUT] fp64 =
    {psnr, ssim, pred min, pred max, gt min, gt max, squared-error sum, SSIM-map sum}, boxes [n, 4] int32 = the crops used) on blob's
    device, and with `debug` the cropped composites [n, 2, 3, max h, max w] fp32 as a third value.  `blob`: device bytes holding every
    plane; `desc`: HOST int64 [n, EVAL_FIELDS] descriptors (include/dm4d.h), which the library checks before it launches; `desc_off`:
    byte offset of the same descriptors inside blob (they went up with it), or None: they are uploaded here."""
    lib = _l.load()
    _req(blob, "blob", torch.uint8)
    if desc.device.type != "cpu" or desc.dtype != torch.int64 or desc.dim() != 2 or desc.shape[1] != EVAL_FIELDS or not desc.is_contiguous():
        raise _l.Dm4dError(f"desc: expected a contiguous host int64 [n, {EVAL_FIELDS}] tensor")
    n = desc.shape[0]
    if desc_off is None:
        desc_dev = desc.to(blob.device)  # alive until the launches are queued: same-stream allocator order keeps it valid after
        desc_ptr = desc_dev.data_ptr()
    else:
        if desc_off < 0 or desc_off % 8 or desc_off + desc.numel() * 8 > blob.numel():
            raise _l.Dm4dError("desc_off: the descriptors lie outside the blob")
        desc_ptr = blob.data_ptr() + desc_off
    max_h, max_w = (int(desc[:, 6].max()), int(desc[:, 7].max())) if n else (0, 0)
    ws = torch.empty(max(int(lib.dm4d_eval_ws_bytes(n, max_h, max_w)), 16), dtype=torch.uint8, device=blob.device)
    out = torch.empty((n, EVAL_OUT), dtype=torch.float64, device=blob.device)
    boxes = torch.empty((n, 4), dtype=torch.int32, device=blob.device)
    dbg = torch.zeros((n, 2, 3, max(max_h, 1), max(max_w, 1)), dtype=F32, device=blob.device) if debug else None
    _l.call("dm4d_eval_psnr_ssim_f64", _stream(), blob.data_ptr(), blob.numel(), desc.data_ptr(), desc_ptr, n, _p(ws), ws.numel(), _p(out),
            _p(boxes), _p(dbg), max_h, max_w)
    return (out, boxes, dbg) if debug else (out, boxes)


def lpips_input(gt: torch.Tensor, pred: torch.Tensor) -> torch.Tensor:
    """LPIPS' input scaling of one pair of cropped composites (fp32 [3, h, w] views with one row / plane stride, in [0, 1]) -> the operand
    of VGG's first convolution, bf16 [2, h, w, LPIPS_IN_COLS] = [hi(3) | lo(3) | hi(3) | zeros] (0 = gt, 1 = pred)."""
    _req(gt, "gt", F32), _req(pred, "pred", F32)
    if gt.dim() != 3 or gt.shape[0] != 3 or gt.shape != pred.shape:
        raise _l.Dm4dError(f"lpips_input: expected two fp32 [3, h, w] images of one shape, got {tuple(gt.shape)} and {tuple(pred.shape)}")
    if gt.stride() != pred.stride():
        gt, pred = gt.contiguous(), pred.contiguous()
    _, h, w = gt.shape
    y = torch.empty((2, h, w, LPIPS_IN_COLS), dtype=BF16, device=gt.device)
    _l.call("dm4d_lpips_input_split", _stream(), _p(gt), _p(pred), gt.stride(0), gt.stride(1), h, w, _p(y))
    return y


def lpips_relu_pool(x: torch.Tensor, pool: bool) -> torch.Tensor:
    """ReLU (+ the 2 x 2 stride-2 floor max-pool) of a convolution's fp32 output [B, H, W, C] -> the pattern-1 operand of the next
    convolution, bf16 [B, Ho, Wo, 3 C] = [hi | lo | hi]."""
    _req(x, "x", F32)
    assert x.dim() == 4 and x.is_contiguous()
    B, H, W, C = x.shape
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    y = torch.empty((B, Ho, Wo, 3 * C), dtype=BF16, device=x.device)
    with _Prof("lpips_relu_pool", 4.0 * x.numel() + 2.0 * y.numel(), "byte", B * Ho * Wo):
        _l.call("dm4d_lpips_relu_pool_split", _stream(), _p(x), _p(y), B, H, W, C, 1 if pool else 0)
    return y


def lpips_ws(h: int, w: int, device) -> torch.Tensor:
    """The workspace of lpips_tap_distance for taps of up to h x w pixels (one per forward: the taps run one after another)."""
    return torch.empty(max(int(_l.load().dm4d_lpips_ws_bytes(h, w)), 16), dtype=torch.uint8, device=device)


def lpips_tap_distance(f: torch.Tensor, lin: torch.Tensor, tap: int, out: torch.Tensor, ws: torch.Tensor) -> None:
    """One LPIPS tap: f fp32 [2, H, W, C] (a convolution's output before ReLU), lin fp32 [C] -> out[tap] = the tap's distance (out: fp64
    [LPIPS_TAPS] on the device); ws: lpips_ws(H, W) or larger."""
    _req(f, "f", F32), _req(lin, "lin", F32), _req(out, "out", torch.float64), _req(ws, "ws", torch.uint8)
    assert f.dim() == 4 and f.shape[0] == 2 and f.is_contiguous() and lin.numel() == f.shape[3] and out.numel() == LPIPS_TAPS
    _, H, W, C = f.shape
    with _Prof("lpips_distance", 4.0 * f.numel(), "byte", H * W):
        _l.call("dm4d_lpips_tap_distance_f64", _stream(), _p(f), _p(lin), H, W, C, tap, _p(ws), ws.numel(), _p(out))


def vhull_pack_masks(masks: torch.Tensor) -> torch.Tensor:
    """Foreground masks bool or uint8 [B, H, W] (nonzero = foreground) -> bits int32 [B, H, ceil(W / 32)]: pixel x of a row is bit x & 31 of
    its word x >> 5 (what vhull_carve_chunk reads)."""
    if isinstance(masks, torch.Tensor) and masks.dtype == torch.bool:
        masks = masks.view(torch.uint8)
    _req(masks, "masks", torch.uint8)
    if masks.dim() != 3 or not masks.is_contiguous():
        raise _l.Dm4dError(f"masks: expected a contiguous [B, H, W] tensor, got {tuple(masks.shape)}")
    B, H, W = masks.shape
    bits = torch.empty((B, H, (W + 31) // 32), dtype=torch.int32, device=masks.device)
    _l.call("dm4d_vhull_pack_masks", _stream(), _p(masks), _p(bits), B, H, W)
    return bits


def vhull_pack_masks_u8(masks: torch.Tensor, threshold: int = 128) -> torch.Tensor:
    """Gray masks uint8 [B, H, W] (decoded mode-L files) -> the bits of vhull_pack_masks(masks >= threshold), without the bool tensor."""
    _req(masks, "masks", torch.uint8)
    if masks.dim() != 3 or not masks.is_contiguous():
        raise _l.Dm4dError(f"masks: expected a contiguous [B, H, W] tensor, got {tuple(masks.shape)}")
    B, H, W = masks.shape
    bits = torch.empty((B, H, (W + 31) // 32), dtype=torch.int32, device=masks.device)
    _l.call("dm4d_vhull_pack_masks_u8", _stream(), _p(masks), _p(bits), B, H, W, int(threshold))
    return bits


def vhull_ws(n_voxels: int, device) -> torch.Tensor:
    """The workspace of vhull_carve_chunk for chunks of up to n_voxels voxels (reused from chunk to chunk)."""
    nbytes = int(_l.load().dm4d_vhull_ws_bytes(n_voxels))
    if nbytes == 0:
        raise _l.Dm4dError(f"vhull_ws: a chunk holds 1 to {VHULL_MAX_CHUNK} voxels, got {n_voxels}")
    return torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=device)


def vhull_carve_chunk(xs: torch.Tensor, ys: torch.Tensor, zs: torch.Tensor, P: torch.Tensor, bits: torch.Tensor, hw: Tuple[int, int],
                      min_views: int, first: int, n_voxels: int, ws: torch.Tensor, total: torch.Tensor, out: torch.Tensor) -> None:
    """Carve the voxels [first, first + n_voxels) of the grid xs x ys x zs (fp32 axes, z fastest) against B views: P fp64 [B, 3, 4],
    bits = vhull_pack_masks of the [B, H, W] masks, hw = (H, W); min_views 0 = every view.  The kept centres are appended to out (fp32
    [capacity, 3]) at the running count total (int64 [1], zeroed by the caller before a frame's first chunk), which grows by their number
    even where out is full.  Three launches on the current stream, no synchronisation."""
    for t, name in ((xs, "xs"), (ys, "ys"), (zs, "zs"), (out, "out")):
        _req(t, name, F32)
    _req(P, "P", torch.float64), _req(bits, "bits", torch.int32), _req(ws, "ws", torch.int64), _req(total, "total", torch.int64)
    H, W = hw
    B = P.shape[0]
    if P.dim() != 3 or tuple(P.shape[1:]) != (3, 4) or not P.is_contiguous():
        raise _l.Dm4dError(f"P: expected a contiguous [B, 3, 4] tensor, got {tuple(P.shape)}")
    if tuple(bits.shape) != (B, H, (W + 31) // 32) or not bits.is_contiguous():
        raise _l.Dm4dError(f"bits: expected a contiguous [{B}, {H}, {(W + 31) // 32}] tensor, got {tuple(bits.shape)}")
    if xs.dim() != 1 or ys.dim() != 1 or zs.dim() != 1 or total.numel() != 1:
        raise _l.Dm4dError("xs, ys, zs: expected one-dimensional axes; total: expected one element")
    if out.dim() != 2 or out.shape[1] != 3 or not out.is_contiguous():
        raise _l.Dm4dError(f"out: expected a contiguous [capacity, 3] tensor, got {tuple(out.shape)}")
    _l.call("dm4d_vhull_carve_chunk", _stream(), _p(xs), _p(ys), _p(zs), xs.numel(), ys.numel(), zs.numel(), _p(P), _p(bits), B, H, W,
            int(min_views), int(first), int(n_voxels), _p(ws), ws.numel() * 8, _p(total), _p(out) if out.shape[0] else None, out.shape[0])


def _cameras(K: torch.Tensor, T: torch.Tensor) -> int:
    _req(K, "K", torch.float64), _req(T, "T", torch.float64)
    if K.dim() != 3 or tuple(K.shape[1:]) != (3, 3) or not K.is_contiguous():
        raise _l.Dm4dError(f"K: expected a contiguous [n, 3, 3] tensor, got {tuple(K.shape)}")
    if tuple(T.shape) != (K.shape[0], 4, 4) or not T.is_contiguous():
        raise _l.Dm4dError(f"T: expected a contiguous [{K.shape[0]}, 4, 4] tensor, got {tuple(T.shape)}")
    return K.shape[0]


def triangulate_points(K: torch.Tensor, T: torch.Tensor, kp2d: torch.Tensor, score: torch.Tensor, thr: torch.Tensor,
                       min_views: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """K fp64 [n, 3, 3], T fp64 [n, 4, 4] (world -> camera), kp2d fp64 [F, n, k, 2], score fp64 [F, n, k], thr fp64 [F, k] (the score
    threshold of each frame and keypoint) -> kp3d fp64 [F, k, 3], reproj fp64 [F, k], n_views int32 [F, k]; -1e6 in kp3d and reproj where
    fewer than min_views views reach the threshold.  One launch on the current stream."""
    n = _cameras(K, T)
    _req(kp2d, "kp2d", torch.float64), _req(score, "score", torch.float64), _req(thr, "thr", torch.float64)
    if kp2d.dim() != 4 or kp2d.shape[1] != n or kp2d.shape[3] != 2 or not kp2d.is_contiguous():
        raise _l.Dm4dError(f"kp2d: expected a contiguous [F, {n}, k, 2] tensor, got {tuple(kp2d.shape)}")
    F, _, k, _ = kp2d.shape
    if tuple(score.shape) != (F, n, k) or not score.is_contiguous():
        raise _l.Dm4dError(f"score: expected a contiguous [{F}, {n}, {k}] tensor, got {tuple(score.shape)}")
    if tuple(thr.shape) != (F, k) or not thr.is_contiguous():
        raise _l.Dm4dError(f"thr: expected a contiguous [{F}, {k}] tensor, got {tuple(thr.shape)}")
    kp3d = torch.empty((F, k, 3), dtype=torch.float64, device=kp2d.device)
    reproj = torch.empty((F, k), dtype=torch.float64, device=kp2d.device)
    n_views = torch.empty((F, k), dtype=torch.int32, device=kp2d.device)
    _l.call("dm4d_triangulate_points_f64", _stream(), _p(K), _p(T), _p(kp2d), _p(score), _p(thr), F, n, k, int(min_views), _p(kp3d),
            _p(reproj), _p(n_views))
    return kp3d, reproj, n_views


def project_points(kp3d: torch.Tensor, K: torch.Tensor, T: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """kp3d fp64 [F, k, 3], K fp64 [m, 3, 3], T fp64 [m, 4, 4] -> kp2d fp64 [F, m, k, 2], depth fp64 [F, m, k]; a point holding -1e6 gives
    -1e6 in both for every camera."""
    _req(kp3d, "kp3d", torch.float64)
    m = _cameras(K, T)
    if kp3d.dim() != 3 or kp3d.shape[2] != 3 or not kp3d.is_contiguous():
        raise _l.Dm4dError(f"kp3d: expected a contiguous [F, k, 3] tensor, got {tuple(kp3d.shape)}")
    F, k, _ = kp3d.shape
    kp2d = torch.empty((F, m, k, 2), dtype=torch.float64, device=kp3d.device)
    depth = torch.empty((F, m, k), dtype=torch.float64, device=kp3d.device)
    _l.call("dm4d_project_points_f64", _stream(), _p(kp3d), _p(K), _p(T), F, m, k, _p(kp2d), _p(depth))
    return kp2d, depth


def skeleton_draw(prims_host: torch.Tensor, prims: torch.Tensor, offsets_host: torch.Tensor, offsets: torch.Tensor, htab_host: torch.Tensor,
                  htab: torch.Tensor, hk: int, vtab_host: torch.Tensor, vtab: torch.Tensor, vk: int, H: int, W: int, h: int,
                  w: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Skeleton maps of a batch of frames -> uint8 [B, h, w, 3] on prims' device, one launch on the current stream (host/skeleton.py).
    prims int32 [n, SKEL_FIELDS] draw records, offsets int32 [B + 1] the frames' ranges in it, htab / vtab int32 bicubic tables of
    the canvas (H, W) -> (h, w) with hk / vk taps per window; every *_host tensor is the host copy of its device twin, on which the
    library checks counts, records and windows before it launches.  `out`: a contiguous uint8 [B, h, w, 3] tensor on prims' device to
    draw into (a view of a larger buffer is fine: no alignment is asked of it); by default one is allocated."""
    for name, dev, host in (("prims", prims, prims_host), ("offsets", offsets, offsets_host), ("htab", htab, htab_host), ("vtab", vtab, vtab_host)):
        _req(dev, name, torch.int32)
        if not isinstance(host, torch.Tensor) or host.device.type != "cpu" or host.dtype != torch.int32 or host.shape != dev.shape:
            raise _l.Dm4dError(f"{name}_host: expected the host copy of {name}")
        if not dev.is_contiguous() or not host.is_contiguous():
            raise _l.Dm4dError(f"{name}: expected contiguous tensors")
    if prims.dim() != 2 or prims.shape[1] != SKEL_FIELDS or prims.shape[0] < 1:
        raise _l.Dm4dError(f"prims: expected [n >= 1, {SKEL_FIELDS}], got {tuple(prims.shape)}")
    B = offsets.numel() - 1
    if offsets.dim() != 1 or B < 1 or int(offsets_host[-1]) > prims.shape[0]:
        raise _l.Dm4dError("offsets: expected [B + 1] with the last entry inside prims")
    if htab.numel() != w * (2 + hk) or vtab.numel() != h * (2 + vk):
        raise _l.Dm4dError(f"htab / vtab: expected {w} x (2 + {hk}) and {h} x (2 + {vk}) entries, got {htab.numel()} and {vtab.numel()}")
    if out is None:
        out = torch.empty((B, h, w, 3), dtype=torch.uint8, device=prims.device)
    else:
        _req(out, "out", torch.uint8)
        if tuple(out.shape) != (B, h, w, 3) or not out.is_contiguous() or out.device != prims.device:
            raise _l.Dm4dError(f"out: expected a contiguous [{B}, {h}, {w}, 3] tensor on {prims.device}, got {tuple(out.shape)} on {out.device}")
    _l.call("dm4d_skeleton_draw_u8", _stream(), prims_host.data_ptr(), _p(prims), offsets_host.data_ptr(), _p(offsets), B, htab_host.data_ptr(),
            _p(htab), int(hk), vtab_host.data_ptr(), _p(vtab), int(vk), int(H), int(W), int(h), int(w), _p(out))
    return out


def _host_twin(dev: torch.Tensor, host, name: str, dtype, shape) -> None:
    """`dev` is a contiguous `dtype` tensor of `shape` on a HIP device and `host` the host copy of it."""
    _req(dev, name, dtype)
    if tuple(dev.shape) != tuple(shape) or not dev.is_contiguous():
        raise _l.Dm4dError(f"{name}: expected a contiguous {list(shape)} tensor, got {tuple(dev.shape)}")
    if not isinstance(host, torch.Tensor) or host.device.type != "cpu" or host.dtype != dtype or host.shape != dev.shape or not host.is_contiguous():
        raise _l.Dm4dError(f"{name}_host: expected the host copy of {name}")


def skeleton_plan_kp3d(kp3d: torch.Tensor, K: torch.Tensor, T: torch.Tensor, jobs_host: torch.Tensor, jobs: torch.Tensor,
                       scores: Optional[torch.Tensor], scale_host: torch.Tensor, scale: torch.Tensor, sizes_host: torch.Tensor,
                       sizes: torch.Tensor, links_host: torch.Tensor, links: torch.Tensor, colors_host: torch.Tensor, colors: torch.Tensor,
                       low_thr: float, high_thr: float, thr_span: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Draw plans of n maps straight from 3-D keypoints, one launch on the current stream (dm4d_skeleton_plan_kp3d, include/dm4d.h) ->
    (records int32 [n, 3 L, SKEL_FIELDS], counts int32 [n], status int32 [n, 2] = {flag bits, dropped links}) on kp3d's device.
    kp3d fp64 [F, k, 3], K fp64 [m, 3, 3], T fp64 [m, 4, 4]; jobs int32 [n, 2] = {frame, camera}; scores fp32 [n, k] or None; scale
    fp64 [n, 2] = {scale_ratio, offset}; sizes int32 [n, 2] = {radius, thickness}; links int32 [L, SKEL_LINK_FIELDS]; colors fp32
    [k + L, 4]; every *_host tensor is the host copy of its device twin, which the library validates before it launches."""
    _req(kp3d, "kp3d", torch.float64)
    m = _cameras(K, T)
    if kp3d.dim() != 3 or kp3d.shape[2] != 3 or not kp3d.is_contiguous():
        raise _l.Dm4dError(f"kp3d: expected a contiguous [F, k, 3] tensor, got {tuple(kp3d.shape)}")
    F, k, _ = kp3d.shape
    n = jobs.shape[0] if isinstance(jobs, torch.Tensor) and jobs.dim() == 2 else 0
    L = links.shape[0] if isinstance(links, torch.Tensor) and links.dim() == 2 else 0
    if n < 1 or L < 1:
        raise _l.Dm4dError("jobs / links: expected [n >= 1, 2] and [L >= 1, SKEL_LINK_FIELDS]")
    _host_twin(jobs, jobs_host, "jobs", torch.int32, (n, 2))
    _host_twin(scale, scale_host, "scale", torch.float64, (n, 2))
    _host_twin(sizes, sizes_host, "sizes", torch.int32, (n, 2))
    _host_twin(links, links_host, "links", torch.int32, (L, SKEL_LINK_FIELDS))
    _host_twin(colors, colors_host, "colors", F32, (k + L, 4))
    if scores is not None:
        _req(scores, "scores", F32)
        if tuple(scores.shape) != (n, k) or not scores.is_contiguous():
            raise _l.Dm4dError(f"scores: expected a contiguous [{n}, {k}] tensor, got {tuple(scores.shape)}")
    if 3 * L > SKEL_MAX_PRIMS:
        raise _l.Dm4dError(f"links: 3 x {L} records a map exceed SKEL_MAX_PRIMS = {SKEL_MAX_PRIMS}")
    records = torch.empty((n, 3 * L, SKEL_FIELDS), dtype=torch.int32, device=kp3d.device)
    counts = torch.empty((n,), dtype=torch.int32, device=kp3d.device)
    status = torch.empty((n, 2), dtype=torch.int32, device=kp3d.device)
    _l.call("dm4d_skeleton_plan_kp3d", _stream(), _p(kp3d), _p(K), _p(T), F, m, k, jobs_host.data_ptr(), _p(jobs), n, _p(scores),
            scale_host.data_ptr(), _p(scale), sizes_host.data_ptr(), _p(sizes), links_host.data_ptr(), _p(links), L, colors_host.data_ptr(),
            _p(colors), float(low_thr), float(high_thr), float(thr_span), _p(records), _p(counts), _p(status))
    return records, counts, status


def skeleton_draw_planned(records: torch.Tensor, counts: torch.Tensor, htab_host: torch.Tensor, htab: torch.Tensor, hk: int,
                          vtab_host: torch.Tensor, vtab: torch.Tensor, vk: int, H: int, W: int, h: int, w: int,
                          out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """skeleton_draw on plans that skeleton_plan_kp3d left on the device: records int32 [B, 3 L, SKEL_FIELDS] and counts int32 [B]
    (contiguous; a slice along B of the plan's tensors is fine) -> uint8 [B, h, w, 3], one launch on the current stream.  Tables and
    `out` as skeleton_draw takes them."""
    _req(records, "records", torch.int32), _req(counts, "counts", torch.int32)
    if records.dim() != 3 or records.shape[2] != SKEL_FIELDS or records.shape[0] < 1 or not records.is_contiguous():
        raise _l.Dm4dError(f"records: expected a contiguous [B >= 1, 3 L, {SKEL_FIELDS}] tensor, got {tuple(records.shape)}")
    B, stride, _ = records.shape
    if tuple(counts.shape) != (B,) or not counts.is_contiguous() or counts.device != records.device:
        raise _l.Dm4dError(f"counts: expected a contiguous [{B}] tensor on {records.device}, got {tuple(counts.shape)}")
    for name, dev, host in (("htab", htab, htab_host), ("vtab", vtab, vtab_host)):
        _req(dev, name, torch.int32)
        _host_twin(dev, host, name, torch.int32, dev.shape)
    if htab.numel() != w * (2 + hk) or vtab.numel() != h * (2 + vk):
        raise _l.Dm4dError(f"htab / vtab: expected {w} x (2 + {hk}) and {h} x (2 + {vk}) entries, got {htab.numel()} and {vtab.numel()}")
    if out is None:
        out = torch.empty((B, h, w, 3), dtype=torch.uint8, device=records.device)
    else:
        _req(out, "out", torch.uint8)
        if tuple(out.shape) != (B, h, w, 3) or not out.is_contiguous() or out.device != records.device:
            raise _l.Dm4dError(f"out: expected a contiguous [{B}, {h}, {w}, 3] tensor on {records.device}, got {tuple(out.shape)} on {out.device}")
    _l.call("dm4d_skeleton_draw_planned_u8", _stream(), _p(records), _p(counts), B, int(stride), htab_host.data_ptr(), _p(htab), int(hk),
            vtab_host.data_ptr(), _p(vtab), int(vk), int(H), int(W), int(h), int(w), _p(out))
    return out


def skeleton_box_mask(maps: torch.Tensor, pads: Tuple[int, int, int], masks: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Bounding boxes and box masks of drawn maps (crop_utils.py skeleton_to_mask; host/capture.py) -> (boxes int32 [B, 4] = {first
    column, first row, last column, last row} of the pixels with a non-zero channel, {w, h, -1, -1} for a map without one; masks uint8
    [B, h, w]: 255 inside the box grown by 1 + pads and clamped to the map, 0 outside), both on maps' device.  maps: contiguous uint8
    [B, h, w, 3]; pads = (pad_top, pad_bottom, pad_x); `masks`: a contiguous uint8 [B, h, w] tensor to fill (a view of a larger buffer
    is fine), by default one is allocated.  Three launches on the current stream; nothing is read back."""
    lib = _l.load()
    _req(maps, "maps", torch.uint8)
    if maps.dim() != 4 or maps.shape[3] != 3 or maps.shape[0] < 1 or not maps.is_contiguous():
        raise _l.Dm4dError(f"maps: expected a contiguous [B >= 1, h, w, 3] tensor, got {tuple(maps.shape)}")
    B, h, w, _ = maps.shape
    if masks is None:
        masks = torch.empty((B, h, w), dtype=torch.uint8, device=maps.device)
    else:
        _req(masks, "masks", torch.uint8)
        if tuple(masks.shape) != (B, h, w) or not masks.is_contiguous() or masks.device != maps.device:
            raise _l.Dm4dError(f"masks: expected a contiguous [{B}, {h}, {w}] tensor on {maps.device}, got {tuple(masks.shape)} on {masks.device}")
    pad_top, pad_bottom, pad_x = (int(v) for v in pads)
    nbytes = int(lib.dm4d_skeleton_box_mask_ws_bytes(B, h, w))
    if nbytes == 0:
        raise _l.Dm4dError(f"skeleton_box_mask: shape {tuple(maps.shape)} is out of range")
    ws = torch.empty(nbytes // 4, dtype=torch.int32, device=maps.device)
    boxes = torch.empty((B, 4), dtype=torch.int32, device=maps.device)
    _l.call("dm4d_skeleton_box_mask_u8", _stream(), _p(maps), B, h, w, pad_top, pad_bottom, pad_x, _p(boxes), _p(masks), h * w, _p(ws), nbytes)
    return boxes, masks


def _pose_blob(blob: torch.Tensor, meta: torch.Tensor) -> None:
    _req(blob, "blob", torch.uint8), _req(meta, "meta", torch.uint8)
    if meta.device != blob.device or not blob.is_contiguous() or blob.numel() == 0:
        raise _l.Dm4dError("blob / meta: expected contiguous non-empty tensors on one device")


def pose_input(blob: torch.Tensor, meta: torch.Tensor, meta_host: torch.Tensor, rows: int, desc_off: int, tab_off: int, tab_len: int,
               H: int, W: int, norm: torch.Tensor) -> torch.Tensor:
    """The pose network's input for `rows` (image, box) pairs (host/pose.py) -> fp32 [rows, 3, H, W] on blob's device, one launch on the
    current stream.  `blob`: device uint8 holding the image and mask planes; `meta`: device uint8 holding int32 warp tables at byte
    `tab_off` and int64 POSE_FIELDS descriptors at byte `desc_off`, `meta_host` its host copy, on which the library checks every
    descriptor and table before it launches.  norm: host fp32 [6] = mean R, G, B | std R, G, B."""
    _pose_blob(blob, meta)
    _check_meta(meta, meta_host, _l.POSE_FIELDS, rows, desc_off, tab_off, tab_len)
    if norm.device.type != "cpu" or norm.dtype != F32 or norm.numel() != 6 or not norm.is_contiguous():
        raise _l.Dm4dError("norm: expected a contiguous host fp32 tensor of 6 values")
    out = torch.empty((rows, 3, H, W), dtype=F32, device=blob.device)
    host, dev = meta_host.data_ptr(), meta.data_ptr()
    _l.call("dm4d_pose_input_u8_f32", _stream(), _p(blob), blob.numel(), host + desc_off, dev + desc_off, rows, host + tab_off, dev + tab_off,
            tab_len, norm.data_ptr(), _p(out), H, W)
    return out


def pose_mask_box(blob: torch.Tensor, meta: torch.Tensor, meta_host: torch.Tensor, n: int, desc_off: int) -> torch.Tensor:
    """[x1, y1, x2, y2] of the pixels >= 128 of the masks that `n` POSE_FIELDS descriptors at byte `desc_off` of meta name ({0, 0, w, h}
    for a mask without one) -> int32 [n, 4] on blob's device; blob / meta / meta_host as for pose_input.  One launch on the current stream."""
    _pose_blob(blob, meta)
    _check_meta(meta, meta_host, _l.POSE_FIELDS, n, desc_off)
    boxes = torch.empty((n, 4), dtype=torch.int32, device=blob.device)
    _l.call("dm4d_pose_mask_box_u8", _stream(), _p(blob), blob.numel(), meta_host.data_ptr() + desc_off, meta.data_ptr() + desc_off, n, _p(boxes))
    return boxes


def pose_udp_decode(heatmaps: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """UDP/DARK decode of heatmaps fp32 [n, K, Hh, Wh] (contiguous) -> (locs fp32 [n, K, 2] = refined (x, y) in heatmap pixels, (-1, -1)
    for a map whose maximum is <= 0; scores fp32 [n, K] = each map's maximum), on the heatmaps' device.  One launch on the current stream."""
    _req(heatmaps, "heatmaps", F32)
    if heatmaps.dim() != 4 or not heatmaps.is_contiguous() or heatmaps.numel() == 0:
        raise _l.Dm4dError(f"heatmaps: expected a contiguous non-empty [n, K, Hh, Wh] tensor, got {tuple(heatmaps.shape)}")
    n, K, Hh, Wh = heatmaps.shape
    locs = torch.empty((n, K, 2), dtype=F32, device=heatmaps.device)
    scores = torch.empty((n, K), dtype=F32, device=heatmaps.device)
    _l.call("dm4d_pose_udp_decode_f32", _stream(), _p(heatmaps), n, K, Hh, Wh, _p(scores), _p(locs))
    return locs, scores


def detect_input(blob: torch.Tensor, meta: torch.Tensor, meta_host: torch.Tensor, n: int, desc_off: int, tab_off: int, tab_len: int,
                 H: int, W: int, norm: torch.Tensor, pad_value: int, bgr: bool) -> torch.Tensor:
    """The detector's input for `n` staged images (host/detect.py) -> fp32 [n, 3, H, W] on blob's device, one launch on the current
    stream.  blob / meta / meta_host as for pose_input, the tables being the resize tables of include/dm4d.h (dm4d_detect_input_u8_f32).
    norm: host fp32 [6] = mean | std per output plane; bgr: plane c is the staged channel 2 - c."""
    _pose_blob(blob, meta)
    _check_meta(meta, meta_host, _l.POSE_FIELDS, n, desc_off, tab_off, tab_len)
    if norm.device.type != "cpu" or norm.dtype != F32 or norm.numel() != 6 or not norm.is_contiguous():
        raise _l.Dm4dError("norm: expected a contiguous host fp32 tensor of 6 values")
    out = torch.empty((n, 3, H, W), dtype=F32, device=blob.device)
    host, dev = meta_host.data_ptr(), meta.data_ptr()
    _l.call("dm4d_detect_input_u8_f32", _stream(), _p(blob), blob.numel(), host + desc_off, dev + desc_off, n, host + tab_off, dev + tab_off,
            tab_len, norm.data_ptr(), _p(out), H, W, int(pad_value), int(bool(bgr)))
    return out


def detect_select(boxes: torch.Tensor, scores: torch.Tensor, inv_scale: torch.Tensor, cat: int, score_thr: float, nms_thr: float,
                  max_per_img: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Dense detector output -> kept boxes (include/dm4d.h, dm4d_detect_select_f32): boxes fp32 [n, A, 4], scores fp32 [n, A, C],
    inv_scale fp32 [n, 2], contiguous on one device -> (counts int32 [n, 3] = kept | dropped | above the threshold, fp32
    [n, max_per_img, 5] = x1, y1, x2, y2, score in kept order, int32 [n, max_per_img] anchor indices).  One launch on the current stream."""
    _req(boxes, "boxes", F32), _req(scores, "scores", F32), _req(inv_scale, "inv_scale", F32)
    if boxes.dim() != 3 or boxes.shape[2] != 4 or scores.dim() != 3 or scores.shape[:2] != boxes.shape[:2] or boxes.numel() == 0 or \
            scores.numel() == 0 or tuple(inv_scale.shape) != (boxes.shape[0], 2):
        raise _l.Dm4dError(f"boxes / scores / inv_scale: expected [n, A, 4], [n, A, C] and [n, 2], got {tuple(boxes.shape)}, "
                           f"{tuple(scores.shape)} and {tuple(inv_scale.shape)}")
    if not (boxes.is_contiguous() and scores.is_contiguous() and inv_scale.is_contiguous()) or len({boxes.device, scores.device, inv_scale.device}) != 1:
        raise _l.Dm4dError("boxes / scores / inv_scale: expected contiguous tensors on one device")
    n, A, C = scores.shape
    keep = min(max(int(max_per_img), 1), _l.DETECT_MAX_KEEP)  # the library refuses what is out of range; the results are sized for what it accepts
    counts = torch.empty((n, 3), dtype=torch.int32, device=boxes.device)
    out = torch.empty((n, keep, 5), dtype=F32, device=boxes.device)
    idx = torch.empty((n, keep), dtype=torch.int32, device=boxes.device)
    _l.call("dm4d_detect_select_f32", _stream(), _p(boxes), _p(scores), _p(inv_scale), n, A, C, int(cat), float(score_thr), float(nms_thr),
            int(max_per_img), _p(counts), _p(out), _p(idx))
    return counts, out, idx


def matting_input(blob: torch.Tensor, meta: torch.Tensor, meta_host: torch.Tensor, n: int, desc_off: int, tab_off: int, tab_len: int,
                  lut: torch.Tensor, scratch: torch.Tensor, S_h: int, S_w: int, rot: int) -> torch.Tensor:
    """The matting network's input for `n` staged images (host/matting.py) -> lut's dtype (fp16 or fp32) [n, 3, S_h, S_w] on blob's
    device, at most two launches on the current stream.  `blob`: device uint8 holding the RGB planes; `meta`: device uint8 holding
    int32 coefficient tables at byte `tab_off` and int64 MATTING_FIELDS descriptors at byte `desc_off`, `meta_host` its host copy, on
    which the library checks every descriptor and table before it launches.  lut: device [3, 256], the normalisation of every byte;
    scratch: device uint8 for the horizontal pass; rot: quarter turns clockwise."""
    _req(blob, "blob", torch.uint8), _req(scratch, "scratch", torch.uint8), _req(meta, "meta", torch.uint8)
    _check_meta(meta, meta_host, _l.MATTING_FIELDS, n, desc_off, tab_off, tab_len)
    if lut.dtype not in (F16, F32):
        raise _l.Dm4dError(f"lut: expected fp16 or fp32, got {lut.dtype}")
    _req(lut, "lut", lut.dtype)
    if tuple(lut.shape) != (3, 256) or not lut.is_contiguous() or not blob.is_contiguous() or blob.numel() == 0 or scratch.numel() == 0 or \
            len({blob.device, meta.device, lut.device, scratch.device}) != 1:
        raise _l.Dm4dError("blob / meta / lut / scratch: expected contiguous non-empty tensors on one device, lut [3, 256]")
    out = torch.empty((n, 3, S_h, S_w), dtype=lut.dtype, device=blob.device)
    host, dev = meta_host.data_ptr(), meta.data_ptr()
    _l.call("dm4d_matting_input_u8", _stream(), _p(blob), blob.numel(), host + desc_off, dev + desc_off, n, host + tab_off, dev + tab_off,
            tab_len, _p(lut), _p(scratch), scratch.numel(), _p(out), S_h, S_w, rot, int(lut.dtype == F32))
    return out


def matting_mask(logits: torch.Tensor, meta: torch.Tensor, meta_host: torch.Tensor, n: int, desc_off: int, tab_off: int, tab_len: int,
                 qtab: torch.Tensor, scratch: torch.Tensor, blob_bytes: int, rot: int) -> torch.Tensor:
    """fp16 logits [n, 1, S_h, S_w] (contiguous) -> the packed uint8 masks of `n` images, `blob_bytes` bytes on the logits' device, at
    most two launches on the current stream.  meta / meta_host as for matting_input (a descriptor's first field: the mask's 16-byte
    aligned offset in the result).  qtab: device uint8 [65536], fp16 bit pattern -> byte; scratch: device uint8 for the horizontal pass."""
    _req(logits, "logits", F16), _req(qtab, "qtab", torch.uint8), _req(scratch, "scratch", torch.uint8), _req(meta, "meta", torch.uint8)
    _check_meta(meta, meta_host, _l.MATTING_FIELDS, n, desc_off, tab_off, tab_len)
    if logits.dim() != 4 or logits.shape[0] != n or logits.shape[1] != 1 or not logits.is_contiguous() or logits.numel() == 0:
        raise _l.Dm4dError(f"logits: expected a contiguous [{n}, 1, S_h, S_w] tensor, got {tuple(logits.shape)}")
    if qtab.numel() != 65536 or not qtab.is_contiguous() or scratch.numel() == 0 or blob_bytes < 1 or \
            len({logits.device, meta.device, qtab.device, scratch.device}) != 1:
        raise _l.Dm4dError("qtab / scratch / meta: expected contiguous tensors on the logits' device, qtab of 65536 bytes")
    blob = torch.empty(blob_bytes, dtype=torch.uint8, device=logits.device)
    host, dev = meta_host.data_ptr(), meta.data_ptr()
    _l.call("dm4d_matting_mask_f16_u8", _stream(), _p(logits), host + desc_off, dev + desc_off, n, host + tab_off, dev + tab_off, tab_len,
            _p(qtab), _p(scratch), scratch.numel(), _p(blob), blob_bytes, int(logits.shape[2]), int(logits.shape[3]), rot)
    return blob


def _encoder_buffers(desc: torch.Tensor, fields: int, dev, blob_bytes: int, ws_bytes: int):
    """What png_encode and webp_encode do around their library call: `desc` is a host int64 [n, fields] tensor -> (n, its device
    copy, the workspace, the blob, the int64 [2 n] result) on `dev`."""
    if desc.device.type != "cpu" or desc.dtype != torch.int64 or desc.dim() != 2 or desc.shape[1] != fields or not desc.is_contiguous() \
            or desc.shape[0] < 1:
        raise _l.Dm4dError(f"desc: expected a contiguous host int64 [n, {fields}] tensor")
    n = int(desc.shape[0])
    return n, desc.to(dev), _workspace(ws_bytes, dev), torch.empty(blob_bytes, dtype=torch.uint8, device=dev), \
        torch.empty(2 * n, dtype=torch.int64, device=dev)


def png_encode(planes: torch.Tensor, rgb: Optional[torch.Tensor], desc: torch.Tensor, blob_bytes: int, ws_bytes: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Complete PNG files of the images that `desc` (host int64 [n, PNG_FIELDS], include/dm4d.h) names in the device uint8 buffers
    `planes` (L planes and alpha planes) and `rgb` (packed RGB images; None when there is no RGBA image) -> (blob of `blob_bytes` on the
    device, device int64 [2 n]: the files' offsets in it, then their lengths).  Five launches on the current stream; nothing is
    synchronised.  The library checks every descriptor against the buffers before it launches."""
    _req(planes, "planes", torch.uint8)
    if rgb is not None:
        _req(rgb, "rgb", torch.uint8)
    if not planes.is_contiguous() or planes.numel() == 0 or (rgb is not None and (not rgb.is_contiguous() or rgb.device != planes.device)):
        raise _l.Dm4dError("planes / rgb: expected contiguous non-empty tensors on one device")
    n, desc_dev, ws, blob, out = _encoder_buffers(desc, _l.PNG_FIELDS, planes.device, blob_bytes, ws_bytes)
    _l.call("dm4d_png_encode_u8", _stream(), _p(planes), planes.numel(), _p(rgb), 0 if rgb is None else rgb.numel(), desc.data_ptr(),
            _p(desc_dev), n, _p(ws), ws.numel() * 8, _p(blob), blob.numel(), _p(out))
    return blob, out


def webp_encode(rgb: torch.Tensor, desc: torch.Tensor, blob_bytes: int, ws_bytes: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Complete lossless WebP files of the packed RGB images that `desc` (host int64 [n, WEBP_FIELDS], include/dm4d.h) names in the device
    uint8 buffer `rgb` -> (blob of `blob_bytes` on the device, device int64 [2 n]: the files' offsets in it, then their lengths).  Five
    launches on the current stream; nothing is synchronised.  The library checks every descriptor against the buffer before it launches."""
    _req(rgb, "rgb", torch.uint8)
    if not rgb.is_contiguous() or rgb.numel() == 0:
        raise _l.Dm4dError("rgb: expected a contiguous non-empty tensor")
    n, desc_dev, ws, blob, out = _encoder_buffers(desc, _l.WEBP_FIELDS, rgb.device, blob_bytes, ws_bytes)
    _l.call("dm4d_webp_encode_u8", _stream(), _p(rgb), rgb.numel(), desc.data_ptr(), _p(desc_dev), n, _p(ws), ws.numel() * 8, _p(blob),
            blob.numel(), _p(out))
    return blob, out


def rectify(blob: torch.Tensor, meta: torch.Tensor, meta_host: torch.Tensor, n: int, desc_off: int, tab_off: int, tab_len: int,
            lut: torch.Tensor, out_bytes: int) -> torch.Tensor:
    """Colour table + undistortion + area resize + crop of `n` staged raw captures (host/rectify.py) -> the packed uint8 RGB results,
    `out_bytes` bytes on blob's device, one launch on the current stream.  `blob`: device uint8 holding the RGB sources; `meta`: device
    uint8 holding the int32 / fp32 tables at byte `tab_off` and the int64 RECTIFY_FIELDS descriptors at byte `desc_off` (a descriptor
    names its result's 16-byte aligned offset), `meta_host` its host copy, on which the library checks every size, offset, window and
    crop before it launches.  lut: device fp32 [n, 3, 256], the colour correction of every byte of every image."""
    _req(blob, "blob", torch.uint8), _req(meta, "meta", torch.uint8), _req(lut, "lut", F32)
    _check_meta(meta, meta_host, _l.RECTIFY_FIELDS, n, desc_off, tab_off, tab_len)
    if tuple(lut.shape) != (n, 3, 256) or not lut.is_contiguous() or not blob.is_contiguous() or blob.numel() == 0 or out_bytes < 1 or \
            len({blob.device, meta.device, lut.device}) != 1:
        raise _l.Dm4dError(f"blob / meta / lut: expected contiguous non-empty tensors on one device, lut [{n}, 3, 256]")
    out = torch.empty(out_bytes, dtype=torch.uint8, device=blob.device)
    host, dev = meta_host.data_ptr(), meta.data_ptr()
    _l.call("dm4d_rectify_u8", _stream(), _p(blob), blob.numel(), host + desc_off, dev + desc_off, n, host + tab_off, dev + tab_off, tab_len,
            _p(lut), _p(out), out_bytes)
    return out
