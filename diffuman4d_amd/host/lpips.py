"""LPIPS-VGG, the reference's third metric (``src/data/utils/metric_utils.py:14-19,134-137``: torchmetrics'
``LearnedPerceptualImagePatchSimilarity(net_type="vgg", normalize=True)``), on the device.

``LpipsVGG(device, vgg16_path, lin_path)`` is the callable ``ImageEvaluator(device, lpips=...)`` expects: ``(gt[None], pred[None]) ->
float`` for fp32 ``[1, 3, h, w]`` composites in [0, 1] on the device.  Per pair (a batch of two images, 0 = ground truth, 1 = prediction):

  input scaling (csrc/lpips.hip) -> 13 x [ReLU (+ max-pool) -> operand (csrc/lpips.hip); 3 x 3 convolution on the MFMA kernel, fp32 out
  (dm4d_conv3x3_nhwc_bf16_flags)] -> per tap: channel normalisation, weighted squared difference, fp64 mean (csrc/lpips.hip) -> their sum.

Arithmetic: VGG's weights are fp32 and its activations unnormalised, so every product has three bf16 terms -- activations
``[hi | lo | hi]`` against weights packed per tap as ``[w_hi | w_hi | w_lo]`` = hi w_hi + lo w_hi + hi w_lo, fp32 accumulation, fp32
bias through the convolution's fp32 row-bias input.  The distances are summed in fp64 in a fixed order: a pair's value is the same bits
on every run, in every batch, and for the two images swapped; identical images give exactly 0.

Weights are neither shipped nor fetched: ``load_lpips_weights`` reads the two files users of the reference already have --
torchvision's VGG-16 checkpoint (``vgg16-397923af.pth``, keys ``features.N.{weight,bias}``) and the LPIPS linear layers (``vgg.pth`` of
the lpips / torchmetrics package, keys ``linN.model.1.weight``).  There is no CPU path: a host tensor or ``device="cpu"`` raises.
"""
from __future__ import annotations

import os
from typing import Dict, List, Tuple

import torch

from . import ops
from .lib import Dm4dError

# torchvision.models.vgg16().features: the indices of the 3 x 3 convolutions, grouped by the tap that follows each group
# (torchmetrics' _LPIPS / Vgg16 slices: relu1_2, relu2_2, relu3_3, relu4_3, relu5_3); a 2 x 2 max-pool precedes every group but the first
VGG_STAGES: Tuple[Tuple[int, ...], ...] = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))
VGG_WIDTHS: Tuple[int, ...] = (64, 128, 256, 512, 512)
# four poolings: an edge of 15 leaves 15 -> 7 -> 3 -> 1 -> 0 pixels for the last tap
MIN_EDGE = 16
# the convolution entry takes tensors below 2^31 elements; the largest here is the 64-channel stage's operand, 2 h w (3 x 64) values
MAX_PIXELS = ((1 << 31) - 1) // (2 * 3 * 64)


def conv_shapes() -> List[Tuple[int, int, int]]:
    """[(features index, Cin, Cout)] of the thirteen convolutions, in order."""
    out, cin = [], 3
    for stage, width in zip(VGG_STAGES, VGG_WIDTHS):
        for idx in stage:
            out.append((idx, cin, width))
            cin = width
    return out


def _read(path) -> Dict[str, torch.Tensor]:
    path = os.fspath(path)
    if not os.path.isfile(path):
        raise FileNotFoundError(f"LPIPS weights: {path} does not exist (nothing is downloaded: pass the file the reference uses)")
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(path, device="cpu")
    sd = torch.load(path, weights_only=True, map_location="cpu")
    if not isinstance(sd, dict):
        raise ValueError(f"{path}: expected a state dict, got {type(sd).__name__}")
    return sd


def _take(sd: Dict[str, torch.Tensor], key: str, shape: Tuple[int, ...], path) -> torch.Tensor:
    if key not in sd:
        raise KeyError(f"{key} is missing in {path}")
    t = sd[key]
    if tuple(t.shape) != shape:
        raise ValueError(f"{key} in {path}: shape {tuple(t.shape)}, expected {shape}")
    return t.detach().to(torch.float32).contiguous()


def load_lpips_weights(vgg16_path, lin_path) -> Dict[str, list]:
    """{"conv": [(weight [Cout, Cin, 3, 3], bias [Cout])] x 13, "lin": [weight [C]] x 5}, fp32 on the host, from torchvision's VGG-16
    checkpoint (``classifier.*`` is ignored) and the LPIPS linear layers; each file ``.pth`` / ``.pt`` or ``.safetensors``."""
    vgg, lin = _read(vgg16_path), _read(lin_path)
    conv = [(_take(vgg, f"features.{i}.weight", (cout, cin, 3, 3), vgg16_path), _take(vgg, f"features.{i}.bias", (cout,), vgg16_path))
            for i, cin, cout in conv_shapes()]
    lins = [_take(lin, f"lin{l}.model.1.weight", (1, c, 1, 1), lin_path).reshape(c) for l, c in enumerate(VGG_WIDTHS)]
    return {"conv": conv, "lin": lins}


def pack_conv_weight(w: torch.Tensor, cols: int = 0) -> torch.Tensor:
    """fp32 [Cout, Cin, 3, 3] -> bf16 [Cout, 9 * cols], (ky, kx, ci) order, every tap's columns = [w_hi(Cin) | w_hi(Cin) | w_lo(Cin) | zeros]
    with w_hi = bf16(w), w_lo = bf16(w - w_hi): the weights of a pattern-1 operand [hi | lo | hi].  `cols` (default 3 Cin) pads a tap to a
    whole K slab (the first layer: 9 of ops.LPIPS_IN_COLS columns).  Load-time helper, any device."""
    cout, cin = w.shape[:2]
    cols = cols or 3 * cin
    assert w.shape[2:] == (3, 3) and cols >= 3 * cin
    t = w.to(torch.float32).permute(0, 2, 3, 1).reshape(cout, 9, cin)
    hi = t.to(torch.bfloat16)
    lo = (t - hi.to(torch.float32)).to(torch.bfloat16)
    out = torch.zeros((cout, 9, cols), dtype=torch.bfloat16, device=w.device)
    out[:, :, :cin], out[:, :, cin: 2 * cin], out[:, :, 2 * cin: 3 * cin] = hi, hi, lo
    return out.reshape(cout, 9 * cols)


class LpipsVGG:
    """``LpipsVGG(device, vgg16_path, lin_path)(gt[None], pred[None]) -> float``; weights are uploaded and packed once per object."""

    def __init__(self, device, vgg16_path, lin_path):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise Dm4dError(f"LpipsVGG: expected a HIP device, got {self.device} (diffuman4d_amd has no CPU path)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        w = load_lpips_weights(vgg16_path, lin_path)
        self.conv = []
        for n, (wt, b) in enumerate(w["conv"]):
            packed = pack_conv_weight(wt, ops.LPIPS_IN_COLS if n == 0 else 0).to(self.device)
            self.conv.append((packed, b.to(self.device)[None].expand(2, -1).contiguous()))  # the row bias of a batch of two
        self.lin = [l.to(self.device) for l in w["lin"]]

    def _check(self, gt, pred) -> Tuple[torch.Tensor, torch.Tensor]:
        for t, name in ((gt, "gt"), (pred, "pred")):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise Dm4dError(f"LpipsVGG: {name}: expected a tensor on a HIP device (no CPU fallback in diffuman4d_amd)")
        if gt.dim() != 4 or gt.shape[:2] != (1, 3) or gt.shape != pred.shape or gt.dtype != torch.float32 or pred.dtype != torch.float32:
            raise ValueError(f"LpipsVGG: expected two fp32 [1, 3, h, w] images of one shape, got {tuple(gt.shape)} and {tuple(pred.shape)}")
        if gt.device != self.device or pred.device != self.device:
            raise Dm4dError(f"LpipsVGG: the images are on {gt.device}, the weights on {self.device}")
        h, w = gt.shape[2:]
        if min(h, w) < MIN_EDGE:
            raise ValueError(f"The cropped region is too small for the five VGG stages of LPIPS: {h} x {w}.")
        if h * w > MAX_PIXELS:
            raise ValueError(f"The cropped region is too large for LPIPS: {h} x {w} = {h * w} pixels, at most {MAX_PIXELS} "
                             "(2^31 operand values in VGG's 64-channel stage).")
        return gt[0], pred[0]

    def _forward(self, gt, pred, keep: bool):
        """-> (out fp64 [5] on the device: the five tap distances, the five raw feature maps when `keep`)."""
        gt, pred = self._check(gt, pred)
        with torch.cuda.device(self.device):
            out = torch.empty(ops.LPIPS_TAPS, dtype=torch.float64, device=self.device)
            ws = ops.lpips_ws(gt.shape[1], gt.shape[2], self.device)  # the first tap is the largest
            taps, f, n = [], None, 0
            for s, stage in enumerate(VGG_STAGES):
                for j in range(len(stage)):
                    x = ops.lpips_input(gt, pred) if f is None else ops.lpips_relu_pool(f, pool=(j == 0))
                    wt, bias = self.conv[n]
                    f = ops.conv3x3(x, wt, rowbias=bias, out_f32=True)
                    n += 1
                ops.lpips_tap_distance(f, self.lin[s], s, out, ws)
                if keep:
                    taps.append(f)
        return out, taps

    def __call__(self, gt: torch.Tensor, pred: torch.Tensor) -> float:
        return self.distances(gt, pred)[ops.LPIPS_TAPS]

    def taps(self, gt: torch.Tensor, pred: torch.Tensor) -> List[torch.Tensor]:
        """The five raw feature maps, fp32 [2, H_l, W_l, C_l] (NHWC; 0 = gt, 1 = pred), as the convolutions leave them: BEFORE the ReLU,
        which the distance kernel applies when it reads them."""
        return self._forward(gt, pred, keep=True)[1]

    def distances(self, gt: torch.Tensor, pred: torch.Tensor) -> List[float]:
        """The five per-tap distances and their sum (the value), fp64."""
        d = self._forward(gt, pred, keep=False)[0].tolist()
        value = d[0]
        for x in d[1:]:  # in tap order, as _LPIPS.forward accumulates
            value = value + x
        return d + [value]
