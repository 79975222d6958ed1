"""Test-side model of LPIPS-VGG (diffuman4d_amd/host/lpips.py, csrc/lpips.hip), used by tests/test_lpips_cpu.py and
tests/test_lpips_gpu.py.

A RESTATEMENT, written for these tests, of what torchmetrics' ``LearnedPerceptualImagePatchSimilarity(net_type="vgg", normalize=True)``
computes; it is not upstream code, and neither torchmetrics nor torchvision is needed to run it.  It is built from torch CPU operators
(F.conv2d, F.max_pool2d) and runs in float64 (the yardstick) or float32 (the upstream arithmetic).

Weights are GENERATED here (seeded, full VGG-16 width) and written in the two checkpoint layouts users of the reference have; nothing is
committed or fetched.  Convolution weights N(0, 2 / (9 Cin)) keep the activations' scale through the thirteen layers; biases U(-0.1, 0.1);
linear weights U(0, 1) * 200 / C put the values of the test pairs between 0.01 and 1.7."""
from __future__ import annotations

from pathlib import Path
from typing import Dict, List, Tuple

import torch
import torch.nn.functional as F

# recorded from torchmetrics' _LPIPS (functional/image/lpips.py): ScalingLayer's buffers ...
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
# ... _normalize_tensor's epsilon, INSIDE the square root ...
NORM_EPS = 1e-8
# ... and torchvision's vgg16().features convolution indices, grouped by the tap behind them (relu1_2 .. relu5_3)
STAGES = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))
WIDTHS = (64, 128, 256, 512, 512)


def random_weights(seed: int = 0) -> Dict[str, torch.Tensor]:
    """One state dict with the keys of BOTH files (features.N.weight / .bias, classifier.0.weight as ballast, linL.model.1.weight)."""
    g = torch.Generator().manual_seed(seed)
    sd, cin = {}, 3
    for stage, width in zip(STAGES, WIDTHS):
        for idx in stage:
            sd[f"features.{idx}.weight"] = torch.randn(width, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
            sd[f"features.{idx}.bias"] = torch.rand(width, generator=g) * 0.2 - 0.1
            cin = width
    sd["classifier.0.weight"] = torch.randn(4, 8, generator=g)  # the loader must ignore it (the real one is 4096 x 25088)
    for l, width in enumerate(WIDTHS):
        sd[f"lin{l}.model.1.weight"] = torch.rand(1, width, 1, 1, generator=g) * (200.0 / width)
    return sd


def write_checkpoints(root: Path, sd: Dict[str, torch.Tensor], fmt: str = "pth") -> Tuple[str, str]:
    """-> (vgg16_path, lin_path) under `root`, `fmt` = "pth" (torch.save of a state dict) or "safetensors"."""
    root.mkdir(parents=True, exist_ok=True)
    vgg = {k: v.contiguous() for k, v in sd.items() if k.startswith(("features.", "classifier."))}
    lin = {k: v.contiguous() for k, v in sd.items() if k.startswith("lin")}
    if fmt == "safetensors":
        from safetensors.torch import save_file
        paths = root / "vgg16.safetensors", root / "lpips_vgg.safetensors"
        save_file(vgg, str(paths[0])), save_file(lin, str(paths[1]))
    else:
        paths = root / "vgg16-397923af.pth", root / "vgg.pth"
        torch.save(vgg, paths[0]), torch.save(lin, paths[1])
    return str(paths[0]), str(paths[1])


def lpips(gt: torch.Tensor, pred: torch.Tensor, sd: Dict[str, torch.Tensor], dtype=torch.float64) -> Tuple[float, List[torch.Tensor]]:
    """gt, pred [3, h, w] in [0, 1] -> (value, the five taps [2, C, H, W] after ReLU; 0 = gt, 1 = pred) in `dtype` on the CPU."""
    x = torch.stack((gt, pred)).to(dtype)
    x = 2 * x - 1
    x = (x - torch.tensor(SHIFT, dtype=dtype)[None, :, None, None]) / torch.tensor(SCALE, dtype=dtype)[None, :, None, None]
    taps, value = [], 0.0
    for s, stage in enumerate(STAGES):
        if s:
            x = F.max_pool2d(x, 2, 2)
        for idx in stage:
            x = F.relu(F.conv2d(x, sd[f"features.{idx}.weight"].to(dtype), sd[f"features.{idx}.bias"].to(dtype), padding=1))
        taps.append(x)
        n = x / torch.sqrt(NORM_EPS + (x * x).sum(1, keepdim=True))
        w = sd[f"lin{s}.model.1.weight"].to(dtype)
        value = value + (w * (n[0:1] - n[1:2]) ** 2).sum(1).mean().item()
    return value, taps


def pair(h: int, w: int, amp: float, seed: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """a = U(0, 1), b = clamp(a + amp N(0, 1)), fp32 [3, h, w]."""
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(3, h, w, generator=g)
    b = (a + amp * torch.randn(3, h, w, generator=g)).clamp(0, 1)
    return a, b


if __name__ == "__main__":  # python tests/lpips_model.py DIR [pth|safetensors]: the two seeded checkpoint files (tools/eval_bench.py --lpips)
    import sys
    print(*write_checkpoints(Path(sys.argv[1]), random_weights(0), sys.argv[2] if len(sys.argv) > 2 else "pth"))
