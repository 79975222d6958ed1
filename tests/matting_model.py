"""Test-side definition of the foreground-mask stage (diffuman4d_amd/host/matting.py, csrc/matting.hip): the reference's
scripts/preprocess/remove_background.py step by step with Pillow's own ``resize`` / ``rotate`` and torch CPU arithmetic, and a
table-driven twin of both resizes (numpy passes over the host's coefficient tables, as tests/capture_model.py) that checks those tables.
numpy + Pillow + torch CPU only; used by tests/test_matting_cpu.py and tests/test_matting_gpu.py."""
from __future__ import annotations

import numpy as np
import torch
from PIL import Image

from capture_model import _pass

MEAN = [0.485, 0.456, 0.406]  # remove_background.py:20
STD = [0.229, 0.224, 0.225]


def rotated(image: Image.Image, rotate_clockwise: int) -> Image.Image:
    """remove_background.py:76-77."""
    return image.rotate(-rotate_clockwise, expand=True) if rotate_clockwise != 0 else image


def normalise(resized_u8: np.ndarray, dtype=torch.float16) -> torch.Tensor:
    """ToTensor (u8 -> fp32, .div(255)), Normalize (.sub(mean).div(std) with fp32 tensors, as torchvision forms them), then .half():
    uint8 [S_h, S_w, 3] -> [3, S_h, S_w]."""
    x = torch.from_numpy(np.array(resized_u8)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    mean = torch.as_tensor(MEAN, dtype=torch.float32).view(-1, 1, 1)
    std = torch.as_tensor(STD, dtype=torch.float32).view(-1, 1, 1)
    x = x.sub(mean).div(std)
    return x.half() if dtype == torch.float16 else x


def matting_input(image_u8: np.ndarray, size=(1024, 1024), rotate_clockwise: int = 0, dtype=torch.float16) -> torch.Tensor:
    """Steps 1-3 of the reference for one uint8 [h, w, 3] image -> [3, S_h, S_w] of `dtype`: rotate, Pillow's antialiased bilinear
    resize to (S_h, S_w) ignoring the aspect ratio (transforms.Resize on a PIL image), ToTensor, Normalize, .half()."""
    image = rotated(Image.fromarray(image_u8), rotate_clockwise)
    resized = image.resize((size[1], size[0]), Image.BILINEAR)
    return normalise(np.asarray(resized), dtype)


def quantise(logits_fp16: torch.Tensor) -> torch.Tensor:
    """fp16 logits -> uint8, by definition: s = fp16(1 / (1 + exp(-x))) evaluated in fp64 and rounded once; m = fp16(fp32(s) * 255);
    byte = trunc(m); NaN -> 0."""
    assert logits_fp16.dtype == torch.float16
    x = logits_fp16.double()
    s64 = x.neg().exp().add(1.0).reciprocal()
    # rounded ONCE: numpy converts fp64 to fp16 directly, torch goes through fp32, and sigmoid(0.0068359375) lies 7e-9 below a tie of
    # fp16 that the detour through fp32 lands on exactly
    s = torch.from_numpy(s64.numpy().astype(np.float16))
    m = s.float().mul(255.0).half()
    return torch.where(torch.isnan(x), torch.zeros_like(m), m).float().to(torch.uint8)


def matting_mask(logits: torch.Tensor, size, rotate_clockwise: int = 0) -> np.ndarray:
    """Steps 4-7 for one plane of fp16 logits [.., S_h, S_w] and the stored image's (h, w) -> uint8 [h, w]: quantise, Pillow's default
    resize (bicubic) to the rotated image's size, rotate back."""
    h, w = size
    plane = quantise(logits.reshape(logits.shape[-2:])).numpy()
    rh, rw = (w, h) if rotate_clockwise in (90, 270) else (h, w)
    fmask = Image.fromarray(plane).resize((rw, rh)).convert("L")
    if rotate_clockwise != 0:
        fmask = fmask.rotate(rotate_clockwise, expand=True)
    out = np.asarray(fmask)
    assert out.shape == (h, w)
    return out


# -- the table-driven twin -----------------------------------------------------------------------------------------------------------
def table_resize(a: np.ndarray, out_hw, table) -> np.ndarray:
    """Pillow's two passes over an [h, w] or [h, w, c] uint8 array with the coefficient tables of `table(in_size, out_size)`: the
    horizontal pass rounded to uint8, then the vertical one; an axis that keeps its size is not filtered."""
    squeeze = a.ndim == 2
    c = a[..., None] if squeeze else a
    H, W = out_hw
    if c.shape[1] != W:
        c = _pass(c, *table(c.shape[1], W), axis=1)
    if c.shape[0] != H:
        c = _pass(c, *table(c.shape[0], H), axis=0)
    return c[..., 0] if squeeze else c
