"""Test-side model of the result evaluator (diffuman4d_amd/host/metrics.py, csrc/metrics.hip), used by tests/test_eval_cpu.py and
tests/test_eval_gpu.py.

This is a RESTATEMENT, written for these tests, of the steps the upstream evaluator performs (composite, torchvision's nearest resize,
mask_to_bbox(padding=8), crop, torchmetrics' PSNR and SSIM with their defaults); it is not upstream code, and neither torchmetrics nor
torchvision is needed to run it.  It is built from torch CPU operators -- F.interpolate(mode="nearest"), F.pad(mode="reflect"), a grouped
F.conv2d with the 11 x 11 Gaussian window, the 5-pixel border crop -- and runs in float32 (the upstream arithmetic) or in float64 (the
yardstick both the native kernel and the float32 form are measured against)."""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from diffuman4d_amd.host import metrics, ops


def nearest_index(out_size: int, in_size: int):
    """Plain-Python form of the index rule of F.interpolate(mode="nearest"): fp32 scale, floor, clamp."""
    scale = np.float32(in_size) / np.float32(out_size)
    return [min(int(math.floor(np.float32(d) * scale)), in_size - 1) for d in range(out_size)]


def to_tensor(a, dtype) -> torch.Tensor:
    """uint8 [h, w, 3] / [h, w] (a decoded file) or a float tensor / array [3, h, w] / [h, w] -> [C, h, w] of `dtype`."""
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a))
    if t.dtype == torch.uint8:
        t = t[..., None] if t.dim() == 2 else t
        return t.permute(2, 0, 1).contiguous().to(dtype).div(255)
    t = t[None] if t.dim() == 2 else t
    return t.to(dtype)


def apply_fmask(image, fmask, background_color):
    if background_color == "black":
        return image * fmask
    if background_color == "white":
        return image * fmask + (1.0 - fmask)
    if background_color == "grey":
        return image * fmask + (1.0 - fmask) * 0.5
    raise ValueError(f"Invalid background color: {background_color}")


def resize_nearest(t: torch.Tensor, canvas_size: int) -> torch.Tensor:
    h, w = t.shape[-2:]
    oh, ow = metrics.resized_size(h, w, canvas_size)
    return F.interpolate(t[None], size=(oh, ow), mode="nearest")[0]


def mask_to_bbox(fmask: torch.Tensor, padding: int = 8):
    fmask = fmask.squeeze(0)
    rows = torch.any(fmask != 0, dim=1).nonzero(as_tuple=True)[0]
    cols = torch.any(fmask != 0, dim=0).nonzero(as_tuple=True)[0]
    if rows.numel() == 0 or cols.numel() == 0:
        return None
    return (max(cols[0].item() - padding, 0), max(rows[0].item() - padding, 0),
            min(cols[-1].item() + 1 + padding, fmask.shape[1]), min(rows[-1].item() + 1 + padding, fmask.shape[0]))


def composites(pred, gt, pred_fmask=None, gt_fmask=None, canvas_size=1024, crop_with_fmask=True, background_color="black",
               dtype=torch.float64, check_area=True):
    """-> (pred, gt) cropped composites [3, h, w] of `dtype`, and the box (left, top, right, bottom) (the whole resized image when
    nothing is cropped)."""
    pred, gt = to_tensor(pred, dtype), to_tensor(gt, dtype)
    pm = None if pred_fmask is None else to_tensor(pred_fmask, dtype)
    gm = None if gt_fmask is None else to_tensor(gt_fmask, dtype)
    if gm is not None:
        gt = apply_fmask(gt, gm, background_color)
    if pm is not None:
        pred = apply_fmask(pred, pm, background_color)
    if canvas_size != gt.shape[-1]:
        gt, pred = resize_nearest(gt, canvas_size), resize_nearest(pred, canvas_size)
        gm = None if gm is None else resize_nearest(gm, canvas_size)
        pm = None if pm is None else resize_nearest(pm, canvas_size)
    box = (0, 0, gt.shape[-1], gt.shape[-2])
    if crop_with_fmask:
        obbs = [mask_to_bbox(m) for m in (gm, pm) if m is not None]
        if obbs:
            if any(o is None for o in obbs):
                return None, None, (0, 0, 0, 0)
            box = (min(o[0] for o in obbs), min(o[1] for o in obbs), max(o[2] for o in obbs), max(o[3] for o in obbs))
            if check_area and (box[2] - box[0]) * (box[3] - box[1]) < gt.numel() * 0.02:
                raise ValueError("The cropped region is too small. Please check your data.")
            l, t, r, b = box
            gt, pred = gt[..., t:b, l:r], pred[..., t:b, l:r]
    return pred.contiguous(), gt.contiguous(), box


def psnr(pred: torch.Tensor, gt: torch.Tensor) -> float:
    mse = ((pred - gt) ** 2).mean()
    return (10.0 * torch.log10(1.0 / mse)).item()


def gaussian_window(dtype) -> torch.Tensor:
    dist = torch.arange(-5, 6, dtype=dtype)
    g = torch.exp(-((dist / 1.5) ** 2) / 2)
    g = g / g.sum()
    return torch.outer(g, g)


def ssim(pred: torch.Tensor, gt: torch.Tensor) -> float:
    """[3, h, w] each; data_range 1, 11 x 11 Gaussian window, sigma 1.5, reflect padding, 5-pixel border dropped, mean."""
    dtype = pred.dtype
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    p, t = pred[None], gt[None]
    C = p.shape[1]
    kernel = gaussian_window(dtype).expand(C, 1, 11, 11).contiguous()
    x = torch.cat((p, t, p * p, t * t, p * t))
    x = F.pad(x, (5, 5, 5, 5), mode="reflect")
    o = F.conv2d(x, kernel, groups=C)
    mu_p, mu_t, e_pp, e_tt, e_pt = (o[i: i + 1] for i in range(5))
    mu_pp, mu_tt, mu_pt = mu_p * mu_p, mu_t * mu_t, mu_p * mu_t
    s_pp = torch.clamp(e_pp - mu_pp, min=0.0)
    s_tt = torch.clamp(e_tt - mu_tt, min=0.0)
    s_pt = e_pt - mu_pt
    m = ((2 * mu_pt + c1) * (2 * s_pt + c2)) / ((mu_pp + mu_tt + c1) * (s_pp + s_tt + c2))
    return m[..., 5:-5, 5:-5].mean().item()


def evaluate(pred, gt, pred_fmask=None, gt_fmask=None, canvas_size=1024, crop_with_fmask=True, background_color="black",
             dtype=torch.float64):
    """-> (psnr, ssim, box)."""
    p, g, box = composites(pred, gt, pred_fmask, gt_fmask, canvas_size, crop_with_fmask, background_color, dtype)
    return psnr(p, g), ssim(p, g), box


def standin_eval_psnr_ssim(blob, desc, desc_off=None, debug=False):
    """Drop-in for ops.eval_psnr_ssim on the host: reads the same staging buffer and descriptors, float32 model."""
    host = blob.numpy()
    n = desc.shape[0]
    if desc_off is not None:
        assert np.array_equal(host[desc_off: desc_off + n * ops.EVAL_FIELDS * 8].view(np.int64).reshape(n, -1), desc.numpy())
    out = torch.full((n, ops.EVAL_OUT), float("nan"), dtype=torch.float64)
    boxes = torch.zeros((n, 4), dtype=torch.int32)
    dbg = torch.zeros((n, 2, 3, int(desc[:, 6].max()), int(desc[:, 7].max()))) if debug else None
    for i, d in enumerate(desc.tolist()):
        op, og, opm, ogm, h, w, oh, ow, flags = d[:9]
        if32, mf32, crop = flags & ops.EVAL_IMAGE_F32, flags & ops.EVAL_MASK_F32, bool(flags & ops.EVAL_CROP_MASKS)
        bg = ["black", "white", "grey"][(flags >> ops.EVAL_BG_SHIFT) & 3]

        def image(o):
            if if32:
                return torch.from_numpy(host[o: o + h * w * 12].view(np.float32).reshape(3, h, w).copy())
            return host[o: o + h * w * 3].reshape(h, w, 3)

        def mask(o):
            if o < 0:
                return None
            if mf32:
                return torch.from_numpy(host[o: o + h * w * 4].view(np.float32).reshape(h, w).copy())
            return host[o: o + h * w].reshape(h, w)

        # the canvas that gives the descriptor's resized size (the model resizes by canvas, the kernel by size)
        canvas = w if (oh, ow) == (h, w) else min(oh, ow)
        assert metrics.resized_size(h, w, canvas) == (oh, ow)
        p, g, box = composites(image(op), image(og), mask(opm), mask(ogm), canvas, crop, bg, torch.float32, check_area=False)
        if not crop:
            l, t, r, b = d[9:13]
            box = (l, t, r, b)
            p, g = p[..., t:b, l:r], g[..., t:b, l:r]
        boxes[i] = torch.tensor(box, dtype=torch.int32)
        if p is None or p.shape[-1] < 11 or p.shape[-2] < 11:
            continue
        out[i] = torch.tensor([psnr(p, g), ssim(p, g), p.min().item(), p.max().item(), g.min().item(), g.max().item(),
                               ((p.double() - g.double()) ** 2).sum().item(), float("nan")], dtype=torch.float64)
        if debug:
            dbg[i, 0, :, : p.shape[-2], : p.shape[-1]] = p
            dbg[i, 1, :, : g.shape[-2], : g.shape[-1]] = g
    return (out, boxes, dbg) if debug else (out, boxes)
