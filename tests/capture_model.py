"""Test-side model of dm4d_capture_crop_resize_f32 (numpy passes over the host coefficient tables + the reference's fp32 epilogue
in torch), used by tests/test_capture_cpu.py and tests/test_capture_gpu.py."""
from __future__ import annotations

import numpy as np
import torch

from diffuman4d_amd.host import capture

ONE = 1 << (capture.PRECISION_BITS - 1)


def clip8(v: np.ndarray) -> np.ndarray:
    return np.where(v >= 1 << 30, 255, np.where(v <= 0, 0, v >> capture.PRECISION_BITS)).astype(np.uint8)


def _pass(a: np.ndarray, bounds: np.ndarray, k: np.ndarray, axis: int) -> np.ndarray:
    """One Pillow pass along `axis` (0 = rows, 1 = columns) of an [h, w, c] uint8 array."""
    idx = bounds[:, :1] + np.arange(k.shape[1])[None, :]
    wt = np.where(np.arange(k.shape[1])[None, :] < bounds[:, 1:], k, 0).astype(np.int64)
    idx = np.minimum(idx, a.shape[axis] - 1)
    g = np.take(a.astype(np.int64), idx, axis=axis)  # axis 1: [h, out, ks, c]; axis 0: [out, ks, w, c]
    if axis == 1:
        s = (g * wt[None, :, :, None]).sum(axis=2)
    else:
        s = (g * wt[:, :, None, None]).sum(axis=1)
    return clip8(ONE + s)


def crop(a: np.ndarray, top: int, left: int, ch: int, cw: int) -> np.ndarray:
    """PIL crop with zero fill outside the image; [h, w, c] -> [ch, cw, c]."""
    out = np.zeros((ch, cw, a.shape[2]), dtype=np.uint8)
    y0, x0 = max(top, 0), max(left, 0)
    y1, x1 = min(top + ch, a.shape[0]), min(left + cw, a.shape[1])
    if y1 > y0 and x1 > x0:
        out[y0 - top: y1 - top, x0 - left: x1 - left] = a[y0:y1, x0:x1]
    return out


def crop_resize(a: np.ndarray, top: int, left: int, ch: int, cw: int, H: int, W: int) -> np.ndarray:
    """Image.crop((left, top, left + cw, top + ch)).resize((W, H), BICUBIC) on an [h, w] or [h, w, c] uint8 array, with Pillow's
    pass skipping (an axis that keeps its size is not filtered)."""
    squeeze = a.ndim == 2
    c = crop(a[..., None] if squeeze else a, top, left, ch, cw)
    if cw != W:
        c = _pass(c, *capture.bicubic_table(cw, W), axis=1)
    if ch != H:
        c = _pass(c, *capture.bicubic_table(ch, H), axis=0)
    return c[..., 0] if squeeze else c


def unit(u: torch.Tensor) -> torch.Tensor:
    """TF.to_tensor + norm_vae_tensor: [.., C] uint8 -> float32 in [-1, 1]."""
    return u.to(torch.float32).div(255) * 2.0 - 1.0


def epilogue(img: np.ndarray, mask: np.ndarray, skel: np.ndarray):
    """The reference's float epilogue on resized uint8 planes -> (pixel_values [3, H, W], skeleton [3, H, W]) fp32."""
    i = unit(torch.from_numpy(np.array(img)).permute(2, 0, 1).contiguous())
    m = unit(torch.from_numpy(np.array(mask))[None].contiguous())
    s = unit(torch.from_numpy(np.array(skel)).permute(2, 0, 1).contiguous())
    i, m = i * 0.5 + 0.5, m * 0.5 + 0.5  # apply_fmask(..., "white", vae_normalized=True)
    p = i * m + (1.0 - m) * 1.0
    return p * 2.0 - 1.0, s


def standin_crop_resize(blob, blob_host, n_frames, desc_off, tab_off, tab_len, H, W):
    """Drop-in for ops.capture_crop_resize on the host: reads the same staging buffer (planes, tables, descriptors)."""
    host = blob_host.numpy()
    desc = host[desc_off: desc_off + n_frames * capture.FIELDS * 8].view(np.int64).reshape(n_frames, capture.FIELDS)
    pix, skel = torch.empty(n_frames, 3, H, W), torch.empty(n_frames, 3, H, W)
    for f, d in enumerate(desc):
        oi, om, os_, sh, sw, top, left, ch, cw = (int(v) for v in d[:9])
        plane = lambda o, c: host[o: o + sh * sw * c].reshape(sh, sw, c)
        img, m, s = plane(oi, 3), plane(om, 1), plane(os_, 3)
        args = (top, left, ch, cw, H, W)
        pix[f], skel[f] = epilogue(crop_resize(img, *args), crop_resize(m, *args)[..., 0], crop_resize(s, *args))
    return pix, skel
