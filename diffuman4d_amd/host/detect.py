"""Person boxes around a caller-named detector: the detector step of the reference's ``predict_keypoints``
(scripts/preprocess/sapiens/lite/demo/vis_pose.py:425-440 -> detector_utils.py process_one_image_bbox -> pose_utils.py nms), which runs
a person detector on every image and hands every kept box to the pose network.

The network is not part of this package and is never downloaded: the caller names a TorchScript file (``load_person_detector``) or hands
over any callable.  Everything around it runs on the device (csrc/detect.hip):

  * ``detector_inputs``: the images (and masks) staged once by ``pose.stage_batch`` -- the very planes ``pose_inputs`` reads -- are
    composited over black, resized keeping their ratio into the top-left corner of the network's canvas, padded and normalised in one
    launch.  The resize is an integer rule of this package ("Person boxes"), modelled on mmcv's ``imrescale`` and OpenCV's
    8-bit bilinear ``resize``; everything of it that a float touches is in the tables ``detector_tables`` makes in fp64;
  * ``select_boxes``: one launch takes the dense output ``boxes [n, A, 4]`` / ``scores [n, A, C]``, which never visits the host, to the
    kept boxes: threshold, rescale to image pixels, exact top ``max_per_img``, greedy NMS as ``pose_utils.py::nms`` computes it in fp32.

There is no CPU path: a ``device`` that is not a HIP device is an error.
"""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import lib as _l
from . import ops
from . import pose as _pose
from . import staging as _st

# UNVERIFIED defaults: mmdet's RTMDet base config as remembered (the reference's detector config only says
# ``_base_ = 'mmdet::rtmdet/...'``, which is not in its tree): BGR-ordered statistics, pad value 114.
MEAN = (103.53, 116.28, 123.675)
STD = (57.375, 57.12, 58.395)
PAD_VALUE = 114
SHAPE = (640, 640)
COEF_ONE = _l.DETECT_COEF_ONE


def rescaled_size(h: int, w: int, shape: Tuple[int, int]) -> Tuple[int, int]:
    """mmcv's ``rescale_size((w, h), scale=(Wnet, Hnet))`` -> (nw, nh), in fp64: the factor is ``min(long / max(h, w),
    short / min(h, w))`` with long / short the canvas' longer / shorter side, the sizes ``int(side * factor + 0.5)``."""
    H, W = shape
    sf = min(max(H, W) / max(h, w), min(H, W) / min(h, w))
    return int(w * sf + 0.5), int(h * sf + 0.5)


def _canvas(shape) -> Tuple[int, int]:
    H, W = int(shape[0]), int(shape[1])
    if not (1 <= H <= _l.DETECT_MAX_CANVAS and 1 <= W <= _l.DETECT_MAX_CANVAS):
        raise ValueError(f"shape: canvas {W} x {H} is outside 1..{_l.DETECT_MAX_CANVAS}")
    return H, W


def axis_table(src: int, dst: int) -> Tuple[np.ndarray, np.ndarray]:
    """One axis of the resize `src` -> `dst` pixels -> (first tap [dst] int32, weights [dst] int32 = c0 | c1 << 16 with c0 on the first
    tap and c1 on the next): ``f = fp32((d + 0.5) * (src / dst) - 0.5)``, ``s = floor(f)``, ``a = f - s``; s < 0 -> s = 0, a = 0;
    s >= src - 1 -> s = src - 1, a = 0; c1 = rint(2048 a), c0 = rint(2048 (1 - a)), saturated to int16.  fp64 apart from the one
    rounding to fp32."""
    scale = src / dst
    f = ((np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32).astype(np.float64)
    s = np.floor(f)
    a = f - s
    low, high = s < 0, s >= src - 1
    s = np.where(low, 0, np.where(high, src - 1, s))
    a = np.where(low | high, 0.0, a)
    c1 = np.clip(np.rint(a * COEF_ONE), -32768, 32767).astype(np.int64)
    c0 = np.clip(np.rint((1.0 - a) * COEF_ONE), -32768, 32767).astype(np.int64)
    packed = ((c0 & 0xffff) | ((c1 & 0xffff) << 16)).astype(np.uint32).view(np.int32)
    return s.astype(np.int32), packed


def detector_tables(sizes: Sequence[Tuple[int, int]], shape: Tuple[int, int] = SHAPE) -> Tuple[List[np.ndarray], np.ndarray, np.ndarray]:
    """Per image of `sizes` = [(h, w)] and the canvas `shape` = (H, W) -> (its int32 table {nw, nh | xofs[nw] | yofs[nh] | alpha[nw] |
    beta[nh]} of include/dm4d.h, [n, 2] int32 = (nw, nh), [n, 2] float32 = (inv_w, inv_h) = fp32(1 / (nw / w)), fp32(1 / (nh / h)): what
    takes a box of the canvas back to image pixels, as mmdet's ``scale_factor`` does).  Numpy, fp64, no device.  ValueError when a
    resized side is 0 or does not fit the canvas (mmcv's rule looks at the longer and the shorter side, not at width and height: a
    landscape image does not fit a portrait canvas)."""
    H, W = _canvas(shape)
    tabs, nwnh, inv = [], [], []
    for k, (h, w) in enumerate(sizes):
        nw, nh = rescaled_size(h, w, (H, W))
        if nw < 1 or nh < 1 or nw > W or nh > H:
            raise ValueError(f"sizes[{k}]: {w} x {h} resizes to {nw} x {nh}, which is empty or does not fit the {W} x {H} canvas")
        xofs, alpha = axis_table(w, nw)
        yofs, beta = axis_table(h, nh)
        tabs.append(np.concatenate([np.array([nw, nh], dtype=np.int32), xofs, yofs, alpha, beta]))
        nwnh.append((nw, nh))
        inv.append((np.float32(1.0 / (nw / w)), np.float32(1.0 / (nh / h))))
    return tabs, np.array(nwnh, dtype=np.int32).reshape(-1, 2), np.array(inv, dtype=np.float32).reshape(-1, 2)


def _norm(mean, std, pad_value, channel_order: str) -> Tuple[torch.Tensor, int, bool]:
    mean, std = [float(v) for v in mean], [float(v) for v in std]
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("mean and std: three values each")
    if channel_order not in ("rgb", "bgr"):
        raise ValueError(f'channel_order must be "rgb" or "bgr", got {channel_order!r}')
    if int(pad_value) != pad_value or not 0 <= int(pad_value) <= 255:
        raise ValueError(f"pad_value must be a byte, got {pad_value!r}")
    return torch.tensor(mean + std, dtype=torch.float32), int(pad_value), channel_order == "bgr"


def detector_inputs_staged(staged: "_pose.Staged", shape: Tuple[int, int] = SHAPE, *, mean=MEAN, std=STD, pad_value: int = PAD_VALUE,
                           channel_order: str = "rgb") -> Tuple[torch.Tensor, dict]:
    """``detector_inputs`` for a batch that is already on the device (``pose.stage_batch``): nothing is decoded or uploaded again but
    the tables and descriptors."""
    H, W = _canvas(shape)
    norm, pad, bgr = _norm(mean, std, pad_value, channel_order)
    tabs, nwnh, inv = detector_tables(staged.sizes, (H, W))
    offs = np.concatenate([[0], np.cumsum([t.size for t in tabs])])
    n = len(tabs)
    with torch.cuda.device(staged.device):
        desc = _pose.descriptors([(k, int(offs[k])) for k in range(n)], staged.sizes, staged.image_off, staged.mask_off)
        meta, meta_host, tab_off, tab_len, desc_off = _st.pack_meta(np.concatenate(tabs), desc, staged.device)
        out = ops.detect_input(staged.blob, meta, meta_host, n, desc_off, tab_off, tab_len, H, W, norm, pad, bgr)
        inv_dev = torch.from_numpy(inv).to(staged.device)
        torch.cuda.current_stream().synchronize()  # meta_host may go; the tensor is complete when it is handed over
    return out, {"sizes": list(staged.sizes), "shape": (H, W), "resized": nwnh, "inv_scale": inv, "inv_scale_dev": inv_dev}


def detector_inputs(images, fmasks=None, shape: Tuple[int, int] = SHAPE, device="cuda", *, mean=MEAN, std=STD, pad_value: int = PAD_VALUE,
                    channel_order: str = "rgb", pool: Optional[ThreadPoolExecutor] = None, device_decode: bool = False) -> Tuple[torch.Tensor, dict]:
    """The detector's input for a batch of images -> (tensor fp32 [n, 3, H, W] on `device`, meta for ``select_boxes``).

    images / fmasks / device_decode: as for ``pose.pose_inputs``; an image is composited over black through its mask.  Each is resized
    keeping its ratio into the top-left corner of the `shape` = (H, W) canvas; the rest is `pad_value`; plane c is
    ``(v[c] - mean[c]) / std[c]`` in fp32.  channel_order "rgb": plane c is the image's RGB channel c -- with the defaults' BGR-ordered
    statistics this is what the reference feeds its detector (its dataset returns BGR, vis_pose.py:430 swaps that to RGB, and the
    pipeline normalises with ``bgr_to_rgb=False``); "bgr": plane c is channel 2 - c.  The defaults (mean, std, pad_value, 640 x 640) are
    mmdet's RTMDet base config as remembered and are NOT verified against it: it is not in the reference's tree.

    meta: ``sizes`` [(h, w)], ``shape``, ``resized`` int32 [n, 2] = (nw, nh), ``inv_scale`` float32 [n, 2] and its device copy."""
    _norm(mean, std, pad_value, channel_order), _canvas(shape)  # refused before anything is decoded
    staged = _pose.stage_batch(images, fmasks, device, pool, device_decode, "detector_inputs", lambda sizes: detector_tables(sizes, shape))
    return detector_inputs_staged(staged, shape, mean=mean, std=std, pad_value=pad_value, channel_order=channel_order)


def select_boxes(boxes: torch.Tensor, scores: torch.Tensor, meta: dict, *, det_cat_id: int = 0, bbox_thr: float = 0.3, nms_thr: float = 0.3,
                 max_per_img: int = 100) -> Tuple[List[np.ndarray], List[np.ndarray]]:
    """Dense detector output -> per image the kept boxes [k_i, 4] float32 (x1, y1, x2, y2 in image pixels, best first) and their
    scores [k_i] float32.  boxes [n, A, 4] in canvas pixels and scores [n, A, C] (probabilities), fp32 on the device: the form of an
    RTMDet export without NMS.  meta: from ``detector_inputs``.  One launch (dm4d_detect_select_f32; include/dm4d.h has the definition):
    ``scores[:, det_cat_id] > bbox_thr`` (fp32, strict), boxes times ``inv_scale``, boxes that are not finite or empty dropped, the best
    `max_per_img` by score (ties by anchor index), greedy NMS with ``ovr <= nms_thr``."""
    for name, t in (("boxes", boxes), ("scores", scores)):
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise _l.Dm4dError(f"{name}: expected a tensor on a HIP device (no CPU fallback in diffuman4d_amd)")
    n = len(meta["sizes"])
    if boxes.dim() != 3 or boxes.shape[0] != n or boxes.shape[2] != 4:
        raise ValueError(f"boxes: expected [{n}, A, 4], got {tuple(boxes.shape)}")
    if scores.dim() != 3 or scores.shape[:2] != boxes.shape[:2]:
        raise ValueError(f"scores: expected [{n}, {boxes.shape[1]}, C], got {tuple(scores.shape)}")
    with torch.cuda.device(boxes.device):
        inv = meta["inv_scale_dev"].to(boxes.device)
        counts, out, _ = ops.detect_select(boxes.float().contiguous(), scores.float().contiguous(), inv, det_cat_id, bbox_thr, nms_thr, max_per_img)
        counts, out = counts.cpu().numpy(), out.cpu().numpy()
    return [out[k, :counts[k, 0], :4].copy() for k in range(n)], [out[k, :counts[k, 0], 4].copy() for k in range(n)]


def load_person_detector(path: str, device) -> Callable:
    """The caller's person detector: ``torch.jit.load`` of a local TorchScript file.  Nothing is ever downloaded.

    The callable takes fp32 ``[n, 3, H, W]`` on the device (``detector_inputs``) and must return ``(boxes, scores)`` on the device:
    boxes ``[n, A, 4]`` = x1, y1, x2, y2 in pixels of the network input, scores ``[n, A, C]`` = per-class probabilities (after the
    sigmoid), for all A anchors, without score filtering and without NMS -- an RTMDet head's decoded output.  A module of another form
    needs a wrapper of the caller's.  This path has not been run with a real export: none is at hand, and the tests go through a
    stand-in callable."""
    if not os.path.isfile(path):
        raise FileNotFoundError(f"person detector {path!r} does not exist (it is never downloaded: name a local file)")
    return torch.jit.load(path, map_location=device).eval()
