"""2-D keypoint prediction around a caller-named pose network: the ``predict_keypoints`` action of the reference's preprocess.sh
(scripts/preprocess/predict_keypoints.py -> sapiens/lite/demo/vis_pose.py, pose_utils.py), which writes
``poses_sapiens/{camera}/{frame}.json``, the files ``host/triang.py`` reads.

The network is not part of this package and is never downloaded: the caller names a checkpoint file (``load_pose_model``) or hands over
any callable (``pose_model``).  Everything around it runs on the device (csrc/pose.hip):

  * ``pose_inputs``: images (and foreground masks) are decoded with Pillow in a thread pool into pinned staging and uploaded once
    (host/staging.py lays the planes out, fills them and packs {tables | descriptors}; ``plane_layout`` and ``descriptors`` say where);
    one launch composites each image over black through its mask, warps every person box to the network's input and normalises it.
    The warp is an integer rule of this package ("Keypoint prediction"), modelled on OpenCV's bilinear warpAffine.  With
    ``device_decode=True`` the JPEG / PNG files among them are decoded on the device into the same planes (``_device_files``);
  * ``decode_heatmaps``: one launch takes the heatmaps, which never visit the host, to refined keypoints (UDP / DARK decoding); the
    last two linear maps to image pixels are done on the host in fp64, as the reference's numpy does.

A batch is staged once (``stage_batch``) for every reader of its planes: ``pose_inputs_staged`` here and, on the detector route of
``predict_keypoints``, ``detect.detector_inputs_staged`` (host/detect.py: the person boxes of a detector the caller names).

There is no CPU path: a ``device`` that is not a HIP device is an error.
"""
from __future__ import annotations

import json
import os
from concurrent.futures import ThreadPoolExecutor
from glob import glob
from typing import Callable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import lib as _l
from . import ops
from . import staging as _st
from .codec import decode_staged, probe_file
from .staging import MAX_HOST_THREADS  # noqa: F401  (importable from here as before)

MEAN = (123.5, 116.5, 103.5)   # vis_pose.py:451-452, RGB order (preprocess_pose's two BGR swaps cancel)
STD = (58.5, 57.0, 57.5)
PADDING = 1.25                 # top_down_affine_transform's default
FIELDS = _l.POSE_FIELDS


# -- boxes -> centre, scale, warp tables (host, numpy) -------------------------------------------------------------------------------
def box_center_scale(bbox, shape: Tuple[int, int], padding: float = PADDING) -> Tuple[np.ndarray, np.ndarray]:
    """[x1, y1, x2, y2] -> (center (2,), scale (2,)) float64 as top_down_affine_transform forms them (pose_utils.py:248-269): the box
    grown by `padding`, then widened or heightened to the aspect of the network input `shape` = (H, W)."""
    box = np.asarray(bbox, dtype=np.float64).reshape(4)
    if not np.all(np.isfinite(box)) or box[2] <= box[0] or box[3] <= box[1]:
        raise ValueError(f"bbox must be finite with x2 > x1 and y2 > y1, got {box.tolist()}")
    H, W = shape
    center = np.array([box[0] + box[2], box[1] + box[3]]) * 0.5
    bw, bh = (box[2] - box[0]) * padding, (box[3] - box[1]) * padding
    aspect = W / H
    scale = np.array([bw, bw / aspect]) if bw > bh * aspect else np.array([bh * aspect, bh])
    return center, scale


def udp_warp_matrix(center: np.ndarray, scale: np.ndarray, shape: Tuple[int, int]) -> np.ndarray:
    """The reference's UDP warp matrix without rotation (its get_udp_warp_matrix(center, scale, 0, (W, H))): 2 x 3 float32, image ->
    network input.  The box corner ``center - scale / 2`` goes to (0, 0) and ``center + scale / 2`` to (W - 1, H - 1): a diagonal of
    ``(last pixel) / scale`` and a translation of ``diagonal * (scale / 2 - center)``, formed in fp64 and rounded to float32 when stored."""
    H, W = shape
    gain = np.array([W - 1, H - 1], dtype=np.float64) / scale
    mat = np.zeros((2, 3), dtype=np.float32)
    mat[[0, 1], [0, 1]] = gain
    mat[:, 2] = gain * (scale * 0.5 - center)
    return mat


def warp_tables(mat: np.ndarray, shape: Tuple[int, int]) -> np.ndarray:
    """The int32 table {adelta[W] | bdelta[W] | X0[H] | Y0[H]} of include/dm4d.h (dm4d_pose_input_u8_f32) from the fp64 inverse of the
    float32 matrix: everything of the warp that a float touches.  Raises ValueError for a box so small or so far away that an entry
    leaves +-2^29."""
    H, W = shape
    m = mat.astype(np.float64)
    det = m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]
    d = 1.0 / det if det != 0 else 0.0
    a00, a01, a10, a11 = m[1, 1] * d, m[0, 1] * -d, m[1, 0] * -d, m[0, 0] * d
    a02 = -a00 * m[0, 2] - a01 * m[1, 2]
    a12 = -a10 * m[0, 2] - a11 * m[1, 2]
    xs, ys = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    with np.errstate(all="ignore"):
        tab = np.concatenate([np.rint(a00 * xs * 1024), np.rint(a10 * xs * 1024), np.rint((a01 * ys + a02) * 1024) + 16,
                              np.rint((a11 * ys + a12) * 1024) + 16])
    if not np.all(np.abs(tab) <= _l.POSE_TAB_LIMIT):  # NaN included
        raise ValueError("bbox: the warp leaves the fixed-point range (a degenerate or far-away box)")
    return tab.astype(np.int32)


# -- staging ---------------------------------------------------------------------------------------------------------------------------
def _open_all(images, fmasks, pool: Optional[ThreadPoolExecutor]):
    """Open (not yet decode) the images and masks and check them -> (PIL images or None, PIL masks with None for an image without one,
    sizes [(h, w)]).  `images` None: masks alone (``fmask_boxes``).  Needs no device."""
    n = len(fmasks) if images is None else len(images)
    if n < 1:
        raise ValueError("images: at least one image")
    if images is not None and fmasks is not None and len(fmasks) != n:
        raise ValueError("fmask_paths and image_paths must have the same length")
    ims = _st.pool_map(pool, _st.open_image, images) if images is not None else None
    mks = _st.pool_map(pool, lambda m: None if m is None else _st.open_image(m), fmasks) if fmasks is not None else [None] * n
    sizes = _st.check_sizes([im.size[::-1] for im in (ims if ims is not None else mks)], _l.POSE_MAX_SIDE, "images")
    for k, m in enumerate(mks):
        if m is not None:
            if m.mode not in ("L", "1"):
                raise ValueError(f"fmasks[{k}]: mode {m.mode!r}, expected 'L' or '1'")
            if m.size != sizes[k][::-1]:
                raise ValueError("images do not match")  # Pillow's text for Image.composite
    return ims, mks, sizes


def plane_layout(sizes: Sequence[Tuple[int, int]], with_images: bool, has_mask: Sequence[bool]) -> Tuple[List[int], List[int], int]:
    """Where the planes of a batch of `sizes` = [(h, w)] lie in its blob: each image (3 bytes per pixel), then its mask (1), every
    plane 16-byte aligned -> (image offsets, mask offsets, bytes of the blob); -1: an absent plane."""
    lay = _st.Layout()
    image_off, mask_off = [], []
    for (h, w), masked in zip(sizes, has_mask):
        image_off.append(lay.add(h * w * 3) if with_images else -1)
        mask_off.append(lay.add(h * w) if masked else -1)
    return image_off, mask_off, lay.total


def descriptors(rows: Sequence[Tuple[int, int]], sizes, image_off, mask_off) -> np.ndarray:
    """rows: (image index, table offset in int32 elements) -> int64 [len(rows), FIELDS] = {image offset, mask offset, h, w, table
    offset, 0, 0, 0} (include/dm4d.h)."""
    desc = np.zeros((len(rows), FIELDS), dtype=np.int64)
    for r, (k, toff) in enumerate(rows):
        desc[r, :5] = [image_off[k], mask_off[k], sizes[k][0], sizes[k][1], toff]
    return desc


def _device_files(ims, mks, sizes, pool: Optional[ThreadPoolExecutor]) -> dict:
    """{("image" | "mask", index): the codec.StagedFile} of the images and masks that were opened from files csrc/jpegdec.hip or
    csrc/pngdec.hip decodes into the plane the kernels read: an RGB image (or a grayscale JPEG, which the decoder replicates as
    convert("RGB") does) and a mode-L mask.  Masks of mode ``1``, WebP files and whatever else the probes refuse are not in it."""
    from . import jpegdec, pngdec

    def probe(job):
        kind, k, im = job
        name = getattr(im, "filename", "") if im is not None else ""
        if not name or im.format not in ("JPEG", "PNG"):
            return None
        f = probe_file(name, (jpegdec, pngdec))
        if f is None or (f.h, f.w) != tuple(sizes[k]) or f.mode != im.mode:
            return None
        ok = f.mode == "L" if kind == "mask" else (f.mode == "RGB" or (f.mode == "L" and f.codec is jpegdec))
        return f if ok else None
    jobs = [("image", k, im) for k, im in enumerate(ims or [])] + [("mask", k, m) for k, m in enumerate(mks)]
    return {job[:2]: f for job, f in zip(jobs, _st.pool_map(pool, probe, jobs)) if f is not None}


def _stage(ims, mks, sizes, device: torch.device, pool: Optional[ThreadPoolExecutor], device_decode: bool = False):
    """Decode one batch into pinned staging and queue its upload -> (blob uint8 on the device, the pinned buffer, image offsets, mask
    offsets).  The pinned buffer has to stay alive until the consumer has synchronised.  device_decode: the files of ``_device_files``
    are not decoded by Pillow: their bytes go up and the device decodes them into their planes of the blob (a file its decoder
    refuses keeps the Pillow route)."""
    image_off, mask_off, total = plane_layout(sizes, ims is not None, [m is not None for m in mks])
    on_device = _device_files(ims, mks, sizes, pool) if device_decode else {}
    jobs = [(o, (ims[k], "RGB")) for k, o in enumerate(image_off) if o >= 0 and ("image", k) not in on_device] + \
           [(o, (mks[k], "L")) for k, o in enumerate(mask_off) if o >= 0 and ("mask", k) not in on_device]
    host = _st.pinned(total, device)
    _st.fill(host.numpy(), jobs, pool)
    blob = host.to(device, non_blocking=True) if jobs else torch.empty(total, dtype=torch.uint8, device=device)
    if on_device:
        entries = [((image_off if kind == "image" else mask_off)[k], f, 3 if kind == "image" else 1) for (kind, k), f in on_device.items()]
        mode = {id(f): "RGB" if ch == 3 else "L" for _, f, ch in entries}
        decode_staged(entries, blob, lambda f: np.asarray(_st.open_image(f.path).convert(mode[id(f)])))
    return blob, host, image_off, mask_off


class Staged(NamedTuple):
    """One batch on the device: what ``pose_inputs`` and ``detect.detector_inputs`` both read.  `host`, the pinned source of the upload,
    has to stay alive until a consumer has synchronised."""
    blob: torch.Tensor
    host: torch.Tensor
    image_off: List[int]
    mask_off: List[int]
    sizes: List[Tuple[int, int]]
    device: torch.device


def stage_batch(images, fmasks, device, pool: Optional[ThreadPoolExecutor] = None, device_decode: bool = False, what: str = "stage_batch",
                check: Optional[Callable] = None) -> Staged:
    """Open, decode and upload a batch once (``_open_all`` + ``_stage``) for every consumer of its planes.  check(sizes): a consumer's
    refusal of the sizes [(h, w)], called once the files are open and before the device is touched."""
    ims, mks, sizes = _open_all(list(images), None if fmasks is None else list(fmasks), pool)
    if check is not None:
        check(sizes)
    dev = _l.hip_device(device, what)
    with torch.cuda.device(dev):
        return Staged(*_stage(ims, mks, sizes, dev, pool, device_decode), sizes, dev)


def _mask_boxes(blob: torch.Tensor, sizes, image_off, mask_off) -> np.ndarray:
    n = len(sizes)
    meta, meta_host, _, _, desc_off = _st.pack_meta(None, descriptors([(k, 0) for k in range(n)], sizes, image_off, mask_off), blob.device)
    return ops.pose_mask_box(blob, meta, meta_host, n, desc_off).cpu().numpy()  # .cpu() synchronises: meta_host may go


def fmask_boxes(fmasks, device="cuda", *, device_decode: bool = False) -> np.ndarray:
    """[n, 4] int32: per mask (path, PIL image or uint8 array; mode ``L`` or ``1``) the box [x1, y1, x2, y2] of its pixels >= 128, x2 and
    y2 exclusive; the whole image for a mask without one.  One launch (dm4d_pose_mask_box_u8).  device_decode: as for ``pose_inputs``."""
    _, mks, sizes = _open_all(None, list(fmasks), None)
    dev = _l.hip_device(device, "fmask_boxes")
    with torch.cuda.device(dev):
        blob, _host, image_off, mask_off = _stage(None, mks, sizes, dev, None, device_decode)
        return _mask_boxes(blob, sizes, image_off, mask_off)


def _boxes_of(b, h: int, w: int) -> List:
    """An image's entry of `bboxes` -> its list of boxes: None (the whole image), one [x1, y1, x2, y2], or several, each of which may
    again be None."""
    whole = [0, 0, w, h]
    if b is None:
        return [whole]
    if isinstance(b, (list, tuple)) and any(x is None or np.ndim(x) > 0 for x in b):
        return [whole if x is None else np.asarray(x, dtype=np.float64).reshape(4) for x in b]
    return list(np.asarray(b, dtype=np.float64).reshape(-1, 4))


def pose_inputs(images, fmasks=None, bboxes=None, shape: Tuple[int, int] = (1024, 768), device="cuda", *, bbox_source: str = "image",
                pool: Optional[ThreadPoolExecutor] = None, device_decode: bool = False) -> Tuple[torch.Tensor, np.ndarray, np.ndarray]:
    """The pose network's input for a batch of images -> (tensor fp32 [rows, 3, H, W] on `device`, centers [rows, 2], scales [rows, 2]
    float64; rows in image order, an image's boxes in their order).

    images: paths, PIL images or uint8 [h, w, 3] arrays, of any sizes.  fmasks: one per image, mode ``L`` or ``1`` (ValueError
    otherwise), of the image's size, or None for an image without one; the image is composited over black through it, as
    ``Image.composite(image, black, fmask)``.  bboxes: per image ``[x1, y1, x2, y2]`` or several of them, float, or None for the whole
    image; bboxes=None: whole images, or, with ``bbox_source="fmask"``, the box of each mask's pixels >= 128.  shape: the network's
    input (H, W).

    device_decode: images that are baseline JPEG files of the supported set (host/jpegdec.py::probe) or 8-bit RGB PNG files
    (host/pngdec.py::probe), and mode-L masks that are such PNG (or JPEG) files, are not decoded by Pillow: their file bytes go up and the
    device decodes them into the planes the kernels read, byte for byte Pillow's pixels, so the result is the same.  Masks of mode
    ``1``, WebP images and every other input keep the Pillow route."""
    if bbox_source not in ("image", "fmask"):
        raise ValueError(f'bbox_source must be "image" or "fmask", got {bbox_source!r}')
    H, W = int(shape[0]), int(shape[1])
    ims, mks, sizes = _open_all(list(images), None if fmasks is None else list(fmasks), pool)
    n = len(ims)
    if bboxes is not None and len(bboxes) != n:
        raise ValueError(f"bboxes: expected one entry per image ({n}), got {len(bboxes)}")
    if bboxes is None and bbox_source == "fmask" and any(m is None for m in mks):
        raise ValueError('bbox_source="fmask" needs a mask for every image')
    dev = _l.hip_device(device, "pose_inputs")
    with torch.cuda.device(dev):
        return pose_inputs_staged(Staged(*_stage(ims, mks, sizes, dev, pool, device_decode), sizes, dev), bboxes, (H, W), bbox_source)


def pose_inputs_staged(staged: Staged, bboxes, shape: Tuple[int, int], bbox_source: str = "image") -> Tuple[torch.Tensor, np.ndarray, np.ndarray]:
    """``pose_inputs`` for a batch that is already on the device (``stage_batch``): the same result, nothing decoded or uploaded again.
    `bboxes` has been checked against the batch by the caller."""
    H, W = int(shape[0]), int(shape[1])
    blob, _host, image_off, mask_off, sizes, dev = staged
    n = len(sizes)
    with torch.cuda.device(dev):
        if bboxes is None:
            boxes = _mask_boxes(blob, sizes, image_off, mask_off)[:, None, :] if bbox_source == "fmask" else [[[0, 0, w, h]] for h, w in sizes]
        else:
            boxes = [_boxes_of(b, *sizes[k]) for k, b in enumerate(bboxes)]
        rows, tabs, centers, scales = [], [], [], []
        per_row = 2 * (W + H)
        for k in range(n):
            for box in boxes[k]:
                c, s = box_center_scale(box, (H, W))
                tabs.append(warp_tables(udp_warp_matrix(c, s, (H, W)), (H, W)))
                rows.append((k, (len(tabs) - 1) * per_row))
                centers.append(c), scales.append(s)
        if not rows:
            raise ValueError("bboxes: no box at all")
        tab = np.concatenate(tabs)
        meta, meta_host, tab_off, tab_len, desc_off = _st.pack_meta(tab, descriptors(rows, sizes, image_off, mask_off), dev)
        out = ops.pose_input(blob, meta, meta_host, len(rows), desc_off, tab_off, tab_len, H, W, torch.tensor(MEAN + STD, dtype=torch.float32))
        torch.cuda.current_stream().synchronize()  # the pinned buffers may go; the tensor is complete when it is handed over
    return out, np.stack(centers), np.stack(scales)


def decode_heatmaps(heatmaps: torch.Tensor, input_size: Tuple[int, int], centers, scales) -> Tuple[np.ndarray, np.ndarray]:
    """heatmaps [n, K, Hh, Wh] on the device, input_size = (W, H) of the network input, centers / scales [n, 2] from ``pose_inputs`` ->
    (keypoints [n, K, 2] float64 in image pixels, scores [n, K] float32).  One launch (dm4d_pose_udp_decode_f32), then
    ``kp / [Wh - 1, Hh - 1] * input_size`` and ``(kp / input_size) * scale + center - 0.5 * scale`` in fp64 (pose_utils.py:177-178,
    vis_pose.py:107).  A map whose maximum is <= 0 is not refined: its heatmap location is (-1, -1)."""
    if not isinstance(heatmaps, torch.Tensor) or heatmaps.device.type != "cuda":
        raise _l.Dm4dError("heatmaps: expected a tensor on a HIP device (no CPU fallback in diffuman4d_amd)")
    if heatmaps.dim() != 4:
        raise ValueError(f"heatmaps: expected [n, K, Hh, Wh], got {tuple(heatmaps.shape)}")
    n, K, Hh, Wh = heatmaps.shape
    centers, scales = np.asarray(centers, dtype=np.float64).reshape(-1, 2), np.asarray(scales, dtype=np.float64).reshape(-1, 2)
    if len(centers) != n or len(scales) != n:
        raise ValueError(f"centers / scales: expected {n} rows, got {len(centers)} and {len(scales)}")
    with torch.cuda.device(heatmaps.device):
        locs, scores = ops.pose_udp_decode(heatmaps.float().contiguous())
        locs, scores = locs.cpu().numpy(), scores.cpu().numpy()
    size = np.asarray(input_size, dtype=np.int64)
    kp = locs / np.array([Wh - 1, Hh - 1]) * size
    kp = (kp / size) * scales[:, None, :] + centers[:, None, :] - 0.5 * scales[:, None, :]
    return kp, scores


# -- the stage -------------------------------------------------------------------------------------------------------------------------
def load_pose_model(path: str, device) -> Callable:
    """The caller's pose checkpoint, by the reference's rule (vis_pose.py:188-212): ``torch.jit.load`` when the file name contains
    ``_torchscript``, else ``torch.export.load(path).module()``.  Nothing is ever downloaded.

    The module is used as loaded and must accept fp32 ``[n, 3, H, W]``: ``predict_keypoints`` feeds fp32 and converts the heatmaps to
    fp32.  The reference instead converts an exported module to bfloat16 and feeds bfloat16 under autocast; a checkpoint exported for
    bfloat16 input needs a wrapper of the caller's (``pose_model=lambda x: module(x.bfloat16())``).  This path has not been run with a
    real Sapiens checkpoint: none is at hand, and the tests go through ``pose_model``."""
    if not os.path.isfile(path):
        raise FileNotFoundError(f"pose checkpoint {path!r} does not exist (it is never downloaded: name a local file)")
    if "_torchscript" in os.path.basename(path):
        return torch.jit.load(path, map_location=device).eval()
    return torch.export.load(path).module().to(device)


def list_inputs(images_dir: str, fmasks_dir: Optional[str]) -> Tuple[List[str], Optional[List[str]]]:
    """``**/*.jpg`` + ``**/*.webp`` under images_dir and ``**/*.png`` under fmasks_dir, each sorted; paired by index (vis_pose.py:367-376)."""
    images = sorted(glob(f"{images_dir}/**/*.jpg", recursive=True) + glob(f"{images_dir}/**/*.webp", recursive=True))
    fmasks = None
    if fmasks_dir is not None and fmasks_dir != "None":
        fmasks = sorted(glob(f"{fmasks_dir}/**/*.png", recursive=True))
        if len(fmasks) != len(images):
            raise ValueError("fmask_paths and image_paths must have the same length")
    return images, fmasks


def output_path(out_kp2d_dir: str, image_path: str) -> str:
    """out_kp2d_dir/<last two components of image_path>.json (vis_pose.py:410-412)."""
    tail = os.path.join(*os.path.normpath(image_path).split(os.sep)[-2:])
    return os.path.join(out_kp2d_dir, os.path.splitext(tail)[0] + ".json")


def _parses(path: str) -> bool:
    try:
        with open(path, "r") as f:
            json.load(f)
        return True
    except Exception:
        return False


def write_instances(path: str, keypoints: np.ndarray, scores: np.ndarray) -> None:
    """``{"instance_info": [{"keypoints", "keypoint_scores"}, ...]}``, one entry per box, indented with one tab (vis_pose.py:111-126)."""
    info = [{"keypoints": np.asarray(kp).tolist(), "keypoint_scores": np.asarray(sc).tolist()} for kp, sc in zip(keypoints, scores)]

    def write(tmp: str) -> None:
        with open(tmp, "w") as f:
            json.dump({"instance_info": info}, f, indent="\t")
    _st.atomic_write(path, write)


def predict_keypoints(images_dir: str, out_kp2d_dir: str, fmasks_dir: Optional[str] = None, sapiens_ckpt_path: Optional[str] = None,
                      detector_ckpt_path: Optional[str] = None, gpu_ids: Optional[Sequence[int]] = None, num_workers: int = 4, *,
                      pose_model: Optional[Callable] = None, shape: Tuple[int, int] = (1024, 768), heatmap_scale: int = 4,
                      batch_size: int = 4, skip_exists: bool = True, bbox_source: str = "image", device_decode: bool = False,
                      person_detector=None, det_shape: Tuple[int, int] = (640, 640), det_cat_id: int = 0, bbox_thr: float = 0.3,
                      nms_thr: float = 0.3) -> dict:
    """Predict the 2-D keypoints of every image under `images_dir` and write ``out_kp2d_dir/{camera}/{frame}.json``.

    pose_model: any callable taking fp32 [n, 3, H, W] on the device and returning [n, K, H / heatmap_scale, W / heatmap_scale] on the
    device; by default ``load_pose_model(sapiens_ckpt_path)``, once per GPU (which must then accept fp32 input; see there).  It is the
    caller's network: its output never visits the host.

    The person boxes (bbox_source): "image", the whole image; "fmask", the box of the foreground mask; "detector", the reference's
    route: `person_detector` -- a callable (``detect.load_person_detector`` says what it takes and returns) or the path of a local
    TorchScript file, loaded once per GPU -- runs on every image, and every kept box (``detect.select_boxes`` with `det_cat_id`,
    `bbox_thr`, `nms_thr`; `det_shape` is the detector's input) becomes a row of the pose network and an entry of the image's
    ``instance_info``, best first; an image without a kept box gets the whole image (vis_pose.py:438-440).  A batch is staged once: the
    detector's input and the pose network's are two readers of the same planes.  "detector" without `person_detector` is refused, and
    so is a ``detector_ckpt_path``: the reference's own detector checkpoint needs mmdet, which this package does not carry.  The
    reference's ``flip`` is not taken (it averages the flipped pass without flipping it back).  One worker thread per GPU id; decoding and the
    JSON files go through a pool of `num_workers` threads.  Returns counts.  device_decode: handed to ``pose_inputs`` (the same files are
    written)."""
    if detector_ckpt_path:
        raise NotImplementedError("detector_ckpt_path: the person detector is mmdet's RTMDet, which diffuman4d_amd does not carry; "
                                  'the box is the whole image, or bbox_source="fmask", or hand over a network of your own: '
                                  'person_detector with bbox_source="detector"')
    if bbox_source not in ("image", "fmask") and not (bbox_source == "detector" and person_detector is not None):
        raise ValueError(f'bbox_source must be "image" or "fmask", or "detector" together with person_detector, got {bbox_source!r}')
    if bbox_source == "fmask" and (fmasks_dir is None or fmasks_dir == "None"):
        raise ValueError('bbox_source="fmask" needs fmasks_dir')
    if pose_model is None and not sapiens_ckpt_path:
        raise ValueError("name the pose network: sapiens_ckpt_path (a local checkpoint file) or pose_model (a callable)")
    H, W = int(shape[0]), int(shape[1])
    if batch_size < 1 or heatmap_scale < 1:
        raise ValueError("batch_size and heatmap_scale must be at least 1")
    images, fmasks = list_inputs(images_dir, fmasks_dir)
    outs = [output_path(out_kp2d_dir, p) for p in images]
    todo = [k for k in range(len(images)) if not (skip_exists and os.path.exists(outs[k]) and _parses(outs[k]))]
    result = {"images": len(images), "written": 0, "skipped": len(images) - len(todo)}
    if not todo:
        return result
    batches = [todo[i: i + batch_size] for i in range(0, len(todo), batch_size)]
    hm_size = (int(W / heatmap_scale), int(H / heatmap_scale))

    def check_heat(heat, rows: int) -> None:
        if not isinstance(heat, torch.Tensor) or heat.device.type != "cuda" or heat.dim() != 4 or heat.shape[0] != rows:
            raise _l.Dm4dError("pose_model: expected a [n, K, Hh, Wh] tensor on the device")
        if (heat.shape[3], heat.shape[2]) != hm_size:
            raise _l.Dm4dError(f"pose_model: heatmaps of {heat.shape[3]} x {heat.shape[2]}, expected {hm_size[0]} x {hm_size[1]} "
                               f"(input {W} x {H}, heatmap_scale {heatmap_scale})")

    def process_batch(model: Callable, batch: List[int], dev: torch.device, pool: ThreadPoolExecutor) -> List:
        x, centers, scales = pose_inputs([images[k] for k in batch], None if fmasks is None else [fmasks[k] for k in batch], None,
                                         (H, W), dev, bbox_source=bbox_source, pool=pool, **({"device_decode": True} if device_decode else {}))
        heat = model(x)
        check_heat(heat, x.shape[0])
        kp, sc = decode_heatmaps(heat, (W, H), centers, scales)
        return [pool.submit(write_instances, outs[k], kp[r: r + 1], sc[r: r + 1]) for r, k in enumerate(batch)]  # one box per image here

    def process_batch_detector(models, batch: List[int], dev: torch.device, pool: ThreadPoolExecutor) -> List:
        from . import detect  # here, not at the top: detect imports this module
        model, detector = models
        staged = stage_batch([images[k] for k in batch], None if fmasks is None else [fmasks[k] for k in batch], dev, pool, device_decode,
                             "predict_keypoints", lambda sizes: detect.detector_tables(sizes, det_shape))
        xd, meta = detect.detector_inputs_staged(staged, det_shape)
        found = detector(xd)
        if not isinstance(found, (tuple, list)) or len(found) != 2:
            raise _l.Dm4dError("person_detector: expected (boxes [n, A, 4], scores [n, A, C]) on the device")
        kept, _ = detect.select_boxes(found[0], found[1], meta, det_cat_id=det_cat_id, bbox_thr=bbox_thr, nms_thr=nms_thr)
        boxes = [list(b) if len(b) else None for b in kept]  # None: the whole image
        x, centers, scales = pose_inputs_staged(staged, boxes, (H, W))
        heats = []
        for r in range(0, x.shape[0], batch_size):
            heats.append(model(x[r: r + batch_size]))
            check_heat(heats[-1], min(batch_size, x.shape[0] - r))
        kp, sc = decode_heatmaps(torch.cat(heats), (W, H), centers, scales)
        first = np.concatenate([[0], np.cumsum([max(len(b), 1) for b in kept])])
        return [pool.submit(write_instances, outs[k], kp[first[i]: first[i + 1]], sc[first[i]: first[i + 1]]) for i, k in enumerate(batch)]

    load_model = lambda dev: pose_model if pose_model is not None else load_pose_model(sapiens_ckpt_path, dev)
    if bbox_source == "detector":
        from . import detect
        load_detector = lambda dev: detect.load_person_detector(person_detector, dev) if isinstance(person_detector, (str, os.PathLike)) else person_detector
        load_model, process_batch = (lambda dev, pose_net=load_model: (pose_net(dev), load_detector(dev))), process_batch_detector
    result["written"] = _st.run_stage("predict_keypoints", gpu_ids, num_workers, "dm4d-pose", batches, load_model, process_batch)
    return result
