"""Result evaluation: PSNR and SSIM of predicted against captured views, the reference's ``ImageEvaluator`` / ``evaluate_results``
(``src/data/utils/metric_utils.py``) built from their behaviour.

What the reference does per pair -- decode, composite over the background through the foreground masks, torchvision's nearest resize
to the canvas, the padded bounding box of the masks, the crop, torchmetrics' PSNR and SSIM -- is split here:

  * host, in a thread pool (Pillow releases the GIL while it decodes): decode, the shape and argument checks with the reference's
    ``ValueError`` texts, the resized size, and -- after the device has answered -- the crop-area and value-range checks;
  * device (``dm4d_eval_psnr_ssim_f64``, csrc/metrics.hip): everything else, for a whole batch of pairs at once.  The reference cannot
    batch "because the croppings are different"; per-pair descriptors remove that limit.

Every batch's planes and descriptors go into one pinned staging buffer (host/staging.py) and up in one copy; uint8 planes stay uint8 on the way
(4 x fewer bytes than ``to_tensor``'s floats).  There is no CPU path: a host tensor is uploaded, a missing library raises.

LPIPS-VGG is built (``host/lpips.py::LpipsVGG``, csrc/lpips.hip: VGG-16 on the MFMA convolution with three-term bf16 products, fp64
distances), but its weights are not part of this package and are never fetched: ``lpips_weights=(vgg16_path, lin_path)`` on
``evaluate_keys`` / ``evaluate_results`` (torchvision's VGG-16 checkpoint and the LPIPS linear layers, the two files the reference's
torchmetrics module loads) builds one ``LpipsVGG`` per worker.  ``ImageEvaluator(device, lpips=callable)`` takes that object or any
other callable: it receives the cropped composites ``(gt[None], pred[None])`` on the device, as torchmetrics' module does.  Without
either ``lpips`` is ``None`` in every result and ``null`` in metrics.json.
"""
from __future__ import annotations

import json
import logging
import os
import threading
from concurrent.futures import ThreadPoolExecutor
from typing import Callable, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from PIL import Image

from . import lpips as _lpips
from . import ops
from .codec import decode_or_fallback, read_file
from .lib import Dm4dError
from .staging import Layout, fill, pinned, write_meta

log = logging.getLogger(__name__)

BACKGROUNDS = {"black": 0, "white": 1, "grey": 2}
MIN_EDGE = 11  # the 11 x 11 SSIM window has to fit into the crop

ImageLike = Union[torch.Tensor, str, np.ndarray]


def resized_size(h: int, w: int, canvas_size: int) -> Tuple[int, int]:
    """(h, w) after the reference's resize step: torchvision's rule (the short edge becomes `canvas_size`, the long edge
    int(canvas_size * long / short)), applied only when canvas_size != w -- the reference compares against the LAST dimension only."""
    if canvas_size == w:
        return h, w
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = canvas_size, int(canvas_size * long / short)
    return (new_long, new_short) if w <= h else (new_short, new_long)


class _DeviceFile:
    """A file the device will decode into its region of the staging blob (`codec`: host/jpegdec.py or host/pngdec.py): an RGB image
    [h, w, 3] or a mode-L mask [h, w].  It stands where the decoded uint8 array would, with its shape, dtype and size, and holds the
    file's bytes and plan instead of pixels."""
    dtype = np.dtype(np.uint8)

    def __init__(self, path, codec, plan, data: bytes):
        self.path, self.codec, self.plan, self.data = path, codec, plan, data
        bpp = plan.bytes_per_pixel
        self.shape = (plan.h, plan.w) if bpp == 1 else (plan.h, plan.w, bpp)
        self.nbytes = plan.h * plan.w * bpp

    def pixels(self) -> np.ndarray:
        """The Pillow route of the same file."""
        with Image.open(self.path) as im:
            return np.asarray(im)


def _load(x: ImageLike, channels: int, device_decode: bool = False):
    """A path -> uint8 [h, w, 3] / [h, w] (what TF.to_tensor would divide by 255); a tensor -> fp32 [3, h, w] / [h, w] on the host.
    A uint8 numpy array is taken as an already decoded file (np.asarray(Image.open(path))).  device_decode: the path of a baseline
    JPEG file the device decodes (host/jpegdec.py::probe; images only) or of an 8-bit PNG file it decodes (host/pngdec.py::probe; images
    and masks) is not decoded here -> a _DeviceFile; the mode check is made on its header."""
    if isinstance(x, np.ndarray):
        if x.dtype != np.uint8 or x.ndim != (3 if channels == 3 else 2) or (channels == 3 and x.shape[2] != 3):
            raise ValueError(f"expected a decoded uint8 [h, w{', 3' if channels == 3 else ''}] array, got {x.dtype} {x.shape}")
        return np.ascontiguousarray(x)
    if isinstance(x, (str, os.PathLike)):
        if device_decode:
            from . import jpegdec, pngdec
            want = "RGB" if channels == 3 else "L"
            data = read_file(x)
            for codec in (jpegdec, pngdec) if channels == 3 else (pngdec,):
                plan = codec.probe(data)
                if plan is not None:
                    if plan.mode != want:
                        raise ValueError(f"{x}: image mode {plan.mode!r}, expected {want!r} (no conversion is made: it would change values)")
                    return _DeviceFile(x, codec, plan, data)
        with Image.open(x) as im:
            want = "RGB" if channels == 3 else "L"
            if im.mode != want:
                raise ValueError(f"{x}: image mode {im.mode!r}, expected {want!r} (no conversion is made: it would change values)")
            return np.asarray(im)
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"expected a path or a tensor, got {type(x).__name__}")
    t = x.detach().to("cpu", torch.float32)
    if channels == 1 and t.dim() == 3 and t.shape[0] == 1:
        t = t[0]
    if t.dim() != (3 if channels == 3 else 2) or (channels == 3 and t.shape[0] != 3):
        raise ValueError(f"expected a [{'3, ' if channels == 3 else '1, '}h, w] tensor, got {tuple(x.shape)}")
    return t.contiguous().numpy()


def _chw_shape(a: np.ndarray, channels: int) -> Tuple[int, ...]:
    """The shape the reference's tensor would have (its messages print it)."""
    if a.dtype == np.uint8:
        return (channels,) + a.shape[:2]
    return a.shape if channels == 3 else (1,) + a.shape


def _as_f32(a: np.ndarray, channels: int) -> np.ndarray:
    """TF.to_tensor of a uint8 plane (a true fp32 division), CHW."""
    if a.dtype != np.uint8:
        return a
    f = a.astype(np.float32) / np.float32(255.0)
    return np.ascontiguousarray(f.transpose(2, 0, 1)) if channels == 3 else f


class ImageEvaluator:
    """The reference's ``ImageEvaluator``: ``evaluator(pred, gt, pred_fmask, gt_fmask, canvas_size, crop_with_fmask,
    background_color) -> (psnr, ssim, lpips)``; ``evaluate_batch`` takes many such argument sets and spends one upload and one
    library call on them.  Results are Python floats (fp64 of the device's fp64 means)."""

    def __init__(self, device, lpips: Optional[Callable] = None, decode_threads: int = 8, device_decode: bool = False):
        """device_decode: predictions and ground truths that are baseline JPEG files of the supported set, and images and masks that
        are 8-bit PNG files of theirs, are decoded on the device, into their regions of the staging blob (host/jpegdec.py,
        host/pngdec.py), instead of by Pillow in the decode threads: the same bytes."""
        self.device = torch.device(device)
        self.device_decode = bool(device_decode)
        if self.device_decode and self.device.type != "cuda":
            raise Dm4dError(f"device_decode: device {device!r} is not a HIP device (no CPU fallback in diffuman4d_amd)")
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.lpips = lpips
        self._pool = ThreadPoolExecutor(max_workers=max(1, int(decode_threads)), thread_name_prefix="dm4d-eval-decode")
        self._tls = threading.local()

    # -- host half of one pair ----------------------------------------------------------------------------------------------------
    @staticmethod
    def _prepare(pred: ImageLike, gt: ImageLike, pred_fmask: Optional[ImageLike] = None, gt_fmask: Optional[ImageLike] = None,
                 canvas_size: int = 1024, crop_with_fmask: bool = True, background_color: str = "black", device_decode: bool = False) -> Dict:
        same_mask = pred_fmask is not None and pred_fmask is gt_fmask or (isinstance(pred_fmask, str) and pred_fmask == gt_fmask)
        p, g = _load(pred, 3, device_decode), _load(gt, 3, device_decode)
        pm = None if pred_fmask is None else _load(pred_fmask, 1, device_decode)
        gm = pm if same_mask else (None if gt_fmask is None else _load(gt_fmask, 1, device_decode))
        ps, gs = _chw_shape(p, 3), _chw_shape(g, 3)
        # the reference's sanity checks, in its order and with its texts (metric_utils.py:86-96)
        if gs != ps:
            raise ValueError("The GT and predicted images should have the same shape.")
        if pm is not None and ps[-2:] != _chw_shape(pm, 1)[-2:]:
            raise ValueError(f"shape mismatch: {torch.Size(ps)} != {torch.Size(_chw_shape(pm, 1))}")
        if gm is not None and gs[-2:] != _chw_shape(gm, 1)[-2:]:
            raise ValueError(f"shape mismatch: {torch.Size(gs)} != {torch.Size(_chw_shape(gm, 1))}")
        if background_color not in BACKGROUNDS:
            raise ValueError(f"Invalid background color: {background_color}")
        if crop_with_fmask and (pm is None and gm is None):
            raise ValueError("Either pred_fmask or gt_fmask should be provided to crop with fmask.")
        if p.dtype != g.dtype:  # one decoded file, one tensor: both travel as fp32
            p, g = (a.pixels() if isinstance(a, _DeviceFile) else a for a in (p, g))
            p, g = _as_f32(p, 3), _as_f32(g, 3)
        if pm is not None and gm is not None and pm.dtype != gm.dtype:
            pm, gm = (a.pixels() if isinstance(a, _DeviceFile) else a for a in (pm, gm))
            pm, gm = _as_f32(pm, 1), _as_f32(gm, 1)
        h, w = ps[-2:]
        oh, ow = resized_size(h, w, int(canvas_size))
        if min(h, w, oh, ow) < MIN_EDGE:
            raise ValueError(f"The image is too small for the 11 x 11 SSIM window: {h} x {w} -> {oh} x {ow}.")
        return {"pred": p, "gt": g, "pmask": pm, "gmask": gm, "h": h, "w": w, "oh": oh, "ow": ow, "bg": BACKGROUNDS[background_color],
                "crop": bool(crop_with_fmask) and (pm is not None or gm is not None)}

    def _stream(self):
        st = getattr(self._tls, "stream", None)
        if st is None:
            st = self._tls.stream = torch.cuda.Stream(device=self.device)
        return st

    # -- device half of a batch ---------------------------------------------------------------------------------------------------
    def _run(self, items: List[Dict], debug: bool):
        """Pack planes and descriptors into one staging buffer, upload it, launch -> (out [n, 8] fp64, boxes [n, 4], debug) on the host
        (debug stays on the device)."""
        lay, jobs, files = Layout(), [], []
        desc = np.zeros((len(items), ops.EVAL_FIELDS), dtype=np.int64)
        for i, it in enumerate(items):
            offs = {}
            for name in ("pred", "gt", "pmask", "gmask"):
                a = it[name]
                if a is None:
                    offs[name] = -1
                elif name == "gmask" and a is it["pmask"]:
                    offs[name] = offs["pmask"]  # evaluate_results passes ONE mask file for both: it is decoded and uploaded once
                else:
                    offs[name] = lay.add(a.nbytes)
                    (files if isinstance(a, _DeviceFile) else jobs).append((offs[name], a))
            mask = it["pmask"] if it["pmask"] is not None else it["gmask"]
            flags = ((ops.EVAL_IMAGE_F32 if it["pred"].dtype != np.uint8 else 0)
                     | (ops.EVAL_MASK_F32 if mask is not None and mask.dtype != np.uint8 else 0)
                     | (ops.EVAL_CROP_MASKS if it["crop"] else 0) | (it["bg"] << ops.EVAL_BG_SHIFT))
            desc[i, :13] = [offs["pred"], offs["gt"], offs["pmask"], offs["gmask"], it["h"], it["w"], it["oh"], it["ow"], flags,
                            0, 0, it["ow"], it["oh"]]
        desc_off = lay.add(desc.nbytes)
        blob = pinned(lay.total, self.device)
        fill(blob.numpy(), jobs, self._pool)
        write_meta(blob.numpy(), None, 0, desc, desc_off)
        desc_t = torch.from_numpy(desc)
        if self.device.type != "cuda":  # no device: the ops call decides (it refuses host tensors -- there is no CPU fallback)
            res = ops.eval_psnr_ssim(blob, desc_t, desc_off, debug=debug)
            return res[0], res[1], (res[2] if debug else None)
        st = self._stream()
        with torch.cuda.device(self.device), torch.cuda.stream(st):
            dev_blob = blob.to(self.device, non_blocking=True)
            if files:  # their regions of the blob went up unfilled: the device decodes into them
                from . import jpegdec, pngdec
                for codec in (pngdec, jpegdec):  # one call per codec; a file the decoder refuses: Pillow's pixels (or Pillow's exception)
                    part = [(off, a) for off, a in files if a.codec is codec]
                    if part:
                        decode_or_fallback(codec, [(a.plan, a.data, off, a.plan.bytes_per_pixel) for off, a in part], dev_blob,
                                           lambda k: part[k][1].pixels())
            res = ops.eval_psnr_ssim(dev_blob, desc_t, desc_off, debug=debug)
            out, boxes = res[0].cpu(), res[1].cpu()
        st.synchronize()
        return out, boxes, (res[2] if debug else None)

    def evaluate_batch(self, pairs: Sequence[Dict]) -> List[Tuple[float, float, Optional[float]]]:
        """`pairs`: keyword sets of ``__call__``.  -> [(psnr, ssim, lpips)] in the same order; the first failing pair raises."""
        if not pairs:
            return []
        items = list(self._pool.map(lambda kw: self._prepare(**kw, device_decode=self.device_decode), pairs))
        out, boxes, dbg = self._run(items, debug=self.lpips is not None)
        out, boxes = out.numpy(), boxes.numpy()
        res = []
        for i, it in enumerate(items):
            l, t, r, b = (int(v) for v in boxes[i])
            if it["crop"] and (r - l) * (b - t) < 3 * it["oh"] * it["ow"] * 0.02:  # gt.numel() counts the 3 channels
                raise ValueError("The cropped region is too small. Please check your data.")
            if r - l < MIN_EDGE or b - t < MIN_EDGE:
                raise ValueError(f"The cropped region is too small for the 11 x 11 SSIM window: {b - t} x {r - l}.")
            psnr, ssim, pmin, pmax, gmin, gmax = (float(v) for v in out[i, :6])
            if 0.0 - 1e-6 > gmin or gmax > 1.0 + 1e-6:
                raise ValueError("The GT image should be normalized.")
            if 0.0 - 1e-6 > pmin or pmax > 1.0 + 1e-6:
                raise ValueError("The predicted image should be normalized.")
            lp = None
            if self.lpips is not None:
                crop = dbg[i, :, :, : b - t, : r - l]
                if self.device.type == "cuda":  # pairs run one after another on the stream the composites were made on
                    with torch.cuda.device(self.device), torch.cuda.stream(self._stream()):
                        lp = float(self.lpips(crop[1][None], crop[0][None]))
                else:  # NOT a CPU path: only a stand-in for ops.eval_psnr_ssim (the non-GPU tests patch one in) gets this far without a device
                    lp = float(self.lpips(crop[1][None], crop[0][None]))
            res.append((psnr, ssim, lp))
        return res

    def __call__(self, pred: ImageLike, gt: ImageLike, pred_fmask: Optional[ImageLike] = None, gt_fmask: Optional[ImageLike] = None,
                 canvas_size: int = 1024, crop_with_fmask: bool = True, background_color: str = "black"):
        return self.evaluate_batch([dict(pred=pred, gt=gt, pred_fmask=pred_fmask, gt_fmask=gt_fmask, canvas_size=canvas_size,
                                         crop_with_fmask=crop_with_fmask, background_color=background_color)])[0]


# -- directories of results -------------------------------------------------------------------------------------------------------
def evaluation_keys(pred_images_dir: str, spa_labels: Optional[List[str]] = None, tem_labels: Optional[List[str]] = None) -> List[str]:
    """The reference's key enumeration: spa_labels x tem_labels, defaults from directory listings (metric_utils.py:184-190)."""
    if spa_labels is None:
        spa_labels = sorted(os.listdir(pred_images_dir))
    if tem_labels is None:
        tem_labels = sorted(os.listdir(f"{pred_images_dir}/{spa_labels[0]}"))
        tem_labels = [tem_label.split(".")[0] for tem_label in tem_labels]
    return [f"{spa_label}/{tem_label}" for spa_label in spa_labels for tem_label in tem_labels]


def evaluate_keys(keys: List[str], device, pred_images_dir: str, gt_images_dir: str, fmasks_dir: Optional[str] = None,
                  pred_image_ext: str = ".jpg", gt_image_ext: str = ".jpg", fmask_ext: str = ".png", crop_with_fmask: bool = True,
                  background_color: str = "black", canvas_size: int = 1024, lpips: Optional[Callable] = None, batch_size: int = 16,
                  decode_threads: int = 8, *, lpips_weights: Optional[Tuple[str, str]] = None, device_decode: bool = False) -> List[Dict]:
    """The reference's evaluate_on_single_gpu: [{key, psnr, ssim, lpips}] of `keys` on one device, `batch_size` pairs per launch.
    `lpips_weights` = (vgg16_path, lin_path): this worker builds its own ``LpipsVGG`` on `device` (instead of a `lpips` callable)."""
    if lpips_weights is not None:
        if lpips is not None:
            raise ValueError("pass either lpips= (a callable) or lpips_weights= (the two weight files), not both")
        lpips = _lpips.LpipsVGG(device, *lpips_weights)
    ev = ImageEvaluator(device, lpips=lpips, decode_threads=decode_threads, **({"device_decode": True} if device_decode else {}))
    res = []
    try:
        for i in range(0, len(keys), max(1, int(batch_size))):
            chunk = keys[i: i + max(1, int(batch_size))]
            pairs = []
            for key in chunk:
                fmask = f"{fmasks_dir}/{key}{fmask_ext}" if fmasks_dir is not None else None
                pairs.append(dict(pred=f"{pred_images_dir}/{key}{pred_image_ext}", gt=f"{gt_images_dir}/{key}{gt_image_ext}",
                                  pred_fmask=fmask, gt_fmask=fmask, canvas_size=canvas_size, crop_with_fmask=crop_with_fmask,
                                  background_color=background_color))
            for key, (psnr, ssim, lp) in zip(chunk, ev.evaluate_batch(pairs)):
                res.append({"key": key, "psnr": psnr, "ssim": ssim, "lpips": lp})
    finally:
        ev._pool.shutdown(wait=True)
    return res


def aggregate_metrics(values: List[Dict], out_metrics_path: Optional[str] = None) -> Dict:
    """{"mean": {...}, "values": [...]} as the reference writes it (metric_utils.py:222-234): values sorted by key, means taken in
    fp32 (torch.tensor(...).mean()) and rounded to 3 decimals; lpips is null where no LPIPS callable produced it."""
    metrics = {"mean": {}, "values": sorted(values, key=lambda x: x["key"])}
    mean = lambda name: round(torch.tensor([x[name] for x in metrics["values"]]).mean().item(), 3)
    have_lpips = bool(metrics["values"]) and all(x["lpips"] is not None for x in metrics["values"])
    metrics["mean"] = {"psnr": mean("psnr"), "ssim": mean("ssim"), "lpips": mean("lpips") if have_lpips else None}
    if out_metrics_path is not None:
        os.makedirs(os.path.dirname(out_metrics_path) or ".", exist_ok=True)
        with open(out_metrics_path, "w") as f:
            json.dump(metrics, f, indent=4)
    return metrics


def _device_of(gpu_id) -> torch.device:
    return torch.device(f"cuda:{gpu_id}") if isinstance(gpu_id, int) else torch.device(gpu_id)


def evaluate_results(pred_images_dir: str, gt_images_dir: str, fmasks_dir: Optional[str] = None, pred_image_ext: str = ".jpg",
                     gt_image_ext: str = ".jpg", fmask_ext: str = ".png", spa_labels: Optional[List[str]] = None,
                     tem_labels: Optional[List[str]] = None, out_metrics_path: Optional[str] = None, crop_with_fmask: bool = True,
                     background_color: str = "black", gpu_ids: Optional[List[int]] = None, *, canvas_size: int = 1024,
                     lpips: Optional[Callable] = None, batch_size: int = 16, decode_threads: int = 8,
                     lpips_weights: Optional[Tuple[str, str]] = None, device_decode: bool = False) -> Dict:
    """The reference's ``evaluate_results`` (its keyword list, its key enumeration, its JSON): one thread per entry of `gpu_ids`
    (default: every visible device) over ``keys[i::n]``.  Keyword-only extensions: `canvas_size` (the reference always uses the
    evaluator's default, 1024), `lpips` (a callable, see the module docstring) or `lpips_weights` = (vgg16_path, lin_path) (every worker
    thread builds its own ``LpipsVGG`` on its device), `batch_size` (pairs per launch), `decode_threads`, `device_decode` (baseline
    JPEG predictions and ground truths, and 8-bit PNG images and masks, are decoded on the device, host/jpegdec.py and
    host/pngdec.py: the same metrics.json)."""
    if lpips is not None and lpips_weights is not None:
        raise ValueError("pass either lpips= (a callable) or lpips_weights= (the two weight files), not both")
    keys = evaluation_keys(pred_images_dir, spa_labels, tem_labels)
    if gpu_ids is None:
        gpu_ids = list(range(torch.cuda.device_count()))
    if not gpu_ids:
        raise Dm4dError("evaluate_results: no HIP device (diffuman4d_amd has no CPU path)")
    if lpips is None and lpips_weights is None:
        log.info("LPIPS is not built: \"lpips\" is null in the metrics (pass lpips=callable to fill it)")
    n = len(gpu_ids)
    kw = dict(pred_images_dir=pred_images_dir, gt_images_dir=gt_images_dir, fmasks_dir=fmasks_dir, pred_image_ext=pred_image_ext,
              gt_image_ext=gt_image_ext, fmask_ext=fmask_ext, crop_with_fmask=crop_with_fmask, background_color=background_color,
              canvas_size=canvas_size, lpips=lpips, batch_size=batch_size, decode_threads=decode_threads)
    if lpips_weights is not None:
        kw["lpips_weights"] = tuple(lpips_weights)
    if device_decode:
        kw["device_decode"] = True
    with ThreadPoolExecutor(max_workers=n, thread_name_prefix="dm4d-eval") as ex:
        futures = [ex.submit(evaluate_keys, keys[i::n], _device_of(g), **kw) for i, g in enumerate(gpu_ids)]
        values = [v for f in futures for v in f.result()]
    return aggregate_metrics(values, out_metrics_path)
