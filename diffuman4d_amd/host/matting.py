"""Foreground-mask prediction around a caller-named matting network: the ``remove_background`` action of the reference's preprocess.sh
(scripts/preprocess/remove_background.py), which writes ``fmasks/{camera}/{frame}.png``, the files that ``host/vhull.py``,
``host/pose.py`` (``bbox_source="fmask"``), ``host/capture.py`` (``SpaTemDataset``) and ``host/metrics.py`` (``evaluate_results``) read.

The network (BiRefNet / RMBG-2.0 in the reference) is not part of this package and is never downloaded: the caller names a local
directory (``load_matting_model``) or hands over any callable (``matting_model``).  Everything around it runs on the device
(csrc/matting.hip):

  * ``matting_inputs``: images are decoded with Pillow in a thread pool into pinned staging and uploaded once as bytes (the buffer,
    its filling and the {tables | descriptors} pack are host/staging.py's; ``_plan`` says where every plane lies); at most two
    launches rotate them (an index map), resize them with Pillow's antialiased bilinear filter to the network's size and normalise them
    through a 3 x 256 table that torch CPU itself fills with the reference's arithmetic;
  * ``matting_masks``: the logits, which never visit the host, become bytes through the 65536-entry table of ``quantiser_table`` (the
    reference's ``.sigmoid()`` + ``to_pil_image`` in fp16, DESIGN.md "Foreground masks"), are resized with Pillow's bicubic filter to
    each image's size and turned back; one packed blob of mask planes comes back in one copy.

Both are byte-exact to the reference's Pillow + torch CPU route.  There is no CPU path: a ``device`` that is not a HIP device is an
error.

``remove_background(device_png=True)`` also keeps the mask planes and the staged source bytes on the device and lets host/png.py
encode the mask and RGBA PNG files there; only file bytes come down.  Those files decode to the same pixels as the default route's
and differ from them in bytes (DESIGN.md "Device PNG").
"""
from __future__ import annotations

import os
import threading
from concurrent.futures import ThreadPoolExecutor
from glob import glob
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from PIL import Image

from . import lib as _l
from . import ops
from . import staging as _st
from .codec import decode_or_fallback, read_file
from .resample import TableSet
from .staging import MAX_HOST_THREADS  # noqa: F401  (importable from here as before)

MEAN = (0.485, 0.456, 0.406)   # remove_background.py:20, the ImageNet constants
STD = (0.229, 0.224, 0.225)
IMAGE_SIZE = (1024, 1024)      # remove_background.py:15
FIELDS = _l.MATTING_FIELDS
ROTATIONS = (0, 90, 180, 270)


# -- the two tables (host) -------------------------------------------------------------------------------------------------------------
def normalisation_table(dtype: torch.dtype = torch.float16) -> torch.Tensor:
    """[3, 256] of `dtype` (fp16 or fp32) on the host: what ``ToTensor`` + ``Normalize(MEAN, STD)`` (+ ``.half()``) make of every byte
    of every channel, computed by torch CPU with the reference's own operations, so that a lookup is bit-equal to them."""
    if dtype not in (torch.float16, torch.float32):
        raise ValueError(f"dtype must be torch.float16 or torch.float32, got {dtype}")
    rows = [torch.arange(256).float().div(255).sub(m).div(s) for m, s in zip(MEAN, STD)]
    return torch.stack(rows).to(dtype).contiguous()


def quantiser_table() -> np.ndarray:
    """uint8 [65536]: fp16 bit pattern of a logit -> mask byte, by definition ``s = fp16(1 / (1 + exp(-x)))`` evaluated in fp64 and
    rounded once, ``m = fp16(fp32(s) * 255)``, byte = trunc(m); NaN -> 0.  The reference's ``.sigmoid()`` then ``to_pil_image``
    (``.mul(255).byte()``) in fp16, made independent of any device's exp: the device only looks values up."""
    x = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        s = (1.0 / (1.0 + np.exp(-x))).astype(np.float16)
        m = (s.astype(np.float32) * np.float32(255.0)).astype(np.float16)
        return np.where(np.isnan(x), 0, np.trunc(m.astype(np.float32))).astype(np.uint8)


_tables_lock = threading.Lock()
_device_tables: Dict[Tuple, torch.Tensor] = {}


def _on_device(kind, device: torch.device) -> torch.Tensor:
    """The normalisation table of a dtype (kind = the dtype) or the quantiser table (kind = "q") on `device`, uploaded once."""
    key = (kind, device)
    with _tables_lock:
        if key not in _device_tables:
            host = torch.from_numpy(quantiser_table()) if kind == "q" else normalisation_table(kind)
            _device_tables[key] = host.to(device)
        return _device_tables[key]


# -- staging ---------------------------------------------------------------------------------------------------------------------------
def _quarter_turns(rotate_clockwise: int) -> int:
    if rotate_clockwise not in ROTATIONS or isinstance(rotate_clockwise, bool):
        raise ValueError(f"rotate_clockwise must be one of 0, 90, 180, 270, got {rotate_clockwise!r}")
    return int(rotate_clockwise) // 90


def _open_all(images, pool: Optional[ThreadPoolExecutor]) -> Tuple[List, List[Tuple[int, int]]]:
    """Open (not yet decode) and check the images -> (PIL images, sizes [(h, w)]).  Needs no device."""
    images = list(images)
    if len(images) < 1:
        raise ValueError("images: at least one image")
    ims = _st.pool_map(pool, _st.open_image, images)
    return ims, _st.check_sizes([im.size[::-1] for im in ims], _l.MATTING_MAX_SIDE, "images")


def _plan(sizes: Sequence[Tuple[int, int]], net: Tuple[int, int], rot: int, to_net: bool):
    """Descriptors and tables of one launch for images of `sizes` = [(h, w)] as stored -> (desc int64 [n, FIELDS] with the plane offsets
    filled in, tab int32, plane bytes, scratch bytes).  to_net: images -> the network's size `net` = (S_h, S_w), bilinear, planes of 3
    bytes per pixel, scratch rh x S_w words; else: `net` -> the images' sizes, bicubic, planes of 1 byte, scratch S_h x rw bytes."""
    S_h, S_w = net
    ts = TableSet()
    desc = np.zeros((len(sizes), FIELDS), dtype=np.int64)
    planes, scratch = _st.Layout(), _st.Layout()
    for k, (h, w) in enumerate(sizes):
        rh, rw = (w, h) if rot & 1 else (h, w)
        row = desc[k]
        row[0], row[1], row[2] = planes.add(h * w * (3 if to_net else 1)), h, w
        pairs = ((rw, S_w), (rh, S_h)) if to_net else ((S_w, rw), (S_h, rh))
        for field, (n_in, n_out) in zip((3, 5), pairs):
            row[field], row[field + 1] = (-1, 0) if n_in == n_out else ts.add(n_in, n_out, "bilinear" if to_net else "bicubic")
        if row[3] >= 0:
            row[7] = scratch.add(rh * S_w * 4 if to_net else S_h * rw)
    tab = ts.array() if ts.tables else np.zeros(1, dtype=np.int32)  # the library wants a table even where no axis changes its size
    return desc, tab, planes.total, max(scratch.total, 16)


def _inputs(ims, sizes, size: Tuple[int, int], dev: torch.device, rot: int, dtype: torch.dtype, pool: Optional[ThreadPoolExecutor]) -> torch.Tensor:
    return _staged_inputs(ims, sizes, size, dev, rot, dtype, pool)[0]


def _device_files(ims, sizes) -> dict:
    """{index: (plan, file bytes)} of the images that were opened from baseline JPEG files of the set csrc/jpegdec.hip decodes."""
    from . import jpegdec
    out = {}
    for k, im in enumerate(ims):
        name = getattr(im, "filename", "")
        if im.format == "JPEG" and name and im.mode in ("RGB", "L"):
            data = read_file(name)
            plan = jpegdec.probe(data)
            if plan is not None and (plan.h, plan.w) == tuple(sizes[k]) and plan.mode == im.mode:
                out[k] = (plan, data)
    return out


def _staged_inputs(ims, sizes, size: Tuple[int, int], dev: torch.device, rot: int, dtype: torch.dtype, pool: Optional[ThreadPoolExecutor],
                   device_decode: bool = False):
    """-> (the network's input, the staged RGB bytes on the device: every image as stored, HWC with tight rows, its byte offsets).
    device_decode: images opened from supported JPEG files upload their file bytes and are decoded into their regions on the device
    (host/jpegdec.py; a grayscale file replicated, as convert("RGB") does); the others, and files the decoder refuses, keep the
    Pillow fill."""
    S_h, S_w = int(size[0]), int(size[1])
    if not (1 <= S_h <= _l.MATTING_MAX_SIDE and 1 <= S_w <= _l.MATTING_MAX_SIDE):
        raise ValueError(f"size {S_h} x {S_w} is outside 1..{_l.MATTING_MAX_SIDE}")
    desc, tab, plane_bytes, scratch_bytes = _plan(sizes, (S_h, S_w), rot, True)
    host = _st.pinned(plane_bytes, dev)
    on_device = _device_files(ims, sizes) if device_decode else {}
    _st.fill(host.numpy(), [(int(desc[k, 0]), (im, "RGB")) for k, im in enumerate(ims) if k not in on_device], pool)
    blob = host.to(dev, non_blocking=True)
    if on_device:
        from . import jpegdec
        ks = sorted(on_device)  # a scan the decoder refuses: Pillow's pixels (or Pillow's exception)
        decode_or_fallback(jpegdec, [(*on_device[k], int(desc[k, 0]), 3) for k in ks], blob, lambda j: np.asarray(ims[ks[j]].convert("RGB")))
    meta, meta_host, tab_off, tab_len, desc_off = _st.pack_meta(tab, desc, dev)
    scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=dev)
    out = ops.matting_input(blob, meta, meta_host, len(ims), desc_off, tab_off, tab_len, _on_device(dtype, dev), scratch, S_h, S_w, rot)
    torch.cuda.current_stream().synchronize()  # the pinned buffers may go; the tensor is complete when it is handed over
    return out, blob, [int(v) for v in desc[:, 0]]


def matting_inputs(images, size: Tuple[int, int] = IMAGE_SIZE, device="cuda", *, rotate_clockwise: int = 0, dtype: torch.dtype = torch.float16,
                   pool: Optional[ThreadPoolExecutor] = None) -> torch.Tensor:
    """The matting network's input for a batch of images -> `dtype` (fp16 or fp32) [n, 3, S_h, S_w] on `device`, bit-equal to the
    reference's ``transform_image(image.rotate(-rotate_clockwise, expand=True))`` (+ ``.half()`` for fp16).

    images: paths, PIL images or uint8 [h, w, 3] arrays, of any sizes from 1 to MATTING_MAX_SIDE (anything else is converted to RGB).
    size: the network's input (S_h, S_w); the aspect ratio is not kept, as in the reference.  rotate_clockwise: 0, 90, 180 or 270."""
    rot = _quarter_turns(rotate_clockwise)
    if dtype not in (torch.float16, torch.float32):
        raise ValueError(f"dtype must be torch.float16 or torch.float32, got {dtype}")
    ims, sizes = _open_all(images, pool)
    dev = _l.hip_device(device, "matting_inputs")
    with torch.cuda.device(dev):
        return _inputs(ims, sizes, size, dev, rot, dtype, pool)


def matting_masks(logits: torch.Tensor, sizes: Sequence[Tuple[int, int]], *, rotate_clockwise: int = 0) -> List[np.ndarray]:
    """The network's logits [n, 1, S_h, S_w] on the device (fp16; bf16 and fp32 are converted to fp16 there first), sizes = the images'
    [(h, w)] -> a list of uint8 [h, w] arrays, byte-equal to the reference's ``to_pil_image(logits.sigmoid()).resize((w', h'))``
    turned back by `rotate_clockwise` (w', h': the rotated image's size).  The planes are packed 16-byte aligned in one device blob and
    copied back once; the arrays are views of that one host buffer."""
    blob, offsets, sizes, _ = _mask_blob(logits, sizes, rotate_clockwise)
    host = blob.cpu().numpy()  # synchronises: the descriptors' host copy may go
    return [host[off: off + h * w].reshape(h, w) for off, (h, w) in zip(offsets, sizes)]


def _mask_blob(logits: torch.Tensor, sizes: Sequence[Tuple[int, int]], rotate_clockwise: int):
    """``matting_masks`` up to the copy: -> (the packed mask planes on the device, their byte offsets, the checked sizes, the host
    copy of the descriptors, which the caller keeps until it has synchronised the stream)."""
    rot = _quarter_turns(rotate_clockwise)
    if not isinstance(logits, torch.Tensor) or logits.device.type != "cuda":
        raise _l.Dm4dError("logits: expected a tensor on a HIP device (no CPU fallback in diffuman4d_amd)")
    if logits.dim() != 4 or logits.shape[1] != 1 or logits.numel() == 0:
        raise ValueError(f"logits: expected [n, 1, S_h, S_w], got {tuple(logits.shape)}")
    if logits.dtype not in (torch.float16, torch.bfloat16, torch.float32):
        raise ValueError(f"logits: expected fp16, bf16 or fp32, got {logits.dtype}")
    sizes = _st.check_sizes(sizes, _l.MATTING_MAX_SIDE, "sizes")
    n, _, S_h, S_w = logits.shape
    if len(sizes) != n:
        raise ValueError(f"sizes: expected one (h, w) per logit plane ({n}), got {len(sizes)}")
    if not (S_h <= _l.MATTING_MAX_SIDE and S_w <= _l.MATTING_MAX_SIDE):
        raise ValueError(f"logits: {S_h} x {S_w} is outside 1..{_l.MATTING_MAX_SIDE}")
    dev = logits.device
    with torch.cuda.device(dev):
        desc, tab, blob_bytes, scratch_bytes = _plan(sizes, (S_h, S_w), rot, False)
        meta, meta_host, tab_off, tab_len, desc_off = _st.pack_meta(tab, desc, dev)
        scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=dev)
        blob = ops.matting_mask(logits.to(torch.float16).contiguous(), meta, meta_host, n, desc_off, tab_off, tab_len, _on_device("q", dev),
                                scratch, blob_bytes, rot)
    return blob, [int(v) for v in desc[:, 0]], sizes, meta_host


# -- the stage -------------------------------------------------------------------------------------------------------------------------
def load_matting_model(model_name: str, device) -> Callable:
    """The caller's matting network from a local directory in the Hugging Face layout (a downloaded ``ZhengPeng7/BiRefNet`` or
    ``briaai/RMBG-2.0``), as the reference loads it (remove_background.py:25-33) but strictly offline:
    ``AutoModelForImageSegmentation.from_pretrained(dir, trust_remote_code=True, local_files_only=True)``, then ``.eval().half()``.
    A `model_name` that is not an existing directory (a hub name, for instance) raises FileNotFoundError before ``transformers`` is
    even imported: nothing is ever downloaded.

    This path has not been run: no checkpoint is at hand, and the tests go through ``matting_model``."""
    if not isinstance(model_name, (str, os.PathLike)) or not os.path.isdir(model_name):
        raise FileNotFoundError(f"matting network {model_name!r} is not a local directory (it is never downloaded: name a directory that "
                                "holds the checkpoint)")
    from transformers import AutoModelForImageSegmentation
    model = AutoModelForImageSegmentation.from_pretrained(os.fspath(model_name), trust_remote_code=True, local_files_only=True)
    return model.to(device).eval().half()


def list_inputs(images_dir: str, out_fmasks_dir: str, out_images_alpha_dir: Optional[str] = None, image_ext: str = ".webp",
                mask_ext: str = ".png") -> Tuple[List[str], List[str], List[Optional[str]]]:
    """``**/*{image_ext}`` under images_dir, sorted, and each one's mask and RGBA path: the image path with `image_ext` replaced by
    `mask_ext` (``.png`` for the RGBA image) and `images_dir` by the output directory, in that order (remove_background.py:124-131)."""
    images = sorted(glob(f"{images_dir}/**/*{image_ext}", recursive=True))
    fmasks = [p.replace(image_ext, mask_ext).replace(images_dir, out_fmasks_dir) for p in images]
    if out_images_alpha_dir is not None:
        alphas: List[Optional[str]] = [p.replace(image_ext, ".png").replace(images_dir, out_images_alpha_dir) for p in images]
    else:
        alphas = [None] * len(images)
    return images, fmasks, alphas


def _verifies(path: str) -> bool:
    try:
        with Image.open(path) as im:
            im.verify()
        return True
    except Exception:
        return False


def pending_batches(fmask_paths: Sequence[str], batch_size: int, skip_exists: bool) -> Tuple[List[List[int]], int]:
    """The batches of indices that have to be predicted, in order, and the number of images skipped.  The reference's rule
    (remove_background.py:56-70): batches are cut before anything is skipped, and with `skip_exists` a batch is skipped only if every
    mask of it exists and ``Image.open(...).verify()`` accepts it; one missing or damaged mask reruns its whole batch."""
    batches = [list(range(i, min(i + batch_size, len(fmask_paths)))) for i in range(0, len(fmask_paths), batch_size)]
    if not skip_exists:
        return batches, 0
    todo = [b for b in batches if not all(os.path.exists(fmask_paths[k]) and _verifies(fmask_paths[k]) for k in b)]
    return todo, len(fmask_paths) - sum(len(b) for b in todo)


def write_mask(mask: np.ndarray, fmask_path: str, image_src=None, image_alpha_path: Optional[str] = None) -> None:
    """``Image.fromarray(mask).save(fmask_path)`` and, with `image_alpha_path`, the image (in its stored orientation) with the mask as
    its alpha channel (``putalpha``, remove_background.py:89-93).  Both appear atomically."""
    _st.atomic_write(fmask_path, Image.fromarray(mask).save)
    if image_alpha_path is not None:
        write_image_alpha(mask, image_src, image_alpha_path)


def write_image_alpha(mask: np.ndarray, image_src, image_alpha_path: str) -> None:
    """The image (in its stored orientation) with `mask` as its alpha channel (``putalpha``), written atomically."""
    image = _st.open_image(image_src).copy()
    image.putalpha(Image.fromarray(mask))
    _st.atomic_write(image_alpha_path, image.save)


def _store_bytes(path: str, data: bytes) -> None:
    def write(tmp):
        with open(tmp, "wb") as f:
            f.write(data)
    _st.atomic_write(path, write)


def _store_device_files(fmask_path: str, fmask_file: bytes, image_alpha_path: Optional[str], alpha_file: Optional[bytes], mask, image_src) -> None:
    """One image of the `device_png` route: the files the device encoded are stored verbatim; an RGBA file the device did not encode
    (the stored image is not RGB) is written by ``write_image_alpha`` from the mask plane `mask`."""
    _store_bytes(fmask_path, fmask_file)
    if image_alpha_path is not None:
        if alpha_file is not None:
            _store_bytes(image_alpha_path, alpha_file)
        else:
            write_image_alpha(mask, image_src, image_alpha_path)


def remove_background(images_dir: str, out_fmasks_dir: str, out_images_alpha_dir: Optional[str] = None, model_name: Optional[str] = None,
                      image_ext: str = ".webp", mask_ext: str = ".png", rotate_clockwise: int = 0, batch_size: int = 8, num_workers: int = 4,
                      skip_exists: bool = False, gpu_ids: Optional[Sequence[int]] = None, *, matting_model: Optional[Callable] = None,
                      image_size: Tuple[int, int] = IMAGE_SIZE, device_png: bool = False, device_decode: bool = False) -> dict:
    """Predict the foreground mask of every ``**/*{image_ext}`` under `images_dir` and write ``out_fmasks_dir/{camera}/{frame}{mask_ext}``
    (and the RGBA images under `out_images_alpha_dir`), with the reference's arguments in its names and order.

    matting_model: any callable taking fp16 [n, 3, S_h, S_w] on the device and returning a tensor [n, 1, S_h, S_w] of logits on the
    device, or a list / tuple of tensors of which the last is taken (BiRefNet's side outputs); by default
    ``load_matting_model(model_name)``, once per GPU.  It is the caller's network: its output never visits the host.  One worker thread
    per GPU id; decoding and the PNG files go through a pool of `num_workers` threads.  Returns counts.

    device_png: the mask planes and the staged source bytes stay on the device and host/png.py encodes ``fmasks/*.png`` (L) and, with
    `out_images_alpha_dir`, ``images_alpha/*.png`` (RGBA = staged RGB + mask) there; only file bytes come down and the pool's threads
    store them.  The files decode to the same pixels as the default route's and differ from them in bytes (DESIGN.md "Device PNG").
    `mask_ext` must be ``.png``.  An image whose stored mode is not RGB gets its RGBA file from the default route's ``putalpha``.

    device_decode: inputs that are baseline JPEG files of the supported set (host/jpegdec.py::probe) are not decoded by Pillow: their
    file bytes go up and csrc/jpegdec.hip decodes them into the staged RGB regions, byte for byte Pillow's pixels, so every file
    written is the same as without it.  Other inputs keep the Pillow route."""
    rot = _quarter_turns(rotate_clockwise)
    if device_png and mask_ext != ".png":
        raise ValueError(f"device_png writes PNG files: mask_ext must be '.png', got {mask_ext!r}")
    if matting_model is None:
        if not model_name:
            raise ValueError("name the matting network: model_name (a local directory) or matting_model (a callable)")
        if not os.path.isdir(model_name):
            load_matting_model(model_name, "cpu")  # raises: a hub name is refused before anything runs
    if batch_size < 1:
        raise ValueError("batch_size must be at least 1")
    size = (int(image_size[0]), int(image_size[1]))
    images, fmasks, alphas = list_inputs(images_dir, out_fmasks_dir, out_images_alpha_dir, image_ext, mask_ext)
    batches, skipped = pending_batches(fmasks, batch_size, skip_exists)
    result = {"images": len(images), "written": 0, "skipped": skipped}
    if not batches:
        return result

    def process_batch(model: Callable, batch: List[int], dev: torch.device, pool: ThreadPoolExecutor) -> List:
        ims, sizes = _open_all([images[k] for k in batch], pool)
        net_in, staged, src_at = _staged_inputs(ims, sizes, size, dev, rot, torch.float16, pool, device_decode)
        out = model(net_in)
        if isinstance(out, (list, tuple)) and len(out) > 0:
            out = out[-1]
        if not isinstance(out, torch.Tensor) or out.device.type != "cuda" or tuple(out.shape) != (len(batch), 1) + size:
            raise _l.Dm4dError(f"matting_model: expected a [{len(batch)}, 1, {size[0]}, {size[1]}] tensor on the device (or a list "
                               "of tensors that ends in one)")
        if not device_png:
            del staged
            masks = matting_masks(out, sizes, rotate_clockwise=rotate_clockwise)
            return [pool.submit(write_mask, masks[r], fmasks[k], images[k], alphas[k]) for r, k in enumerate(batch)]
        from . import png
        blob, mask_at, _, keep = _mask_blob(out, sizes, rotate_clockwise)
        items = [(png.L, h, w, mask_at[r], w) for r, (h, w) in enumerate(sizes)]
        rgba = [r for r, k in enumerate(batch) if alphas[k] is not None and ims[r].mode == "RGB"]
        items += [(png.RGBA, sizes[r][0], sizes[r][1], src_at[r], 3 * sizes[r][1], mask_at[r], sizes[r][1]) for r in rgba]
        files = png.png_encode_planes(blob, staged if rgba else None, items)  # synchronises
        del keep
        alpha_file = {r: files[len(batch) + j] for j, r in enumerate(rgba)}
        writes = []
        for r, k in enumerate(batch):
            h, w = sizes[r]
            host_mask = None
            if alphas[k] is not None and r not in alpha_file:
                host_mask = blob[mask_at[r]: mask_at[r] + h * w].cpu().numpy().reshape(h, w)
            writes.append(pool.submit(_store_device_files, fmasks[k], files[r], alphas[k], alpha_file.get(r), host_mask, images[k]))
        return writes

    load_model = lambda dev: matting_model if matting_model is not None else load_matting_model(model_name, dev)
    result["written"] = _st.run_stage("remove_background", gpu_ids, num_workers, "dm4d-matting", batches, load_model, process_batch)
    return result
