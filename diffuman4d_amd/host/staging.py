"""The host's way to the device, written once for every module that stages bytes for a kernel (``capture``, ``metrics``, ``pose``,
``matting``, ``rectify``) or drives a per-GPU stage (``pose.predict_keypoints``, ``matting.remove_background``, ``rectify.extract_images``):

  * ``Layout``: byte offsets of the regions of one buffer (planes, int32 tables, int64 descriptors), each 16-byte aligned;
  * ``pinned`` + ``fill``: the host buffer (page-locked when it goes to a HIP device) and its filling from arrays or from PIL images
    that are converted, and so decoded, in the pool's threads;
  * ``write_meta`` / ``pack_meta``: tables and descriptors into a view at given offsets, or as a buffer ``{tab | desc}`` of their own;
  * ``run_stage``: device resolution, the decode / write pool, one worker thread per GPU id with its own stream, and the collection of
    the write futures;
  * ``pool_map``, ``open_image``, ``check_sizes``, ``atomic_write``, ``MAX_HOST_THREADS``.

Nothing here launches a kernel.
"""
from __future__ import annotations

import os
import threading
from concurrent.futures import ThreadPoolExecutor
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch
from PIL import Image

from . import lib as _l

MAX_HOST_THREADS = 16  # the widest decode / write pool a stage opens, whatever num_workers asks for


# -- layout, buffer, fill --------------------------------------------------------------------------------------------------------------
class Layout:
    """Offsets of the regions of one staging buffer: ``add(nbytes)`` -> where the region starts; the next one starts at the following
    multiple of 16.  ``total``: the bytes the buffer needs (a multiple of 16)."""

    def __init__(self, start: int = 0):
        self.total = _l.align16(start)

    def add(self, nbytes: int) -> int:
        off = self.total
        self.total = _l.align16(off + int(nbytes))
        return off


def pinned(nbytes: int, device: torch.device) -> torch.Tensor:
    """An uninitialised host uint8 buffer, page-locked when `device` is a HIP device.  ``.to(device, non_blocking=True)`` only queues
    the copy: the caller keeps the buffer referenced until it has synchronised the stream the copy was queued on."""
    return torch.empty(nbytes, dtype=torch.uint8, pin_memory=torch.device(device).type == "cuda")


def pool_map(pool: Optional[ThreadPoolExecutor], fn: Callable, xs) -> List:
    """``[fn(x) for x in xs]``, through `pool` when there is one."""
    return list(pool.map(fn, xs)) if pool is not None else [fn(x) for x in xs]


def fill(view: np.ndarray, jobs: Sequence[Tuple[int, object]], pool: Optional[ThreadPoolExecutor]) -> None:
    """Copy every job's bytes to its offset of `view` (uint8).  A job is (offset, source); a source is an ndarray of any dtype or a
    (PIL image, mode) pair, which is converted -- and with that decoded -- by the thread that copies it."""
    def put(job):
        off, src = job
        if isinstance(src, tuple):
            src = np.asarray(src[0].convert(src[1]))
        flat = np.ascontiguousarray(src).reshape(-1).view(np.uint8)
        np.copyto(view[off: off + flat.size], flat)
    pool_map(pool, put, jobs)


# -- tables and descriptors ------------------------------------------------------------------------------------------------------------
def write_meta(view: np.ndarray, tab: Optional[np.ndarray], tab_off: int, desc: np.ndarray, desc_off: int) -> None:
    """The int32 tables `tab` (None: none) at byte `tab_off` of `view` and the int64 descriptors `desc` at byte `desc_off`."""
    if tab is not None:
        view[tab_off: tab_off + tab.nbytes] = tab.view(np.uint8)
    view[desc_off: desc_off + desc.nbytes] = desc.reshape(-1).view(np.uint8)


def pack_meta(tab: Optional[np.ndarray], desc: np.ndarray, device: torch.device) -> Tuple[torch.Tensor, torch.Tensor, int, int, int]:
    """{tab at byte 0 | desc at the next multiple of 16} in a buffer of its own, queued for upload -> (meta on `device`, its host copy,
    tab_off, tab_len in int32 elements, desc_off).  The gap is zero.  tab None: descriptors alone, desc_off 0."""
    lay = Layout()
    tab_bytes = 0 if tab is None else tab.nbytes
    tab_off = lay.add(tab_bytes)
    desc_off = lay.add(desc.nbytes)
    host = pinned(lay.total, device)
    host.numpy()[tab_bytes: desc_off] = 0
    write_meta(host.numpy(), tab, tab_off, desc, desc_off)
    return host.to(device, non_blocking=True), host, tab_off, tab_bytes // 4, desc_off


# -- small helpers ---------------------------------------------------------------------------------------------------------------------
def open_image(src) -> Image.Image:
    """A path, a PIL image or an array -> a PIL image (not yet decoded for a path)."""
    if isinstance(src, Image.Image):
        return src
    if isinstance(src, np.ndarray):
        return Image.fromarray(src)
    return Image.open(os.fspath(src))


def check_sizes(sizes, max_side: int, name: str) -> List[Tuple[int, int]]:
    """`sizes` = [(h, w)] as ints, each side within 1..max_side; else ValueError naming ``{name}[k]`` (and, where the name does not
    say so itself, that it is a size)."""
    sizes = [(int(h), int(w)) for h, w in sizes]
    noun = "" if name.startswith("size") else "size "
    for k, (h, w) in enumerate(sizes):
        if not (1 <= h <= max_side and 1 <= w <= max_side):
            raise ValueError(f"{name}[{k}]: {noun}{w} x {h} is outside 1..{max_side}")
    return sizes


def atomic_write(path: str, write_fn: Callable[[str], object]) -> None:
    """``write_fn(tmp)`` then ``os.replace(tmp, path)``: a reader (or a skip_exists pass) never sees half a file.  The temporary file
    sits beside `path`, is this thread's own and keeps the extension (Pillow picks the format by it)."""
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    root, ext = os.path.splitext(path)
    tmp = f"{root}.tmp{threading.get_ident()}{ext}"
    write_fn(tmp)
    os.replace(tmp, path)


# -- the stage driver ------------------------------------------------------------------------------------------------------------------
def run_stage(what: str, gpu_ids: Optional[Sequence[int]], num_workers: int, thread_prefix: str, batches: Sequence,
              load_model: Callable, process_batch: Callable) -> int:
    """Run `batches` over the GPUs of `gpu_ids` (None: every visible one) -> the number of completed writes.

    One worker thread per GPU id takes ``batches[g::n]`` on its device, on a stream of its own and without autograd: it calls
    ``load_model(device)`` once and ``process_batch(model, batch, device, pool)`` per batch, which returns the futures of the files it
    has handed to `pool`, the one pool of min(num_workers, MAX_HOST_THREADS) threads that decoding and writing share.  The first
    exception of a worker or of a write is raised here; the pool is shut down either way."""
    if gpu_ids is None:
        gpu_ids = list(range(torch.cuda.device_count()))
    devices = [_l.hip_device(f"cuda:{int(g)}", what) for g in gpu_ids]
    if not devices:
        raise _l.Dm4dError(f"{what}: no HIP device is available (no CPU fallback in diffuman4d_amd)")
    pool = ThreadPoolExecutor(max_workers=max(1, min(int(num_workers), MAX_HOST_THREADS)), thread_name_prefix=thread_prefix)

    def worker(g: int) -> List:
        dev, writes = devices[g], []
        with torch.cuda.device(dev), torch.cuda.stream(torch.cuda.Stream(device=dev)), torch.no_grad():
            model = load_model(dev)
            for batch in batches[g::len(devices)]:
                writes += process_batch(model, batch, dev, pool)
        return writes

    written = 0
    try:
        with ThreadPoolExecutor(max_workers=len(devices), thread_name_prefix=f"{thread_prefix}-gpu") as gpus:
            for fut in [gpus.submit(worker, g) for g in range(len(devices))]:
                for w in fut.result():
                    w.result()
                    written += 1
    finally:
        pool.shutdown(wait=True)
    return written
