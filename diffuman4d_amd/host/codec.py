"""What the image codecs (``jpeg``, ``png``, ``webp``, ``jpegdec``, ``pngdec``) and their consumers (``metrics``, ``matting``, ``vhull``,
``capture``, ``pose``) say around the library calls, written once:

  * ``read_file``, ``pillow_pixels``: a file's bytes, and the Pillow route of a file;
  * ``chunks``: the ranges of a batch whose device memory stays within a budget;
  * ``require_device_u8``, ``gather``: an encoder's check of an input tensor, and its inputs as places in one device buffer;
  * ``workspace``, ``read_back``: the workspace tensor of a call, and the files of an encoder call brought to the host;
  * ``decode_plans``, ``decode_batch``: the bodies of a decoder module's ``decode_plans`` and ``decode_*_batch``;
  * ``decode_or_fallback``: one ``decode_plans`` call into a consumer's buffer, the refused files filled in by the consumer;
  * ``StagedFile``, ``probe_file``, ``decode_staged``: a file of either decoder that stands in a consumer's staging plan where its
    pixels would (``capture``, ``pose``), and one ``decode_or_fallback`` per codec over a mixed list of them, with ``decode_batch``'s stats.

A `codec` is a decoder module (``jpegdec``, ``pngdec``): ``probe``, ``stage_chunk``, ``launch_chunk``, ``decode_plans``, and plans with
``h``, ``w``, ``bytes_per_pixel``, ``workspace_need`` and ``payload_len``.  Its attributes are looked up when they are called.
Nothing here launches a kernel.
"""
from __future__ import annotations

import io
from pathlib import Path
from typing import Callable, List, Optional, Sequence, Tuple

from . import lib as _l

MAX_DECODE_CHUNK = 65535  # files of one decoder call (the libraries' limit on n)


def read_file(f) -> bytes:
    """A file's bytes: `f` is a path, or the bytes themselves."""
    if isinstance(f, (bytes, bytearray, memoryview)):
        return bytes(f)
    return Path(f).read_bytes()


def pillow_pixels(data: bytes):
    """The Pillow route: ``np.asarray(Image.open(file))``.  Raises what Pillow raises."""
    import numpy as np
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im)


def chunks(needs: Sequence[int], budget: int, cap: Optional[int] = None) -> List[Tuple[int, int]]:
    """The ranges [first, last) of consecutive items whose needs add up to at most `budget`, of at most `cap` items (None: any
    number).  A range holds at least one item: an item over the budget stands alone."""
    out = []
    first = 0
    while first < len(needs):
        last, used = first, 0
        while last < len(needs) and (cap is None or last - first < cap):
            if last > first and used + needs[last] > budget:
                break
            used += needs[last]
            last += 1
        out.append((first, last))
        first = last
    return out


def workspace(nbytes: int, dev):
    """An uninitialised device workspace of at least `nbytes`, in 16-byte units (an int64 tensor: ``numel() * 8`` bytes)."""
    import torch
    return torch.empty((nbytes + 15) // 16 * 2, dtype=torch.int64, device=dev)


def require_device_u8(t, name: str):
    """`t` is a uint8 tensor on a HIP device, or a Dm4dError that names it `name`."""
    import torch
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise _l.Dm4dError(f"{name}: expected a tensor on a HIP device (no CPU fallback in diffuman4d_amd)")
    if t.dtype != torch.uint8:
        raise _l.Dm4dError(f"{name}: expected uint8, got {t.dtype}")
    return t


def gather(tensors, bpp: int):
    """Tensors [h, w] (`bpp` 1) or [h, w, bpp] of one byte a channel -> (one uint8 buffer, [(byte offset, row stride)]): the tensors'
    common storage where they share one and their pixels are contiguous within a row, else a copy of them back to back.  The stride
    of a dimension of size 1 says nothing: a one-row view's row stride is at least its row."""
    import torch
    base = tensors[0].untyped_storage().data_ptr()
    rows_ok = all(t.stride(1) == bpp and (bpp == 1 or t.stride(2) == 1) and (t.shape[0] == 1 or t.stride(0) >= t.shape[1] * bpp)
                  for t in tensors)
    if rows_ok and all(t.untyped_storage().data_ptr() == base for t in tensors):
        buf = torch.empty(0, dtype=torch.uint8, device=tensors[0].device).set_(tensors[0].untyped_storage())
        return buf, [(t.data_ptr() - base, max(int(t.stride(0)), int(t.shape[1]) * bpp)) for t in tensors]
    buf = torch.cat([t.reshape(-1) for t in tensors])
    at, off = [], 0
    for t in tensors:
        at.append((off, int(t.shape[1]) * bpp))
        off += t.numel()
    return buf, at


def read_back(blob, out) -> List[bytes]:
    """The n files of an encoder call: `blob` is the device uint8 buffer they lie in back to back, `out` the device int64 [2 n] tensor
    of their offsets, then their lengths.  One synchronisation (the lengths) and one copy of exactly the bytes produced."""
    import torch
    n = out.numel() // 2
    where = out.cpu().tolist()
    total = where[n - 1] + where[2 * n - 1]
    host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
    host.copy_(blob[:total])
    data = host.numpy().tobytes()
    return [data[where[k]:where[k] + where[n + k]] for k in range(n)]


def decode_plans(codec, plans, files, out, offsets, channels, workspace_bytes: int) -> List[int]:
    """`codec`'s ``decode_plans``: the argument checks, then one ``stage_chunk`` and ``launch_chunk`` per chunk of files whose workspace
    stays below `workspace_bytes`; one synchronisation, at the end -> the status words."""
    import torch
    from .ops import _req
    _req(out, "out", torch.uint8)
    if not out.is_contiguous():
        raise _l.Dm4dError("out: expected a contiguous uint8 tensor")
    if not (len(plans) == len(files) == len(offsets) == len(channels)):
        raise ValueError("decode_plans: plans, files, offsets and channels differ in length")
    statuses = []
    with torch.cuda.device(out.device):
        for first, last in chunks([p.workspace_need for p in plans], workspace_bytes, MAX_DECODE_CHUNK):
            staged = codec.stage_chunk(plans[first:last], files[first:last], offsets[first:last], channels[first:last], out.device)
            statuses.append(codec.launch_chunk(staged, out))
        return torch.cat(statuses).cpu().tolist() if statuses else []


def decode_batch(codec, what: str, files, device, workspace_bytes: int, stats: Optional[dict]) -> list:
    """`codec`'s ``decode_*_batch`` (`what`: its name): files (paths or bytes) -> uint8 device tensors [h, w] or [h, w, c].  The files
    ``codec.probe`` takes are decoded into one buffer by one ``codec.decode_plans`` call; the others, and those with a nonzero status,
    are ``pillow_pixels`` of the file, uploaded.  stats: "device", "pillow" and "bytes_uploaded" are added to."""
    import torch
    dev = _l.hip_device(device, what)
    datas = [read_file(f) for f in files]
    plans = [codec.probe(d) for d in datas]
    ours = [k for k, p in enumerate(plans) if p is not None]
    offsets, total = [], 0
    for k in ours:
        offsets.append(total)
        total += _l.align16(plans[k].h * plans[k].w * plans[k].bytes_per_pixel)
    out = [None] * len(datas)
    uploaded = 0
    if ours:
        buf = torch.empty(total, dtype=torch.uint8, device=dev)
        st = codec.decode_plans([plans[k] for k in ours], [datas[k] for k in ours], buf, offsets, [plans[k].bytes_per_pixel for k in ours],
                                workspace_bytes)
        for k, at, s in zip(ours, offsets, st):
            p = plans[k]
            uploaded += p.payload_len
            if s == 0:
                shape = (p.h, p.w) if p.bytes_per_pixel == 1 else (p.h, p.w, p.bytes_per_pixel)
                out[k] = buf[at:at + p.h * p.w * p.bytes_per_pixel].view(shape)
    routed = 0
    for k in range(len(datas)):
        if out[k] is None:
            a = pillow_pixels(datas[k])
            out[k] = torch.from_numpy(a.copy()).to(dev)
            uploaded += a.nbytes
            routed += 1
    if stats is not None:
        stats["device"] = stats.get("device", 0) + len(datas) - routed
        stats["pillow"] = stats.get("pillow", 0) + routed
        stats["bytes_uploaded"] = stats.get("bytes_uploaded", 0) + uploaded
    return out


class StagedFile:
    """A file that `codec` (``jpegdec`` or ``pngdec``) will decode into its region of a consumer's device buffer: it stands where the
    decoded uint8 array would, with the plan's ``h``, ``w``, ``mode`` and ``nbytes``, and holds the file's bytes instead of pixels."""

    def __init__(self, path, codec, plan, data: bytes):
        self.path, self.codec, self.plan, self.data = path, codec, plan, data
        self.h, self.w, self.mode = plan.h, plan.w, plan.mode
        self.nbytes = plan.h * plan.w * plan.bytes_per_pixel


def probe_file(path, codecs: Sequence) -> Optional[StagedFile]:
    """Read the file at `path` and ask each of `codecs` in turn -> the StagedFile of the first that takes it, or None (the file keeps its
    Pillow route).  Nothing is decoded."""
    data = read_file(path)
    for codec in codecs:
        plan = codec.probe(data)
        if plan is not None:
            return StagedFile(path, codec, plan, data)
    return None


def decode_staged(entries: Sequence[Tuple[int, StagedFile, int]], buf, fallback: Callable[[StagedFile], object], stats: Optional[dict] = None) -> None:
    """Decode `entries` = [(byte offset in `buf`, file, output channels)] into the uint8 device buffer `buf`: one ``decode_or_fallback``
    per codec on the current stream; ``fallback(file)`` gives the pixels of a file its decoder refused.  stats: "device", "pillow" and
    "bytes_uploaded" are added to, as ``decode_batch`` counts them."""
    for codec in dict.fromkeys(f.codec for _, f, _ in entries):
        part = [e for e in entries if e[1].codec is codec]
        status = decode_or_fallback(codec, [(f.plan, f.data, off, ch) for off, f, ch in part], buf, lambda k: fallback(part[k][1]))
        if stats is not None:
            refused = sum(1 for s in status if s)
            stats["device"] = stats.get("device", 0) + len(part) - refused
            stats["pillow"] = stats.get("pillow", 0) + refused
            stats["bytes_uploaded"] = stats.get("bytes_uploaded", 0) + sum(f.plan.payload_len for _, f, _ in part) + \
                sum(off_f[1].h * off_f[1].w * off_f[2] for off_f, s in zip(part, status) if s)


def decode_or_fallback(codec, entries: Sequence[Tuple], buf, fallback: Callable[[int], object]) -> List[int]:
    """Decode `entries` = [(plan, file bytes, byte offset in `buf`, output channels)] into the uint8 device buffer `buf` with one
    ``codec.decode_plans`` call -> the status words.  Where the decoder refused a file (a nonzero status), ``fallback(k)``, the
    pixels of entry k as a uint8 array, is copied into the entry's region instead; what `fallback` raises is raised here."""
    import numpy as np
    import torch
    plans, files, offsets, channels = ([e[i] for e in entries] for i in range(4))
    status = codec.decode_plans(plans, files, buf, offsets, channels)
    for k, s in enumerate(status):
        if s:
            px = np.array(fallback(k)).reshape(-1)  # a copy: Pillow's arrays are read-only
            buf[offsets[k]: offsets[k] + px.size].copy_(torch.from_numpy(px))
    return status
