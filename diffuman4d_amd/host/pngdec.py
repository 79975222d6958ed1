"""8-bit PNG files decoded on the device, byte for byte what ``np.asarray(Image.open(file))`` of Pillow gives.

``probe`` reads a file's chunks on the host and says whether the device decoder takes it (bit depth 8, colour type 0 / 2 / 6 = modes
``L`` / ``RGB`` / ``RGBA``, not interlaced, every CRC right, no ``tRNS`` / ``acTL`` / ``CgBI``); every other file keeps its Pillow route.
``decode_plans`` uploads the concatenated IDAT payloads and has csrc/pngdec.hip decode the batch into a caller-given device buffer at
caller-given offsets (``dm4d_png_decode_u8``): one workgroup per image inflates the zlib stream through an LDS window into the filtered
scanlines, a second launch undoes the row filters in a skewed wavefront.  ``decode_png_batch`` is the list-in, tensors-out form.
What is specific to PNG is here (``probe``, ``Plan``, ``stage_chunk``, ``launch_chunk``); the chunked driver behind ``decode_plans``,
the body of ``decode_png_batch`` and the Pillow route are host/codec.py's, shared with host/jpegdec.py.
DESIGN.md "Device PNG decode" has the definition; tests/pngdec_model.py is the same in numpy.  There is no CPU path: a non-HIP device
is an error.
"""
from __future__ import annotations

import struct
import sys
import zlib
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

from . import codec as _c
from . import lib as _l

_this = sys.modules[__name__]  # the codec of host/codec.py's bodies: its attributes are looked up when they are called

DEFAULT_WORKSPACE = 1 << 30
MAX_ROW_BYTES = 32768         # lib.PNGDEC_MAX_ROW_BYTES: a band's last row is kept in LDS
MAX_STREAM_BYTES = 1 << 28    # lib.PNGDEC_MAX_STREAM_BYTES: bit positions of a stream are 32-bit on the device
SIGNATURE = b"\x89PNG\r\n\x1a\n"
_MODES = {0: (1, "L"), 2: (3, "RGB"), 6: (4, "RGBA")}
_REFUSED = (b"tRNS", b"acTL", b"CgBI")


@dataclass(frozen=True)
class Plan:
    """What the device needs of one supported file: the size, the channels and where the zlib stream's pieces lie."""
    h: int
    w: int
    channels: int       # 1 (mode "L"), 3 ("RGB") or 4 ("RGBA")
    mode: str
    idat: Tuple[Tuple[int, int], ...]  # [start, end) of every IDAT payload in the file, in order

    @property
    def filtered_bytes(self) -> int:
        """bytes of the filtered scanlines = what the zlib stream must inflate to"""
        return self.h * (1 + self.w * self.channels)

    # what host/codec.py asks of a plan
    @property
    def bytes_per_pixel(self) -> int:
        return self.channels

    @property
    def workspace_need(self) -> int:
        """bytes of the workspace: the filtered scanlines, 16-byte aligned"""
        return _l.align16(self.filtered_bytes)

    @property
    def payload_len(self) -> int:
        """bytes of the file that go up: the zlib stream"""
        return sum(e - s for s, e in self.idat)

    def stream_bytes(self, data: bytes) -> bytes:
        """The zlib stream: the IDAT payloads joined."""
        return b"".join(bytes(data[s:e]) for s, e in self.idat)


def probe(data) -> Optional[Plan]:
    """The plan of a file the device decoder takes, or None (the file keeps its Pillow route).  Host only; nothing is decoded."""
    data = bytes(data)
    n = len(data)
    if data[:8] != SIGNATURE:
        return None
    pos = 8
    header = None
    idat: List[Tuple[int, int]] = []
    closed = False  # an IDAT run has ended
    while True:
        if pos + 12 > n:
            return None  # no IEND
        length, kind = struct.unpack_from(">I4s", data, pos)
        if length > 0x7FFFFFFF or pos + 12 + length > n:
            return None
        body = data[pos + 8:pos + 8 + length]
        if zlib.crc32(body, zlib.crc32(kind)) != struct.unpack_from(">I", data, pos + 8 + length)[0]:
            return None
        if header is None:
            if kind != b"IHDR" or length != 13:
                return None
            header = struct.unpack(">IIBBBBB", body)
        elif kind == b"IHDR" or kind in _REFUSED:
            return None
        elif kind == b"IDAT":
            if closed:
                return None
            idat.append((pos + 8, pos + 8 + length))
        elif kind == b"IEND":
            break
        else:
            if not (kind[0] & 0x20) or not all(65 <= c <= 90 or 97 <= c <= 122 for c in kind):
                return None  # an unknown critical chunk, or no chunk name at all
            closed = closed or bool(idat)
        pos += 12 + length
    w, h, depth, colour, compression, filtering, interlace = header
    if depth != 8 or colour not in _MODES or compression or filtering or interlace or w < 1 or h < 1 or not idat:
        return None
    channels, mode = _MODES[colour]
    total = sum(e - s for s, e in idat)
    if w * channels > MAX_ROW_BYTES or not 2 <= total < MAX_STREAM_BYTES or h * (1 + w * channels) >= 1 << 31:
        return None
    return Plan(h, w, channels, mode, tuple(idat))


def decode_plans(plans: Sequence[Plan], files: Sequence[bytes], out, offsets: Sequence[int], channels: Sequence[int],
                 workspace_bytes: int = DEFAULT_WORKSPACE) -> List[int]:
    """Decode files[k] (whose plan is plans[k]) into the uint8 device tensor `out` at byte offsets[k], rows tight, channels[k] bytes a
    pixel (the file's own count).  -> the status words: nonzero (lib.PNGDEC_ST_* bits) = the decoder refused the file and its region of
    `out` holds nothing of use (the caller decodes it with Pillow).  The batch goes in chunks whose workspace of filtered scanlines
    stays below `workspace_bytes` (a chunk holds at least one file); one synchronisation, at the end."""
    return _c.decode_plans(_this, plans, files, out, offsets, channels, workspace_bytes)


def stage_chunk(plans, files, offsets, channels, dev) -> dict:
    """Everything one ``dm4d_png_decode_u8`` call reads, uploaded: the zlib streams (each on a multiple of 4 bytes), the descriptors,
    and the workspace and status tensors.  -> the dict ``launch_chunk`` takes; its "bytes_up" is what crossed PCIe."""
    import torch
    lib = _l.load()
    n = len(plans)
    desc = torch.zeros((n, _l.PNGDEC_FIELDS), dtype=torch.int64)
    streams = bytearray()
    ws0 = 0
    for k, p in enumerate(plans):
        s = p.stream_bytes(files[k])
        desc[k] = torch.tensor([len(streams), len(s), p.h, p.w, p.channels, int(offsets[k]), int(channels[k]), ws0])
        streams += s + bytes(-len(s) % 4)
        ws0 += p.workspace_need
    nbytes = int(lib.dm4d_png_decode_ws_bytes(ws0, n))
    if nbytes == 0 or not streams:
        raise _l.Dm4dError(f"decode_plans: {n} files with {ws0} filtered bytes are out of range for one call")
    streams_dev = torch.frombuffer(streams, dtype=torch.uint8).to(dev)
    desc_dev = desc.to(dev)
    ws = _c.workspace(nbytes, dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    return {"n": n, "streams": streams_dev, "desc": desc, "desc_dev": desc_dev, "ws": ws, "status": status,
            "bytes_up": len(streams) + desc.numel() * 8}


def launch_chunk(staged: dict, out):
    """The library call on the current stream -> the device int32 status tensor (not yet synchronised)."""
    from .ops import _p, _stream
    _l.call("dm4d_png_decode_u8", _stream(), _p(staged["streams"]), staged["streams"].numel(), staged["desc"].data_ptr(),
            _p(staged["desc_dev"]), staged["n"], _p(staged["ws"]), staged["ws"].numel() * 8, _p(out), out.numel(), _p(staged["status"]))
    return staged["status"]


def decode_png_batch(files, device="cuda", *, workspace_bytes: int = DEFAULT_WORKSPACE, stats: Optional[dict] = None) -> list:
    """Image files (paths or bytes) -> uint8 device tensors [h, w] (mode L) or [h, w, 3 / 4] (RGB / RGBA), what
    ``np.asarray(Image.open(f))`` gives.  PNG files of the supported set are decoded on the device; a file ``probe`` refuses, or one
    the decoder reports a nonzero status for, is decoded by Pillow and uploaded (and raises what Pillow raises).
    stats: if given, receives "device" and "pillow" = how many files took each route, "bytes_uploaded"."""
    return _c.decode_batch(_this, "decode_png_batch", files, device, workspace_bytes, stats)
