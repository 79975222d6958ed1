"""Baseline JPEG files decoded on the device, byte for byte what ``np.asarray(Image.open(file))`` of Pillow / libjpeg gives.

``probe`` reads a file's markers on the host and says whether the device decoder takes it (one interleaved Huffman scan, 8 bits, no
restart markers, grayscale or YCbCr at 4:4:4 / 4:2:2 / 4:2:0); every other file keeps its Pillow route.  ``decode_plans`` uploads the
entropy-coded segments (their ``FF 00`` stuffing removed with one ``bytes.replace``), the raw BITS / HUFFVAL and quantisation tables, and
has csrc/jpegdec.hip decode the batch into a caller-given device buffer at caller-given offsets (``dm4d_jpeg_decode_u8``): one workgroup
per image finds the symbol boundaries of the scan by speculative decoding and writes int16 coefficients, a second launch dequantises,
inverts the DCT (jidctint "islow"), up-samples the chroma ("fancy" triangle filter) and converts to RGB.  ``decode_jpeg_batch`` is the
list-in, tensors-out form.  What is specific to JPEG is here (``probe``, ``Plan``, ``stage_chunk``, ``launch_chunk``); the chunked
driver behind ``decode_plans``, the body of ``decode_jpeg_batch`` and the Pillow route are host/codec.py's, shared with host/pngdec.py.
DESIGN.md "Device JPEG decode" has the definition; tests/jpegdec_model.py is the same in numpy.  There is no CPU path: a non-HIP
device is an error.
"""
from __future__ import annotations

import re
import struct
import sys
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

from . import codec as _c
from . import lib as _l
from .jpeg import ZIGZAG

_this = sys.modules[__name__]  # the codec of host/codec.py's bodies: its attributes are looked up when they are called

DEFAULT_WORKSPACE = 1 << 30
MAX_SCAN_BYTES = 1 << 28  # bit positions of a scan are 32-bit on the device

_MARKER = re.compile(rb"\xff[^\x00]", re.S)
_STANDALONE = frozenset([0x01, *range(0xD0, 0xD8)])


@dataclass(frozen=True)
class Plan:
    """What the device needs of one supported file: the size, the layout of an MCU, the tables and where the scan lies."""
    h: int
    w: int
    ncomp: int          # 1 (mode "L") or 3 (mode "RGB")
    hs: int             # luma sampling factors: (2, 2) = 4:2:0, (2, 1) = 4:2:2, (1, 1) = 4:4:4 or grayscale
    vs: int
    tables: bytes       # lib.JPEGDEC_TABLE_BYTES: per component DC bits, DC values, AC bits, AC values; then 3 x 64 quantisers, natural order
    scan: Tuple[int, int]  # [start, end) of the entropy-coded segment in the file

    @property
    def mode(self) -> str:
        return "L" if self.ncomp == 1 else "RGB"

    @property
    def mcus(self) -> int:
        return ((self.h + 8 * self.vs - 1) // (8 * self.vs)) * ((self.w + 8 * self.hs - 1) // (8 * self.hs))

    @property
    def blocks(self) -> int:
        """int16 [64] coefficient blocks of the whole scan, dummy blocks of edge MCUs included"""
        return self.mcus * (1 if self.ncomp == 1 else self.hs * self.vs + 2)

    # what host/codec.py asks of a plan
    @property
    def bytes_per_pixel(self) -> int:
        return self.ncomp

    @property
    def workspace_need(self) -> int:
        """bytes of the coefficient workspace"""
        return self.blocks * 128

    @property
    def payload_len(self) -> int:
        """bytes of the file that go up: the scan as it lies in the file"""
        return self.scan[1] - self.scan[0]

    def scan_bytes(self, data: bytes) -> bytes:
        """The entropy-coded segment without its byte stuffing."""
        return bytes(data[self.scan[0]:self.scan[1]]).replace(b"\xff\x00", b"\xff")


def huffman_ok(bits: Sequence[int], nvals: int, dc: bool, vals: Sequence[int]) -> bool:
    """libjpeg's jpeg_make_d_derived_tbl accepts the table: the counts match, no code overflows its length, DC categories <= 15."""
    if sum(bits) != nvals or nvals > (16 if dc else 256):
        return False
    code = 0
    for length in range(1, 17):
        code += bits[length - 1]
        if code > (1 << length):
            return False
        code <<= 1
    return not dc or all(v <= 15 for v in vals)


def probe(data) -> Optional[Plan]:
    """The plan of a file the device decoder takes, or None (the file keeps its Pillow route).  Host only; nothing is decoded."""
    data = bytes(data)
    n = len(data)
    if n < 4 or data[:2] != b"\xff\xd8":
        return None
    pos = 2
    quant, huff = {}, {}
    frame = None
    jfif = False
    adobe = None
    while True:
        # a marker: any number of FF fill bytes, then the code
        if pos >= n or data[pos] != 0xFF:
            return None
        while pos < n and data[pos] == 0xFF:
            pos += 1
        if pos >= n:
            return None
        m = data[pos]
        pos += 1
        if m in _STANDALONE:
            return None  # a restart marker or TEM before the scan: not ours
        if m in (0xD8, 0xD9) or pos + 2 > n:
            return None
        length = struct.unpack_from(">H", data, pos)[0]
        if length < 2 or pos + length > n:
            return None
        seg = data[pos + 2:pos + length]
        pos += length
        if m == 0xDB:
            i = 0
            while i < len(seg):
                pq, tq = seg[i] >> 4, seg[i] & 15
                if pq != 0 or tq > 3 or i + 65 > len(seg):
                    return None
                quant[tq] = seg[i + 1:i + 65]
                i += 65
        elif m == 0xC4:
            i = 0
            while i < len(seg):
                if i + 17 > len(seg):
                    return None
                tc, th = seg[i] >> 4, seg[i] & 15
                bits = seg[i + 1:i + 17]
                cnt = sum(bits)
                if tc > 1 or th > 3 or i + 17 + cnt > len(seg):
                    return None
                vals = seg[i + 17:i + 17 + cnt]
                if not huffman_ok(bits, cnt, tc == 0, vals):
                    return None
                huff[(tc, th)] = (bits, vals)
                i += 17 + cnt
        elif m == 0xC0:
            if frame is not None or len(seg) < 6:
                return None
            prec, h, w, nc = struct.unpack_from(">BHHB", seg)
            if prec != 8 or h < 1 or w < 1 or nc not in (1, 3) or len(seg) != 6 + 3 * nc:
                return None
            frame = (h, w, [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(nc)])
        elif 0xC1 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            return None  # extended, progressive, lossless, arithmetic
        elif m == 0xCC:
            return None
        elif m == 0xDD:
            if len(seg) != 2 or seg != b"\0\0":
                return None
        elif m == 0xE0:
            if len(seg) >= 14 and seg[:5] == b"JFIF\0":
                jfif = True
        elif m == 0xEE:
            if len(seg) >= 12 and seg[:5] == b"Adobe":
                adobe = seg[11]
        elif m == 0xDA:
            break
    if frame is None:
        return None
    h, w, comps = frame
    nc = len(comps)
    if len(seg) != 4 + 2 * nc or seg[0] != nc or tuple(seg[1 + 2 * nc:]) != (0, 63, 0):
        return None
    if nc == 1:
        if comps[0][1:3] != (1, 1):
            return None
        hs = vs = 1
    else:
        hs, vs = comps[0][1], comps[0][2]
        if (hs, vs) not in ((2, 2), (2, 1), (1, 1)) or comps[1][1:3] != (1, 1) or comps[2][1:3] != (1, 1):
            return None
        ids = tuple(c[0] for c in comps)
        if len(set(ids)) != 3:
            return None
        # libjpeg's guess of the colour space (jdapimin.c): only YCbCr is ours
        if not jfif:
            if adobe is not None:
                if adobe != 1:
                    return None
            elif ids != (1, 2, 3):
                return None
    rec = bytearray()
    qrec = bytearray()
    for c in range(3):
        cid, _, _, tq = comps[min(c, nc - 1)]
        k = min(c, nc - 1)
        if seg[1 + 2 * k] != cid:
            return None  # the scan lists the components in frame order
        td, ta = seg[2 + 2 * k] >> 4, seg[2 + 2 * k] & 15
        if tq not in quant or (0, td) not in huff or (1, ta) not in huff:
            return None
        for bits, vals, room in ((*huff[(0, td)], 16), (*huff[(1, ta)], 256)):
            rec += bytes(bits) + bytes(vals) + bytes(room - len(vals))
        q = bytearray(64)
        for z in range(64):
            q[ZIGZAG[z]] = quant[tq][z]
        qrec += q
    # the entropy-coded segment runs to the next marker, which must be EOI (RSTn: restart intervals; anything else: more scans)
    end = _MARKER.search(data, pos)
    if end is None or data[end.start() + 1] != 0xD9 or not 0 < end.start() - pos < MAX_SCAN_BYTES:
        return None
    return Plan(h, w, nc, hs, vs, bytes(rec + qrec), (pos, end.start()))


def decode_plans(plans: Sequence[Plan], files: Sequence[bytes], out, offsets: Sequence[int], channels: Sequence[int],
                 workspace_bytes: int = DEFAULT_WORKSPACE) -> List[int]:
    """Decode files[k] (whose plan is plans[k]) into the uint8 device tensor `out` at byte offsets[k], rows tight, channels[k] bytes a
    pixel (3, or 1 for a grayscale file).  -> the status words: nonzero = the decoder refused the file and its region of `out` holds
    nothing of use (the caller decodes it with Pillow).  The batch goes in chunks whose coefficient workspace stays below
    `workspace_bytes` (a chunk holds at least one file); one synchronisation, at the end."""
    return _c.decode_plans(_this, plans, files, out, offsets, channels, workspace_bytes)


def stage_chunk(plans, files, offsets, channels, dev) -> dict:
    """Everything one ``dm4d_jpeg_decode_u8`` call reads, uploaded: the unstuffed scans (each on a multiple of 4 bytes), descriptors,
    tables, and the workspace and status tensors.  -> the dict ``launch_chunk`` takes; its "bytes_up" is what crossed PCIe."""
    import torch
    lib = _l.load()
    n = len(plans)
    desc = torch.zeros((n, _l.JPEGDEC_FIELDS), dtype=torch.int64)
    scans = bytearray()
    block0 = 0
    for k, p in enumerate(plans):
        s = p.scan_bytes(files[k])
        desc[k, :10] = torch.tensor([len(scans), len(s), p.h, p.w, p.ncomp, p.hs, p.vs, int(offsets[k]), int(channels[k]), block0])
        scans += s + bytes(-len(s) % 4)
        block0 += p.blocks
    nbytes = int(lib.dm4d_jpeg_decode_ws_bytes(block0, n))
    if nbytes == 0 or not scans:
        raise _l.Dm4dError(f"decode_plans: {n} files with {block0} blocks are out of range for one call")
    tab = torch.frombuffer(bytearray(b"".join(p.tables for p in plans)), dtype=torch.uint8)
    scans_dev = torch.frombuffer(scans, dtype=torch.uint8).to(dev)
    desc_dev, tab_dev = desc.to(dev), tab.to(dev)
    ws = _c.workspace(nbytes, dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    return {"n": n, "scans": scans_dev, "desc": desc, "desc_dev": desc_dev, "tab": tab, "tab_dev": tab_dev, "ws": ws, "status": status,
            "bytes_up": len(scans) + desc.numel() * 8 + tab.numel()}


def launch_chunk(staged: dict, out):
    """The library call on the current stream -> the device int32 status tensor (not yet synchronised)."""
    from .ops import _p, _stream
    _l.call("dm4d_jpeg_decode_u8", _stream(), _p(staged["scans"]), staged["scans"].numel(), staged["desc"].data_ptr(), _p(staged["desc_dev"]),
            staged["n"], staged["tab"].data_ptr(), _p(staged["tab_dev"]), _p(staged["ws"]), staged["ws"].numel() * 8, _p(out), out.numel(),
            _p(staged["status"]))
    return staged["status"]


def decode_jpeg_batch(files, device="cuda", *, workspace_bytes: int = DEFAULT_WORKSPACE, stats: Optional[dict] = None) -> list:
    """Image files (paths or bytes) -> uint8 device tensors [h, w, 3] (mode RGB) or [h, w] (mode L), what
    ``np.asarray(Image.open(f))`` gives.  Baseline JPEG files of the supported set are decoded on the device; a file ``probe`` refuses,
    or one the decoder reports a nonzero status for, is decoded by Pillow and uploaded (and raises what Pillow raises).
    stats: if given, receives "device" and "pillow" = how many files took each route, "bytes_uploaded"."""
    return _c.decode_batch(_this, "decode_jpeg_batch", files, device, workspace_bytes, stats)
