"""A plain numpy / Python restatement of libjpeg's default decompression of a baseline JPEG file, as far as the device decoder
(csrc/jpegdec.hip) takes it: Huffman decoding of one interleaved scan, dequantisation, jidctint "islow", "fancy" chroma up-sampling and
the 16-bit fixed-point YCbCr -> RGB tables.  Integer arithmetic throughout: ``decode(data)`` is ``np.asarray(Image.open(file))``, and
it is held to Pillow on the CPU (tests/test_jpegdec_cpu.py).  The markers are read by ``diffuman4d_amd.host.jpegdec.probe``.

It also carries a plain-Python emulation of the device's entropy stage (``speculative_coefficients``): the scan is cut into
subsequences of SUB_BITS bits, TILE_LANES of them make a tile, every lane decodes its subsequence from a guessed state (bit position,
block slot in the MCU, zig-zag index) and rounds re-decode from the predecessor's exit state until nothing changes.  Its counters
say how many rounds a file needed and how many tiles it spans.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np

from diffuman4d_amd.host.jpeg import ZIGZAG
from diffuman4d_amd.host.jpegdec import Plan, probe

SUB_BITS = 1024    # DM4D_JPEGDEC_SUB_BITS
TILE_LANES = 256   # DM4D_JPEGDEC_TILE_LANES
ST_BAD_CODE, ST_ZIGZAG, ST_END, ST_RANGE = 1, 2, 4, 8  # DM4D_JPEGDEC_ST_*

CONST_BITS, PASS1_BITS = 13, 2
F_0_298, F_0_390, F_0_541, F_0_765, F_0_899, F_1_175 = 2446, 3196, 4433, 6270, 7373, 9633
F_1_501, F_1_847, F_1_961, F_2_053, F_2_562, F_3_072 = 12299, 15137, 16069, 16819, 20995, 25172


def _fix(x: float) -> int:
    return int(x * 65536 + 0.5)


# -- entropy decoding -------------------------------------------------------------------------------------------------------------------
def huff_lookup(bits, vals) -> list:
    """(BITS, HUFFVAL) -> a list over every 16-bit window: (length << 8) | symbol of the code it starts with, 0 = no such code."""
    lut = np.zeros(65536, dtype=np.int32)
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            lut[code << (16 - length):(code + 1) << (16 - length)] = (length << 8) | vals[k]
            code += 1
            k += 1
        code <<= 1
    return lut.tolist()


class Scan:
    """The unstuffed scan of a file with the lookup tables of its components."""

    def __init__(self, plan: Plan, data: bytes):
        self.plan = plan
        raw = plan.scan_bytes(data)
        self.nbytes = len(raw)
        self.total_bits = 8 * len(raw)
        self.buf = raw + bytes(8)  # bits beyond the scan read as zeros
        t = plan.tables
        self.dc, self.ac = [], []
        cache = {}
        for c in range(3):
            rec = t[304 * c:304 * (c + 1)]
            for kind, bits, vals in ((self.dc, rec[0:16], rec[16:32]), (self.ac, rec[32:48], rec[48:304])):
                key = (bytes(bits), bytes(vals))
                if key not in cache:
                    cache[key] = huff_lookup(bits, vals)
                kind.append(cache[key])
        self.comp = [0] if plan.ncomp == 1 else [0] * (plan.hs * plan.vs) + [1, 2]
        self.nb = len(self.comp)
        self.total_blocks = plan.blocks

    def run(self, state: Tuple[int, int, int], end: int, emit: Optional[np.ndarray] = None, block: int = 0):
        """Decode symbols from state = (bit position, block slot, zig-zag index; 0 = the DC symbol is next) while the position is
        below `end`.  -> (exit state, blocks completed, status, position at which the last block of the image ended or -1).
        With `emit` (int32 [blocks, 64], zig-zag order) the values are stored, `block` being the index of the block the state is in,
        and decoding stops once every block of the image is complete; without it nothing is stored and no block count ends it."""
        p, b, k = state
        buf, comp, nb, total = self.buf, self.comp, self.nb, self.total_blocks
        n = status = 0
        done_at = -1
        write = emit is not None
        while p < end:
            if write and block + n >= total:
                break
            at = p >> 3
            win = ((int.from_bytes(buf[at:at + 5], "big") >> (8 - (p & 7))) & 0xFFFFFFFF)
            c = comp[b]
            e = (self.dc[c] if k == 0 else self.ac[c])[win >> 16]
            if e == 0:
                length, sym = 16, 0  # a window no code starts: 16 bits are dropped
                status |= ST_BAD_CODE
            else:
                length, sym = e >> 8, e & 255
            if k == 0:
                s = sym & 15
                if s:
                    v = (win >> (32 - length - s)) & ((1 << s) - 1)
                    if write:
                        emit[block + n, 0] = v if v >= (1 << (s - 1)) else v - (1 << s) + 1
                p += length + s
                k = 1
            else:
                r, s = sym >> 4, sym & 15
                if s:
                    k += r
                    if k > 63:
                        status |= ST_ZIGZAG
                        k = 64
                    else:
                        v = (win >> (32 - length - s)) & ((1 << s) - 1)
                        if write:
                            emit[block + n, k] = v if v >= (1 << (s - 1)) else v - (1 << s) + 1
                        k += 1
                elif r == 15:
                    k += 16
                else:
                    k = 64  # EOB (libjpeg ends the block at any other run with size 0 too)
                p += length + s
                if k >= 64:
                    k = 0
                    b = b + 1 if b + 1 < nb else 0
                    n += 1
                    if block + n == total:
                        done_at = p
        return (p, b, k), n, (status if write else 0), done_at

    def finish(self, coef: np.ndarray, status: int, done_at: int) -> Tuple[np.ndarray, int]:
        """DC differences -> DC values per component (truncated to int16 like libjpeg's JCOEF), and the end-of-scan rule."""
        if done_at < 0 or (done_at + 7) >> 3 != self.nbytes:
            status |= ST_END
        blocks = coef.reshape(-1, self.nb, 64)
        for c in range(max(self.comp) + 1):
            slots = [i for i, cc in enumerate(self.comp) if cc == c]
            dc = blocks[:, slots, 0]
            blocks[:, slots, 0] = np.cumsum(dc.reshape(-1), dtype=np.int64).reshape(dc.shape).astype(np.int16)
        return blocks.reshape(-1, 64).astype(np.int16), status


def serial_coefficients(plan: Plan, data: bytes) -> Tuple[np.ndarray, int]:
    """-> (int16 [blocks, 64] in zig-zag order, blocks in scan order; status)."""
    sc = Scan(plan, data)
    coef = np.zeros((sc.total_blocks, 64), dtype=np.int32)
    _, _, status, done_at = sc.run((0, 0, 0), sc.total_bits, coef, 0)
    return sc.finish(coef, status, done_at)


def speculative_coefficients(plan: Plan, data: bytes, sub_bits: int = SUB_BITS, lanes: int = TILE_LANES,
                             counters: Optional[Dict[str, int]] = None) -> Tuple[np.ndarray, int]:
    """The same result by the device's scheme.  counters: "tiles" = tiles of the scan, "rounds" = the most propagation rounds any tile
    needed AFTER the first pass in which a lane's state changed, "passes" = decoded subsequences in all."""
    sc = Scan(plan, data)
    coef = np.zeros((sc.total_blocks, 64), dtype=np.int32)
    carried, carried_blocks = (0, 0, 0), 0
    status, done_at = 0, -1
    tiles = max_rounds = passes = 0
    tile_bits = sub_bits * lanes
    for t0 in range(0, sc.total_bits, tile_bits):
        tiles += 1
        starts = [t0 + i * sub_bits for i in range(lanes)]
        live = [s < sc.total_bits for s in starts]
        ends = [min(s + sub_bits, sc.total_bits) for s in starts]
        entry = [carried if i == 0 else (starts[i], 0, 0) for i in range(lanes)]
        exits, counts = list(entry), [0] * lanes
        for i in range(lanes):  # the first pass: every lane from its guess
            if live[i]:
                exits[i], counts[i], _, _ = sc.run(entry[i], ends[i])
                passes += 1
        rounds = 0
        for _ in range(lanes):  # a round fixes at least one more lane: never more than `lanes` of them
            new_entry = [carried if i == 0 else exits[i - 1] for i in range(lanes)]
            changed = False
            for i in range(lanes):  # lanes beyond the scan take no part
                if live[i] and new_entry[i] != entry[i]:
                    entry[i] = new_entry[i]
                    changed = True
                    exits[i], counts[i], _, _ = sc.run(entry[i], ends[i])
                    passes += 1
            if not changed:
                break
            rounds += 1
        max_rounds = max(max_rounds, rounds)
        block = carried_blocks
        for i in range(lanes):  # the write pass
            if live[i]:
                ex, n, st, da = sc.run(entry[i], ends[i], coef, block)
                status |= st
                done_at = da if da >= 0 else done_at
            block += counts[i]
        carried, carried_blocks = exits[sum(live) - 1], block
    if counters is not None:
        counters["tiles"] = max(counters.get("tiles", 0), tiles)
        counters["rounds"] = max(counters.get("rounds", 0), max_rounds)
        counters["passes"] = counters.get("passes", 0) + passes
    return sc.finish(coef, status, done_at)


# -- dequantisation and inverse DCT -----------------------------------------------------------------------------------------------------
def _idct_sums(d):
    """jidctint.c jpeg_idct_islow, one pass over the last axis of d [..., 8] (Python / int64 integers): the eight sums before the
    descale."""
    z2, z3 = d[..., 2], d[..., 6]
    z1 = (z2 + z3) * F_0_541
    tmp2 = z1 - z3 * F_1_847
    tmp3 = z1 + z2 * F_0_765
    tmp0 = (d[..., 0] + d[..., 4]) * (1 << CONST_BITS)
    tmp1 = (d[..., 0] - d[..., 4]) * (1 << CONST_BITS)
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = d[..., 7], d[..., 5], d[..., 3], d[..., 1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * F_1_175
    tmp0, tmp1, tmp2, tmp3 = tmp0 * F_0_298, tmp1 * F_2_053, tmp2 * F_3_072, tmp3 * F_1_501
    z1, z2, z3, z4 = -z1 * F_0_899, -z2 * F_2_562, -z3 * F_1_961 + z5, -z4 * F_0_390 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    return [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]


def _idct_1d(d, shift: int):
    """... descaled by `shift` with rounding."""
    half = 1 << (shift - 1)
    return [(o + half) >> shift for o in _idct_sums(d)]


def range_limit(v):
    """libjpeg's IDCT range-limit table on v & 1023."""
    v = v & 1023
    return np.where(v < 128, v + 128, np.where(v < 512, 255, np.where(v < 896, 0, v - 896)))


def idct_islow(deq: np.ndarray) -> np.ndarray:
    """deq int64 [..., 8, 8] dequantised coefficients (natural order) -> uint8 samples: columns first (descale 11), then rows (18)."""
    cols = np.stack(_idct_1d(np.swapaxes(deq, -1, -2), CONST_BITS - PASS1_BITS), axis=-1)  # [..., col, row]
    ws = np.swapaxes(cols, -1, -2)
    rows = np.stack(_idct_1d(ws, CONST_BITS + PASS1_BITS + 3), axis=-1)
    return range_limit(rows).astype(np.uint8)


# -- planes, up-sampling, colour ---------------------------------------------------------------------------------------------------------
def component_planes(plan: Plan, coef: np.ndarray) -> Tuple[list, int]:
    """coef int16 [blocks, 64] zig-zag -> ([plane uint8 per component, cut to its down-sampled size], ST_RANGE or 0)."""
    nat = np.zeros((coef.shape[0], 64), dtype=np.int64)
    nat[:, ZIGZAG] = coef
    hs, vs, nc = plan.hs, plan.vs, plan.ncomp
    nb = 1 if nc == 1 else hs * vs + 2
    my, mx = (plan.h + 8 * vs - 1) // (8 * vs), (plan.w + 8 * hs - 1) // (8 * hs)
    nat = nat.reshape(my, mx, nb, 8, 8)
    q = np.frombuffer(plan.tables, dtype=np.uint8)[912:].astype(np.int64).reshape(3, 8, 8)
    planes, status = [], 0
    for c in range(nc):
        ch, cv = (hs, vs) if c == 0 else (1, 1)
        first = 0 if c == 0 else hs * vs + c - 1
        deq = nat[:, :, first:first + ch * cv] * q[c]
        if deq.min() < -8192 or deq.max() > 8191:
            status = ST_RANGE
        px = idct_islow(deq).reshape(my, mx, cv, ch, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(my * cv * 8, mx * ch * 8)
        dh, dw = -(-plan.h * cv // vs), -(-plan.w * ch // hs)
        planes.append(px[:dh, :dw])
    return planes, status


def upsample(p: np.ndarray, fx: int, fy: int, h: int, w: int) -> np.ndarray:
    """jdsample.c: a plane down-sampled by (fx, fy) in {(1, 1), (2, 1), (2, 2)} -> [h, w]."""
    if fx == 1 and fy == 1:
        return p[:h, :w]
    dh, dw = p.shape
    if dw <= 2:  # too narrow for the triangle filter: replication in both directions
        return np.repeat(np.repeat(p, fy, axis=0), fx, axis=1)[:h, :w]
    p = p.astype(np.int64)
    if fy == 2:
        up, down = p[np.maximum(np.arange(dh) - 1, 0)], p[np.minimum(np.arange(dh) + 1, dh - 1)]
        cs = np.empty((2 * dh, dw), dtype=np.int64)
        cs[0::2], cs[1::2] = 3 * p + up, 3 * p + down
        left, right = np.roll(cs, 1, axis=1), np.roll(cs, -1, axis=1)
        even, odd = (3 * cs + left + 8) >> 4, (3 * cs + right + 7) >> 4
        even[:, 0], odd[:, -1] = (4 * cs[:, 0] + 8) >> 4, (4 * cs[:, -1] + 7) >> 4
    else:
        left, right = np.roll(p, 1, axis=1), np.roll(p, -1, axis=1)
        even, odd = (3 * p + left + 1) >> 2, (3 * p + right + 2) >> 2
        even[:, 0], odd[:, -1] = p[:, 0], p[:, -1]
    out = np.empty((even.shape[0], 2 * dw), dtype=np.int64)
    out[:, 0::2], out[:, 1::2] = even, odd
    return out[:h, :w].astype(np.uint8)


def ycc_to_rgb(y: np.ndarray, cb: np.ndarray, cr: np.ndarray) -> np.ndarray:
    y, cb, cr = y.astype(np.int64), cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    r = y + ((_fix(1.40200) * cr + 32768) >> 16)
    b = y + ((_fix(1.77200) * cb + 32768) >> 16)
    g = y + ((-_fix(0.34414) * cb + 32768 - _fix(0.71414) * cr) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def pixels(plan: Plan, coef: np.ndarray) -> Tuple[np.ndarray, int]:
    planes, status = component_planes(plan, coef)
    if plan.ncomp == 1:
        return planes[0], status
    cb, cr = (upsample(p, plan.hs, plan.vs, plan.h, plan.w) for p in planes[1:])
    return ycc_to_rgb(planes[0], cb, cr), status


def decode_status(data: bytes) -> Tuple[np.ndarray, int]:
    """-> (uint8 [h, w, 3] or [h, w], status word: nonzero = the device refuses the file and its pixels are unspecified)."""
    plan = probe(data)
    if plan is None:
        raise ValueError("not a file of the supported set")
    coef, st = serial_coefficients(plan, data)
    out, st2 = pixels(plan, coef)
    return out, st | st2


def decode(data: bytes) -> np.ndarray:
    return decode_status(data)[0]
