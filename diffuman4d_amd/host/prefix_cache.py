"""Bookkeeping of the per-sweep prefix cache (Diffuman4DPipeline.window_call): which rows of a window call's CFG batch run the UNet's
per-frame head, which are copied from the cache, and where a row's tensors live.  Host-only numpy; nothing here touches the device.

The UNet layers in front of the first 3-D transformer are strictly per frame, a conditioning frame's timestep is 0 and its packed
input is made of task tensors that do not change during a sweep -- so what those layers give for a conditioning frame is the same in
every window call of the sweep.  A SLOT holds that result (one row of each head tensor) for one (task row, CFG half) pair.  Slots are
numbered in the order their rows are first computed and live in chunks of `chunk_slots`, so that memory grows with the windows a sweep
has actually visited."""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Tuple

import numpy as np


class MoveRows(NamedTuple):
    """Rows of one copy job: row dst[k] of the destination takes row src[k] of the source; `chunk` names the cache chunk on the cache's
    side of the job (-1: none)."""
    chunk: int
    src: np.ndarray  # int32
    dst: np.ndarray  # int32


class CallTables(NamedTuple):
    """One window call, F frames and `cfg` halves: full-batch row = half * F + frame, compact row = half * len(frames) + position."""
    call: int
    frames: np.ndarray        # int32 [n]: window-local frames that run the head, ascending
    out_row: np.ndarray       # int32 [F]: position of a frame in `frames`, -1 = not computed (ops.pack_model_input out_row)
    batch_rows: np.ndarray    # int64 [cfg * n]: full-batch row of every compact row (selects the compact rows of per-row inputs)
    whole: bool               # every frame is computed: the head runs on the full batch, nothing is scattered or gathered
    scatter: MoveRows         # compact -> full batch (empty when `whole`)
    stores: Tuple[MoveRows, ...]   # compact (or, when `whole`, full batch) -> cache chunk, newly computed conditioning rows
    gathers: Tuple[MoveRows, ...]  # cache chunk -> full batch
    new_rows: Tuple[int, ...]      # task rows whose slots the stores fill


_I32 = np.int32


def _i32(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=_I32).reshape(-1))


class PrefixBook:
    """win [calls, F] task rows and cond [calls, F] conditioning flags of a sweep's window calls (the tables of upload_plan, stacked
    tasks included), cfg = CFG halves of a call's batch."""

    def __init__(self, win: np.ndarray, cond: np.ndarray, cfg: int, chunk_slots: int = 64):
        self.win, self.cond, self.cfg, self.chunk_slots = np.asarray(win), np.asarray(cond).astype(bool), int(cfg), int(chunk_slots)
        assert self.win.shape == self.cond.shape and self.win.ndim == 2 and self.cfg in (1, 2) and self.chunk_slots >= 1
        self.calls, self.F = self.win.shape
        self.reset()

    def reset(self) -> None:
        """Forget every slot (the task tensors changed)."""
        self.slot_of: Dict[Tuple[int, int], int] = {}  # (task row, half) -> slot, assigned when the row's store is planned
        self.filled = set()                            # task rows whose stores have been enqueued
        self._memo: Dict[Tuple[int, frozenset], CallTables] = {}

    def total_slots(self) -> int:
        """Slots of a sweep that visits every call: distinct conditioning rows x halves."""
        return int(np.unique(self.win[self.cond]).size) * self.cfg

    def chunks(self) -> int:
        return -(-len(self.slot_of) // self.chunk_slots)

    def _slot(self, row: int, half: int) -> int:
        return self.slot_of.setdefault((row, half), len(self.slot_of))

    def tables(self, i: int) -> CallTables:
        """The tables of call i given what is cached now; memoised per (call, frames still to compute)."""
        win, cond, F, cfg = self.win[i], self.cond[i], self.F, self.cfg
        frames = [f for f in range(F) if not cond[f] or int(win[f]) not in self.filled]
        key = (int(i), frozenset(frames))
        hit = self._memo.get(key)
        if hit is not None:
            return hit
        n = len(frames)
        out_row = np.full(F, -1, dtype=_I32)
        out_row[frames] = np.arange(n, dtype=_I32)
        batch_rows = np.concatenate([np.asarray(frames, dtype=np.int64) + h * F for h in range(cfg)])
        whole = n == F
        scatter = MoveRows(-1, _i32([]), _i32([])) if whole else MoveRows(-1, _i32(np.arange(cfg * n)), _i32(batch_rows))
        # newly computed conditioning frames: a task row that sits in the window twice is stored once
        new, seen = [], set()
        for p, f in enumerate(frames):
            if cond[f] and int(win[f]) not in seen:
                seen.add(int(win[f]))
                new.append((p, f))
        per_chunk: Dict[int, List[Tuple[int, int]]] = {}
        for p, f in new:
            for h in range(cfg):
                s = self._slot(int(win[f]), h)
                src = (h * F + f) if whole else (h * n + p)
                per_chunk.setdefault(s // self.chunk_slots, []).append((src, s % self.chunk_slots))
        stores = tuple(MoveRows(c, _i32([a for a, _ in v]), _i32([b for _, b in v])) for c, v in sorted(per_chunk.items()))
        per_chunk = {}
        for f in range(F):
            if out_row[f] < 0:
                for h in range(cfg):
                    s = self.slot_of[(int(win[f]), h)]
                    per_chunk.setdefault(s // self.chunk_slots, []).append((s % self.chunk_slots, h * F + f))
        gathers = tuple(MoveRows(c, _i32([a for a, _ in v]), _i32([b for _, b in v])) for c, v in sorted(per_chunk.items()))
        t = CallTables(int(i), _i32(frames), out_row, batch_rows, whole, scatter, stores, gathers, tuple(int(win[f]) for _, f in new))
        self._memo[key] = t
        return t

    def commit(self, t: CallTables) -> None:
        """The stores of `t` have been enqueued: its new rows count as cached from the next call on."""
        self.filled.update(t.new_rows)
