"""The device cell cache of ``SpaTemDataset(device_cache=True)``: bookkeeping only, nothing here launches a kernel.

A *cell* is one resized frame as ``dm4d_capture_crop_resize_packed_u8`` leaves it: ``H * W`` packed pixels of 8 bytes ``{i0 i1 i2 m
s0 s1 s2 0}`` (include/dm4d.h).  Cells live in *slabs*, ``torch.uint8`` tensors of ``slab_cells`` cells each that are allocated on
demand while their total stays within ``budget_bytes``.  There is no eviction: a job's access pattern is known and its grid fits or
the budget says how much of it is kept; a cell that the budget does not cover is simply not retained (the dataset then packs it into a
temporary slab of its own and loads it again the next time).  Dropping cells in mid-job would need a completion event per reader.

Per key the state is absent | pending | ready.  ``claim(keys)`` is atomic under one lock and sorts the keys into the ready hits, the
keys the caller now owns (marked pending) and the keys another caller holds pending.  The protocol of a caller:

  1. load what it owns (``reserve`` names the cells to write into),
  2. ``publish`` every cell, or ``abandon`` the keys (an error, or a cell the budget did not cover),
  3. only then ``wait`` for the keys of others, and ``claim`` them again: a key its owner abandoned comes back as absent.

No caller waits while it still owes cells, so there is no cycle of waiters.  A ready cell carries the host metadata of its frame (the
crop box) and the ``torch.cuda.Event`` recorded after the launch that wrote it (``None`` on a CPU device, where the unit tests run)."""
from __future__ import annotations

import threading
from typing import Any, Dict, Hashable, List, NamedTuple, Optional, Sequence, Tuple

import torch

_PENDING = object()


class Cell(NamedTuple):
    key: Hashable
    slab: torch.Tensor  # the uint8 tensor the cell lies in
    offset: int         # its byte offset there, a multiple of 16
    meta: Any           # what the sample needs of the frame besides pixels: its crop box
    event: Any          # recorded after the pack launch that wrote the cell; None on a CPU device


class CellCache:
    def __init__(self, device, cell_bytes: int, budget_bytes: int, slab_cells: int = 64):
        if cell_bytes < 16 or cell_bytes % 16 or slab_cells < 1 or budget_bytes < 0:
            raise ValueError(f"CellCache: cell_bytes must be a positive multiple of 16, slab_cells >= 1 and budget_bytes >= 0 "
                             f"(got {cell_bytes}, {slab_cells}, {budget_bytes})")
        self.device, self.cell_bytes, self.budget_bytes, self.slab_cells = torch.device(device), int(cell_bytes), int(budget_bytes), int(slab_cells)
        self._cond = threading.Condition(threading.Lock())
        self._state: Dict[Hashable, Any] = {}                      # key -> _PENDING | Cell; absent keys are not in it
        self._reserved: Dict[Hashable, Tuple[int, int]] = {}       # pending key -> (slab index, offset) it will be published in
        self._slabs: List[torch.Tensor] = []
        self._free: List[Tuple[int, int]] = []                     # (slab index, offset) of cells without a key, last in first out
        self._counts = {"hits": 0, "misses": 0, "unretained": 0}

    # -- the claim protocol ---------------------------------------------------------------------------------------------------------
    def claim(self, keys: Sequence[Hashable]) -> Tuple[List[Cell], List[Hashable], List[Hashable]]:
        """-> (the ready cells, the keys the caller owns from now on, the keys another caller holds pending), each in the order of `keys`."""
        hits, owned, others = [], [], []
        with self._cond:
            for k in dict.fromkeys(keys):
                st = self._state.get(k)
                if st is None:
                    self._state[k] = _PENDING
                    owned.append(k)
                elif st is _PENDING:
                    others.append(k)
                else:
                    hits.append(st)
            self._counts["hits"] += len(hits)
            self._counts["misses"] += len(owned)
        return hits, owned, others

    def reserve(self, keys: Sequence[Hashable]) -> List[Optional[Tuple[torch.Tensor, int]]]:
        """Where the caller writes the cells of keys it owns -> per key (slab, byte offset), or None for a cell that the budget does
        not cover: it is not retained, the caller abandons its key after use."""
        out = []
        with self._cond:
            for k in keys:
                if self._state.get(k) is not _PENDING or k in self._reserved:
                    raise RuntimeError(f"CellCache.reserve: {k!r} is not a key its caller claimed")
                if not self._free and (len(self._slabs) + 1) * self.slab_cells * self.cell_bytes <= self.budget_bytes:
                    self._slabs.append(torch.empty(self.slab_cells * self.cell_bytes, dtype=torch.uint8, device=self.device))
                    i = len(self._slabs) - 1
                    self._free.extend((i, c * self.cell_bytes) for c in reversed(range(self.slab_cells)))
                if not self._free:
                    self._counts["unretained"] += 1
                    out.append(None)
                    continue
                self._reserved[k] = slot = self._free.pop()
                out.append((self._slabs[slot[0]], slot[1]))
        return out

    def publish(self, key: Hashable, meta: Any, event: Any = None) -> None:
        """The reserved cell of `key` is written (or will be, once `event` completes): pending -> ready."""
        with self._cond:
            if self._state.get(key) is not _PENDING or key not in self._reserved:
                raise RuntimeError(f"CellCache.publish: {key!r} has no reserved cell")
            i, off = self._reserved.pop(key)
            self._state[key] = Cell(key, self._slabs[i], off, meta, event)
            self._cond.notify_all()

    def abandon(self, keys: Sequence[Hashable]) -> None:
        """Pending keys of the caller -> absent; their reserved cells are free again.  Keys in any other state are left alone."""
        with self._cond:
            for k in keys:
                if self._state.get(k) is _PENDING:
                    del self._state[k]
                    slot = self._reserved.pop(k, None)
                    if slot is not None:
                        self._free.append(slot)
            self._cond.notify_all()

    def wait(self, keys: Sequence[Hashable]) -> None:
        """Block until none of `keys` is pending.  Only for a caller that owes nothing: every key it owned is published or abandoned."""
        with self._cond:
            self._cond.wait_for(lambda: all(self._state.get(k) is not _PENDING for k in keys))

    # -- the rest -------------------------------------------------------------------------------------------------------------------
    def state(self, key: Hashable) -> str:
        with self._cond:
            st = self._state.get(key)
        return "absent" if st is None else "pending" if st is _PENDING else "ready"

    def clear(self) -> None:
        """Drop every cell and slab.  The device is synchronised first: a launch that reads a cell may still be queued.  Not while a
        key is pending (a load in flight would publish into a slab that is gone)."""
        with self._cond:
            if any(st is _PENDING for st in self._state.values()):
                raise RuntimeError("CellCache.clear: keys are pending; clear between jobs, not during a load")
            if self.device.type == "cuda":
                torch.cuda.synchronize(self.device)
            self._state.clear()
            self._slabs.clear()
            self._free.clear()

    @property
    def stats(self) -> Dict[str, int]:
        with self._cond:
            cells = sum(1 for st in self._state.values() if st is not _PENDING)
            return dict(self._counts, cells=cells, bytes=sum(s.numel() for s in self._slabs))
