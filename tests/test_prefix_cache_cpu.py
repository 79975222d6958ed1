"""CPU: the bookkeeping of the per-sweep prefix cache (host/prefix_cache.py) on the window plans of the flagship workload -- the
spatial task (48 cameras, 4 inputs) and the temporal task (2 x 150 frames), alone and as a stack of two."""
import numpy as np
import pytest

from diffuman4d_amd.host.prefix_cache import PrefixBook
from diffuman4d_amd.host.schedule import plan_sweep


def plan_tables(domain: str, copies: int):
    if domain == "spatial":
        n, cond = 48, [i in (1, 13, 25, 37) for i in range(48)]
    else:
        n, cond = 300, [i < 150 for i in range(300)]
    plan = plan_sweep(cond, [0] * n, domain, 12, 2, 0, False, 1, 3)
    win, c = np.stack(plan.windows), np.stack(plan.is_cond)
    if copies > 1:  # what Diffuman4DPipeline.upload_plan does for a stack of tasks
        win = np.concatenate([win + k * n for k in range(copies)], axis=1)
        c = np.concatenate([c] * copies, axis=1)
    return win, c, n


def apply(t, book, F, cfg, cache):
    """Plays the call's row moves on sets of (task row, half): returns what every full-batch row ends up holding."""
    win = book.win[t.call]
    full = {}
    compact = {h * len(t.frames) + p: (int(win[f]), h, "computed") for h in range(cfg) for p, f in enumerate(t.frames)}
    if t.whole:
        full = {h * F + f: (int(win[f]), h, "computed") for h in range(cfg) for f in range(F)}
        assert t.scatter.src.size == 0 and not t.gathers
    else:
        assert sorted(t.scatter.src) == list(range(cfg * len(t.frames)))
        for s, d in zip(t.scatter.src, t.scatter.dst):
            assert int(d) not in full
            full[int(d)] = compact[int(s)]
    for m in t.gathers:
        for s, d in zip(m.src, m.dst):
            assert int(d) not in full and 0 <= s < book.chunk_slots
            row, h = cache[(m.chunk, int(s))]
            full[int(d)] = (row, h, "cached")
    stored = {}
    for m in t.stores:
        for s, d in zip(m.src, m.dst):
            row, h, _ = (full if t.whole else compact)[int(s)]
            assert (m.chunk, int(d)) not in cache and (m.chunk, int(d)) not in stored and 0 <= d < book.chunk_slots
            stored[(m.chunk, int(d))] = (row, h)
    cache.update(stored)
    return full


@pytest.mark.parametrize("domain,copies", [("spatial", 1), ("spatial", 2), ("temporal", 1), ("temporal", 2)])
def test_every_row_of_every_call_exactly_once_and_every_cond_row_computed_once(domain, copies):
    win, cond, n = plan_tables(domain, copies)
    assert win[0, :4].tolist() == [1, 13, 25, 37] if domain == "spatial" else cond[0, :12].all() and not cond[0, 12:24].any()
    cfg = 2
    book = PrefixBook(win, cond, cfg, chunk_slots=64)
    calls, F = win.shape
    cache, computed = {}, {}
    for i in range(calls):
        t = book.tables(i)
        full = apply(t, book, F, cfg, cache)
        # compact rows and cached rows together are the CFG batch, every row exactly once, each holding its own (task row, half)
        assert sorted(full) == list(range(cfg * F))
        for b, (row, h, how) in full.items():
            assert (row, h) == (int(win[i, b % F]), b // F)
            assert how == "computed" or cond[i, b % F]
        assert t.out_row.tolist() == [list(t.frames).index(f) if f in t.frames else -1 for f in range(F)]
        assert t.batch_rows.tolist() == [h * F + f for h in range(cfg) for f in t.frames]
        for f in t.frames:
            if cond[i, f]:
                computed[int(win[i, f])] = computed.get(int(win[i, f]), 0) + 1
        book.commit(t)
    cond_rows = set(int(r) for r in win[cond])
    assert computed == {r: 1 for r in cond_rows}
    assert len(book.slot_of) == book.total_slots() == cfg * len(cond_rows) == len(cache)
    assert book.chunks() == -(-book.total_slots() // 64)
    # a wrapped-around call index (bench.py: call_idx % calls): targets only, and the same tables object on every later visit
    for i in (0, 1, calls - 1):
        t = book.tables(i)
        assert not t.whole and not t.stores and t.frames.tolist() == [f for f in range(F) if not cond[i, f]]
        full = apply(t, book, F, cfg, cache)
        assert sorted(full) == list(range(cfg * F))
        book.commit(t)
        assert book.tables(i) is t


def test_reset_forgets_the_slots_and_the_memo():
    win, cond, _ = plan_tables("spatial", 1)
    book = PrefixBook(win, cond, 1, chunk_slots=3)
    first = book.tables(0)
    book.commit(first)
    assert first.whole and [m.chunk for m in first.stores] == [0, 1] and book.chunks() == 2  # 4 slots in chunks of 3
    assert not book.tables(1).whole and [m.chunk for m in book.tables(1).gathers] == [0, 1]
    book.reset()
    again = book.tables(0)
    assert again is not first and again.whole and not book.filled
    assert book.tables(1).whole  # nothing was committed
