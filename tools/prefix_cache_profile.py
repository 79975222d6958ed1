#!/usr/bin/env python
"""Per-window-call time of the UNet's per-frame head in a rocprofv3 --kernel-trace database of tools/profile_bench.sh's bench command
(--task-streams 1: one stack at a time, launches in stream order).
usage: python tools/prefix_cache_profile.py <results.db> <title> > profiles/<name>.log

A window call starts at its pack_kernel launch.  Inside it the head is every launch from conv_in (the launch after the time embedding's
three GEMMs, silu_kernel + 2; with the prefix cache the time embedding precedes the pack launch and conv_in follows it) up to
  - the launch before rows_move_kernel, where the call has one (the prefix cache is on), else
  - the last convolution before the call's THIRD attention launch (the two level-0 transformers are per frame; the third attention is the
    first 3-D one, and the launch that feeds its GroupNorm is conv2 of down block 1's first resnet).
bench.py runs units of two F = 16 calls and one F = 24 call, so a call's type is its position in the unit."""
import re
import sqlite3
import sys
from collections import defaultdict

COND_SHARE = {"F16": 4 / 16, "F24": 12 / 24}  # conditioning rows of a spatial / temporal window (host/schedule.py::plan_sweep)

db = sqlite3.connect(sys.argv[1])
rows = [(re.sub(r"\(anonymous namespace\)::", "", n), s, e) for n, s, e in db.execute("select name, start, end from kernels order by start")]
starts = [i for i, r in enumerate(rows) if "pack_kernel" in r[0] and "vhull" not in r[0]]
calls = [rows[a:b] for a, b in zip(starts, starts[1:] + [len(rows)])]
stat = defaultdict(lambda: defaultdict(list))
for ci, call in enumerate(calls):
    names = [r[0] for r in call]
    attn = [i for i, n in enumerate(names) if "attn" in n]
    silu = [i for i, n in enumerate(names) if n.startswith("silu_kernel")]
    if len(attn) < 3:
        continue
    # the time embedding runs after the pack launch on the single path and in front of it (in the previous segment) with the cache
    first = silu[0] + 2 if silu and silu[0] < attn[0] else 1
    mover = [i for i, n in enumerate(names) if "rows_move_kernel" in n]
    if mover:
        last = mover[0] - 1
    else:
        last = max(i for i in range(attn[2]) if "conv" in names[i])
    # the call ends at its scheduler step; what follows (set-up of the next bench pass) is not the call's
    end = next((i for i, n in enumerate(names) if n.startswith("void cfg_")), len(call) - 1)
    kind = "F16" if ci % 3 < 2 else "F24"
    d = stat[kind]
    d["head_us"].append(sum(e - s for _, s, e in call[first:last + 1]) / 1e3)
    d["head_launches"].append(last + 1 - first)
    d["call_us"].append(sum(e - s for _, s, e in call[:end + 1]) / 1e3)
    d["mover_us"].append(sum(call[i][2] - call[i][1] for i in mover) / 1e3)


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


print(f"# {sys.argv[2]}")
print(f"# window calls found: {len(calls)}; medians over the calls of a type (kernel time, one stack of 2 tasks at a time)")
print(f"{'call':5s} {'calls':>5s} {'head launches':>13s} {'head us':>10s} {'rows_move us':>12s} {'call us':>10s} {'head/call':>9s} "
      f"{'cond rows':>9s} {'cond rows of head us':>20s}")
unit_head, unit_call, unit_mover = 0.0, 0.0, 0.0
for kind, mult in (("F16", 2), ("F24", 1)):
    d = stat[kind]
    if not d["head_us"]:
        continue
    h, c, m = med(d["head_us"]), med(d["call_us"]), med(d["mover_us"])
    print(f"{kind:5s} {len(d['head_us']):5d} {med(d['head_launches']):13d} {h:10.1f} {m:12.1f} {c:10.1f} {h / c:9.4f} "
          f"{COND_SHARE[kind]:9.2f} {h * COND_SHARE[kind]:20.1f}")
    unit_head += mult * h * COND_SHARE[kind]
    unit_call += mult * c
    unit_mover += mult * m
if unit_call:
    print(f"# unit of 2 F16 + 1 F24: kernel time {unit_call / 1e3:.3f} ms; conditioning rows' share of the head as the full-batch launches "
          f"run it: {unit_head / 1e3:.3f} ms = {100 * unit_head / unit_call:.2f} % of the unit; rows_move {unit_mover / 1e3:.3f} ms "
          f"= {100 * unit_mover / unit_call:.2f} %")
