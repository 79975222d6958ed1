#!/usr/bin/env python
"""What ``device_cache`` does to the loader side of a whole job (diffuman4d_amd/host/capture.py, host/capture_cache.py): the three
rounds of a 4D job driven through ``get_item`` with the flag off and on, alternately in one process on the same kernels.

A synthetic scene of tools/capture_bench.py is written once: 48 cameras x --frames frames (default 30), --src sources (default
1024x1024), samples of --out (default 576x320), 4 input cameras.  It is read as two scenes:
  dna_rendering  WebP images and skeleton maps, PNG masks
  fdvai          JPEG images and skeleton maps (quality 90, 4:2:0), PNG masks
each with ``device_decode`` off and on and plucker="cameras" (no Pluecker maps on the host: what is left of ``get_item`` is the loader's
own work), and the first once more with plucker="host", the dataset's default, whose fp32 maps of every row are computed on the CPU
inside ``get_item`` whatever the flag.  A job is round 1: one spatial task per frame (48 cells each), round 2: one temporal task per
target camera (44 tasks of 2 x frames cells), round 3: round 1 again -- the tasks of a round handed to --loaders (3) concurrent threads
that call ``get_item`` with --threads (16) decode threads, as the runner's loader threads do.  The flag-on dataset's cache is cleared
before each of its jobs.  JSON lines, written to --log (default profiles/capture_cache_bench.log):
  job        per scene and device_decode: wall seconds per round, flag off and on alternately for --rounds jobs each (every time, the
             median and the range, the ratio of the medians), image / mask / skeleton files opened per round, bytes uploaded per job
             (flag off without device_decode: 7 bytes per source pixel per cell load; with it: ``decode_stats["bytes_uploaded"]``),
             bytes the cache retains, its counters, whether every sample of the last flag-on job equalled the flag-off one
  launches   device time per row of the pack launch pair and of the unpack launch, by HIP events around the two ops calls of one
             spatial round loaded cold and once more from cells (not part of the timed jobs)
  hit_call   wall time of one spatial ``get_item`` served from cells only, with plucker="host" (the dataset's default: fp32 Pluecker
             maps on the CPU) and plucker="cameras": what a hit-only call spends outside the unpack launch

  python tools/capture_cache_bench.py [--frames 30 --rounds 5 --host-plucker-rounds 5 --threads 16 --loaders 3 --src 1024x1024 --out 576x320]
"""
from __future__ import annotations

import argparse
import json
import shutil
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from capture_bench import write_scene  # noqa: E402
from capture_decode_bench import SCENES, add_jpeg_files, spread  # noqa: E402
from diffuman4d_amd.host import capture, ops  # noqa: E402

INPUTS = ["01", "13", "25", "37"]
CAMS = [f"{c:02d}" for c in range(48)]
OPENED = []  # every path capture._open / capture._read is asked for (list.append is atomic)


def count_opens() -> None:
    for name in ("_open", "_read"):
        real = getattr(capture, name)
        setattr(capture, name, lambda path, mode, _real=real: OPENED.append(path) or _real(path, mode))


def rounds_of(frames):
    tems = [f"{t:06d}" for t in range(frames)]
    spatial = [(CAMS, [t]) for t in tems]
    temporal = [([c], tems) for c in CAMS if c not in INPUTS]
    return [("1 spatial", spatial), ("2 temporal", temporal), ("3 spatial", spatial)]


def run_job(ds, frames: int, loaders: int, keep=None):
    """One job -> (wall seconds per round, files opened per round, cell loads asked for)."""
    secs, opened, cells = [], [], 0
    with ThreadPoolExecutor(loaders, thread_name_prefix="loader") as ex:
        for name, tasks in rounds_of(frames):
            del OPENED[:]
            t0 = time.perf_counter()
            out = list(ex.map(lambda task: ds.get_item("bench", task[0], task[1], INPUTS), tasks))
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
            opened.append(len(OPENED))
            cells += sum(len(s["labels"]) for s in out)
            if keep is not None:  # a digest per sample: the samples themselves would not fit
                keep.append([(float(s["pixel_values"].double().sum()), float(s["skeletons"].double().sum()), s["crops"]) for s in out])
    return secs, opened, cells


def bench_job(root: Path, name: str, device_decode: bool, plucker: str, jobs: int, a, hw) -> dict:
    images, skeletons, ext = SCENES[name]
    H, W = a.out_hw
    kw = dict(data_dir=str(root), scene_label="bench", height=H, width=W, decode_threads=a.threads, plucker=plucker,
              image_path_pat="{data_dir}/{scene_label}/" + images + "/{spa_label}/{tem_label}" + ext,
              skeleton_path_pat="{data_dir}/{scene_label}/" + skeletons + "/{spa_label}/{tem_label}" + ext,
              **({"device_decode": True} if device_decode else {}))
    ds = {False: capture.SpaTemDataset(**kw), True: capture.SpaTemDataset(device_cache=True, device_cache_bytes=a.cache_gb << 30, **kw)}
    times = {False: [], True: []}
    opened, digests, uploaded, cells, stats = {}, {}, {}, {}, None
    for r in range(jobs):
        for flag in (False, True):
            if flag:
                ds[True].clear_device_cache()
            before = ds[flag].decode_stats["bytes_uploaded"]
            digests[flag] = []
            secs, opened[flag], cells[flag] = run_job(ds[flag], a.frames, a.loaders, digests[flag] if r == jobs - 1 else None)
            times[flag].append(secs)
            print(f"# {name} device_decode={device_decode} plucker={plucker} job {r} device_cache={flag}: {[round(s, 2) for s in secs]} s", flush=True)
            loads = cells[False]  # flag off: every cell a task names is loaded
            if flag:
                now = ds[True].cache_stats
                loads, stats = now["misses"] - (stats["misses"] if stats else 0), now
            uploaded[flag] = ds[flag].decode_stats["bytes_uploaded"] - before if device_decode else loads * hw[0] * hw[1] * 7
    per_round = {}
    for i, (rname, _) in enumerate(rounds_of(a.frames)):
        off, on = [t[i] for t in times[False]], [t[i] for t in times[True]]
        per_round[rname] = {"flag_off": spread(off), "flag_on": spread(on), "off_over_on": round(statistics.median(off) / statistics.median(on), 3),
                            "files_opened_flag_off": opened[False][i], "files_opened_flag_on": opened[True][i]}
    tot_off, tot_on = [sum(t) for t in times[False]], [sum(t) for t in times[True]]
    res = {"what": "job", "scene": name, "device_decode": device_decode, "plucker": plucker, "frames": a.frames, "src": [hw[1], hw[0]], "out": [H, W], "loaders": a.loaders,
           "decode_threads": a.threads, "jobs_each": jobs, "timing": "wall clock per round of a job, flag off and on alternately; the cache is cleared before each flag-on job",
           "rounds": per_round, "job_flag_off": spread(tot_off), "job_flag_on": spread(tot_on),
           "job_off_over_on": round(statistics.median(tot_off) / statistics.median(tot_on), 3),
           "cell_loads_per_job": cells[False], "distinct_cells": 48 * a.frames, "bytes_uploaded_per_job_flag_off": uploaded[False],
           "bytes_uploaded_per_job_flag_on": uploaded[True], "bytes_retained": stats["bytes"], "cache_stats_all_jobs": stats,
           "equal": digests[False] == digests[True]}
    ds[True].clear_device_cache()
    return res, ds


def bench_launches(ds_on, a) -> dict:
    """HIP events around the two ops calls of one spatial task, cold and from cells."""
    ms = {"pack": [], "unpack": []}
    real = {"pack": ops.capture_crop_resize_packed, "unpack": ops.capture_unpack_cells}

    def timed(name):
        def w(*args, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = real[name](*args, **kw)
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
            return out
        return w
    ops.capture_crop_resize_packed, ops.capture_unpack_cells = timed("pack"), timed("unpack")
    try:
        for t in range(min(a.frames, 6)):  # the first task warms the code objects up
            ds_on.get_item("bench", CAMS, [f"{t:06d}"], INPUTS)
        for t in range(min(a.frames, 6)):
            ds_on.get_item("bench", CAMS, [f"{t:06d}"], INPUTS)
    finally:
        ops.capture_crop_resize_packed, ops.capture_unpack_cells = real["pack"], real["unpack"]
    ds_on.clear_device_cache()
    return {"what": "launches", "rows_per_call": 48, "out": list(a.out_hw), "timing": "HIP events around the ops call (both launches of the pack), first call dropped",
            "pack_us_per_row": round(1e3 * statistics.median(ms["pack"][1:]) / 48, 2), "unpack_us_per_row": round(1e3 * statistics.median(ms["unpack"][1:]) / 48, 2),
            "pack_ms_per_call": spread(ms["pack"][1:])["median"], "unpack_ms_per_call": spread(ms["unpack"][1:])["median"]}


def bench_hit_call(kw_of, a) -> dict:
    out = {"what": "hit_call", "rows": 48, "out": list(a.out_hw), "timing": "wall clock of a spatial get_item whose 48 cells are all hits, median of 9"}
    for plucker in ("host", "cameras"):
        ds = capture.SpaTemDataset(device_cache=True, plucker=plucker, **kw_of)
        ds.get_item("bench", CAMS, ["000000"], INPUTS)
        ts = []
        for _ in range(9):
            t0 = time.perf_counter()
            ds.get_item("bench", CAMS, ["000000"], INPUTS)
            ts.append(time.perf_counter() - t0)
        out[f"ms_plucker_{plucker}"] = round(1e3 * statistics.median(ts), 3)
        ds.clear_device_cache()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--src", default="1024x1024", help="source size W x H")
    ap.add_argument("--out", default="576x320", help="sample size H x W")
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5, help="jobs per flag setting")
    ap.add_argument("--host-plucker-rounds", type=int, default=5, help="jobs per flag setting of the plucker=\"host\" run (0: leave it out)")
    ap.add_argument("--threads", type=int, default=16, help="decode threads of the dataset")
    ap.add_argument("--loaders", type=int, default=3, help="concurrent get_item calls")
    ap.add_argument("--cache-gb", type=int, default=16)
    ap.add_argument("--scenes", default="dna_rendering,fdvai")
    ap.add_argument("--log", default=str(ROOT / "profiles" / "capture_cache_bench.log"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("capture_cache_bench: no HIP device (nothing here is measured without one)")
    a.out_hw = tuple(int(v) for v in a.out.split("x"))
    W, H = (int(v) for v in a.src.split("x"))
    lines = [{"what": "run", "device": torch.cuda.get_device_name(torch.cuda.current_device()), "args": {k: v for k, v in vars(a).items()}}]
    count_opens()
    tmp = Path(tempfile.mkdtemp(prefix="dm4d_capture_cache_"))

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)
        Path(a.log).parent.mkdir(parents=True, exist_ok=True)
        with open(a.log, "w") as f:  # rewritten after every line: a run that is cut short leaves what it measured
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    try:
        t0 = time.perf_counter()
        write_scene(tmp / "bench", W, H, 48, a.frames, temporal_cams=CAMS, threads=a.threads)
        add_jpeg_files(tmp / "bench", a.threads)
        print(f"# scene written in {time.perf_counter() - t0:.1f} s", flush=True)
        last = None
        for name in a.scenes.split(","):
            for device_decode in (False, True):
                res, last = bench_job(tmp, name, device_decode, "cameras", a.rounds, a, (H, W))
                emit(res)
        emit(bench_launches(last[True], a))
        images, skeletons, ext = SCENES[a.scenes.split(",")[0]]
        emit(bench_hit_call(dict(data_dir=str(tmp), scene_label="bench", height=a.out_hw[0], width=a.out_hw[1], decode_threads=a.threads,
                                 image_path_pat="{data_dir}/{scene_label}/" + images + "/{spa_label}/{tem_label}" + ext,
                                 skeleton_path_pat="{data_dir}/{scene_label}/" + skeletons + "/{spa_label}/{tem_label}" + ext), a))
        if a.host_plucker_rounds > 0:  # the dataset's default: fp32 Pluecker maps of every row on the CPU, inside get_item
            emit(bench_job(tmp, a.scenes.split(",")[0], False, "host", a.host_plucker_rounds, a, (H, W))[0])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
