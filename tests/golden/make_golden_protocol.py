#!/usr/bin/env python
"""Record what the REFERENCE's own sampler / runner and ray utilities produce, for the CPU tests that pin this repo to them
(tests/test_reference_protocol.py, tests/test_plucker.py) -- so that those tests run from the repository alone.

Run where the reference checkout exists (REFERENCE_ROOT of oracle/refshim.py):   python tests/golden/make_golden_protocol.py
  * reference_protocol.pt  the reference's SlidingIterativeSampler + SamplingRunner (src/samplers/, imported unmodified through
                           oracle/refshim.py) driving the recording stub pipeline of the test, with one and with two pipelines:
                           the call trace, the stub's per-call bookkeeping, the task lists and labels, the final grid
  * plucker_reference.pt   src/data/utils/ray_utils.py calc_relative_poses / calc_plucker_embeds on the test's cameras
"""
from __future__ import annotations

import importlib.util
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
OUT = Path(__file__).resolve().parent

from oracle import refshim  # noqa: E402


def golden_protocol():
    from diffuman4d_amd.host.dataset import SyntheticSpaTemDataset
    import test_reference_protocol as trp
    refshim.install()
    import src.samplers.sliding_iterative_sampler as ref_mod
    import src.samplers.sampling_runner as run_mod
    from src.samplers.sampling_runner import SamplingRunner
    ref_mod.save_sampling_results = lambda *a, **k: None  # the writer is tested separately (tests/test_results.py)
    ref_mod.check_sampling_results = lambda *a, **k: True
    run_mod.check_sampling_results = lambda *a, **k: True
    out = {"kw": trp.KW}
    for n_pipes in (1, 2):
        ds = SyntheticSpaTemDataset(height=16, width=16, num_cameras=48)
        pipes = [trp.RecordingPipeline() for _ in range(n_pipes)]
        s = ref_mod.SlidingIterativeSampler(ds, pipes, "/tmp/dm4d_unused", **trp.KW)
        SamplingRunner(s).inference()
        latents, tidx = trp._grid(s)
        out[f"pipes{n_pipes}"] = {
            "traces": [p.trace for p in pipes], "calls": [p.calls for p in pipes], "all_tasks": s.all_tasks,
            "spa_labels": list(s.spa_labels), "tem_labels": list(s.tem_labels),
            "latents": latents, "timestep_indices": {c: {f: int(v) for f, v in d.items()} for c, d in tidx.items()}}
    torch.save(out, OUT / "reference_protocol.pt")


def golden_plucker():
    from test_plucker import cameras
    spec = importlib.util.spec_from_file_location("ref_ray_utils", Path(refshim.REFERENCE_ROOT) / "src/data/utils/ray_utils.py")
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    Ks, poses = cameras()
    rel = ref.calc_relative_poses(poses)
    torch.save({"Ks": Ks, "poses": poses, "relative_poses": rel, "plucker_64x40": ref.calc_plucker_embeds(64, 40, Ks, rel)},
               OUT / "plucker_reference.pt")


if __name__ == "__main__":
    golden_protocol()
    golden_plucker()
