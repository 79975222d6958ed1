"""Host stand-ins for ops.skeleton_plan_kp3d and ops.skeleton_draw_planned (tests/test_skel_plan_cpu.py): the plan is the numpy model's
(tests/skel_plan_model.py on triang_model.project), the draw is either the rasteriser model or, by default, a cheap picture of the
records (their digest in the first row), which is all that tests of job lists, grouping and listings look at.  `install` also lets a
"cpu" device through lib.hip_device and records every call."""
import hashlib

import numpy as np
import torch

import kp2d_scene as ks
import skel_plan_model as model
import triang_model
from diffuman4d_amd.host import lib, ops


def install(monkeypatch, paint: bool = False):
    calls = {"plan": [], "draw": []}

    def plan(kp3d, K, T, jobs_host, jobs, scores, scale_host, scale, sizes_host, sizes, links_host, links, colors_host, colors, low, high, span):
        n, L = jobs_host.shape[0], links_host.shape[0]
        calls["plan"].append({"jobs": jobs_host.tolist(), "scale": scale_host.tolist(), "sizes": sizes_host.tolist(),
                              "scores": None if scores is None else scores.numpy().copy()})
        records = torch.zeros((n, 3 * L, ops.SKEL_FIELDS), dtype=torch.int32)
        counts, status = torch.zeros(n, dtype=torch.int32), torch.zeros((n, 2), dtype=torch.int32)
        for i, (f, cam) in enumerate(jobs_host.tolist()):
            with np.errstate(all="ignore"):
                uv, depth = triang_model.project(kp3d[f:f + 1].numpy(), K[cam:cam + 1].numpy(), T[cam:cam + 1].numpy())
            rec, bits, dropped = model.plan(uv[0, 0], depth[0, 0], None if scores is None else scores[i].numpy(), *scale_host[i].tolist(),
                                            *sizes_host[i].tolist(), links_host.numpy(), colors_host.numpy(), low, high, span)
            records[i, :len(rec)] = torch.from_numpy(rec)
            counts[i], status[i, 0], status[i, 1] = len(rec), bits, dropped
        return records, counts, status

    def draw(records, counts, htab_host, htab, hk, vtab_host, vtab, vk, H, W, h, w, out=None):
        n = records.shape[0]
        calls["draw"].append({"n": n, "hw": (h, w), "canvas": (H, W)})
        if out is None:
            out = torch.empty((n, h, w, 3), dtype=torch.uint8)
        for i in range(n):
            rec = records[i, :int(counts[i])].numpy()
            if paint:
                out[i] = torch.from_numpy(ks.model_map(rec, (H, W), (w, h)).copy())
            else:
                out[i] = 0
                out[i, 0, :10] = torch.from_numpy(np.frombuffer(hashlib.sha256(rec.tobytes()).digest()[:30], dtype=np.uint8).reshape(10, 3).copy())
        return out

    monkeypatch.setattr(ops, "skeleton_plan_kp3d", plan)
    monkeypatch.setattr(ops, "skeleton_draw_planned", draw)
    monkeypatch.setattr(lib, "hip_device", lambda device, what: torch.device(device))
    return calls
