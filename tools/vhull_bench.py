#!/usr/bin/env python
"""Time visual-hull carving (diffuman4d_amd/host/vhull.py) on the reference's default job: bounds +-3, voxel 0.025 (240^3 voxels),
48 views of 1024 x 1024 masks of a projected synthetic body, every-view mode and min_views = 40.

Per mode, after a warm-up, HIP events around one frame's work, the median of --reps frames:
  native   dm4d_vhull_pack_masks + the chunks of dm4d_vhull_carve_chunk + the one read of the count (masks, P and axes already on
           the device); `pack` is the mask packing alone and `chunks` the three launches per chunk over the whole grid, without
           the packing and without the read (the split by kernel: run this file with --native-only under a kernel trace)
  torch    the same semantics written with torch operators on the same device in this process, in batches of 1e6 voxels as the
           reference walks them (this file's own restatement: not the reference's file, not the code under test)
and the kept count, the bytes of the masks in both forms, and whether the two results are identical.

  python tools/vhull_bench.py [--views 48 --size 1024 --voxel 0.025 --reps 5]
"""
from __future__ import annotations

import argparse
import json
import math
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from diffuman4d_amd.host import ops, vhull  # noqa: E402

BODY = [((0.0, 0.0, 0.0), (0.25, 0.55, 0.18)), ((0.02, 0.70, 0.01), (0.13, 0.15, 0.14)),
        ((-0.12, -0.85, 0.0), (0.09, 0.45, 0.09)), ((0.12, -0.85, 0.02), (0.09, 0.45, 0.09))]


def scene(views: int, size: int, dev):
    """-> (masks bool [views, size, size] on dev, P fp64 [views, 3, 4] on the host): cameras on a ring of radius 2.6, the body = four
    ellipsoids rendered through each pixel centre."""
    f = 1.15 * size
    K = torch.tensor([[f, 0, size / 2 - 0.3], [0, f, size / 2 + 0.2], [0, 0, 1]], dtype=torch.float64)
    vv, uu = torch.meshgrid(torch.arange(size, dtype=torch.float64, device=dev), torch.arange(size, dtype=torch.float64, device=dev),
                            indexing="ij")
    masks, Ps = [], []
    for c in range(views):
        a = 2 * math.pi * c / views + 0.1
        o = torch.tensor([2.6 * math.cos(a), 0.1 + 0.3 * math.sin(3 * a), 2.6 * math.sin(a)], dtype=torch.float64)
        fwd = -o / o.norm()  # OpenCV: +z looks at the subject, +y down
        right = torch.linalg.cross(fwd, torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64))
        right = right / right.norm()
        down = torch.linalg.cross(fwd, right)
        R = torch.stack([right, down, fwd])  # world -> camera
        Ps.append(K @ torch.cat([R, (-R @ o).reshape(3, 1)], dim=1))
        d = (torch.stack([(uu - K[0, 2]) / f, (vv - K[1, 2]) / f, torch.ones_like(uu)], dim=-1) @ R.to(dev))  # camera -> world: R^T
        hit = torch.zeros((size, size), dtype=torch.bool, device=dev)
        for centre, radii in BODY:
            r = torch.tensor(radii, dtype=torch.float64, device=dev)
            dd, oo = d / r, (o.to(dev) - torch.tensor(centre, dtype=torch.float64, device=dev)) / r
            A, B, C = (dd * dd).sum(-1), (dd * oo).sum(-1), (oo * oo).sum() - 1.0
            hit |= (B * B - A * C >= 0) & (B < 0)
        masks.append(hit)
    return torch.stack(masks), torch.stack(Ps)


def torch_carve(fmasks, P, axes, min_views, batch=1_000_000):
    """The semantics of include/dm4d.h in torch operators (fp64, the same operation order), batch by batch."""
    xs, ys, zs = axes
    B, H, W = fmasks.shape
    ny, nz = ys.numel(), zs.numel()
    N = xs.numel() * ny * nz
    need = B if min_views is None else int(min_views)
    bidx = torch.arange(B, device=P.device).view(B, 1)
    kept = []
    for start in range(0, N, batch):
        idx = torch.arange(start, min(start + batch, N), device=P.device)
        X = torch.stack([xs[idx // (ny * nz)], ys[(idx // nz) % ny], zs[idx % nz]], dim=-1)
        Xd = X.to(torch.float64)
        X0, X1, X2 = Xd[None, :, 0], Xd[None, :, 1], Xd[None, :, 2]
        r = [((P[:, k, 0:1] * X0 + P[:, k, 1:2] * X1) + P[:, k, 2:3] * X2) + P[:, k, 3:4] for k in range(3)]
        z = r[2]
        den = z.clamp_min(1e-8)
        u, v = torch.round(r[0] / den), torch.round(r[1] / den)
        valid = (z > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
        ui = torch.where(valid, u, torch.zeros_like(u)).to(torch.long)
        vi = torch.where(valid, v, torch.zeros_like(v)).to(torch.long)
        inside = valid & fmasks[bidx.expand_as(ui), vi, ui]
        keep = inside.sum(dim=0) >= need
        kept.append(X[keep])
    return torch.cat(kept, dim=0)


def timed(fn, reps: int):
    for _ in range(2):  # warm-up: code objects, then the allocator's steady state
        out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = fn()
        e.record()
        e.synchronize()
        ms.append(s.elapsed_time(e))
    return out, statistics.median(ms), min(ms), max(ms)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--views", type=int, default=48)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--voxel", type=float, default=0.025)
    ap.add_argument("--bound", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch_size", type=float, default=1e6)
    ap.add_argument("--native-only", action="store_true", help="skip the torch composition (for a run under a kernel trace)")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("vhull_bench needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda", torch.cuda.current_device())
    fmasks, P = scene(args.views, args.size, dev)
    b = args.bound
    axes = tuple(a.to(dev) for a in vhull.build_voxel_grid_linspaces((-b, b, -b, b, -b, b), args.voxel))
    Pd = P.to(dev)
    hw = (args.size, args.size)
    N = axes[0].numel() * axes[1].numel() * axes[2].numel()
    head = {"voxels": N, "views": args.views, "mask": f"{args.size}x{args.size}", "batch_size": int(args.batch_size),
            "mask_bytes_bool": fmasks.numel(), "mask_bytes_bits": args.views * args.size * ((args.size + 31) // 32) * 4,
            "foreground_fraction": round(float(fmasks.float().mean()), 4)}
    print(json.dumps(head), flush=True)
    _, pack_ms, _, _ = timed(lambda: ops.vhull_pack_masks(fmasks), args.reps)
    bits = ops.vhull_pack_masks(fmasks)
    chunk = vhull._chunk_voxels(args.batch_size)
    ws, total = ops.vhull_ws(min(chunk, N), dev), torch.zeros(1, dtype=torch.int64, device=dev)
    out = torch.empty((min(N, max(1 << 20, N // 16)), 3), dtype=torch.float32, device=dev)

    def chunks(need):
        total.zero_()
        for first in range(0, N, chunk):
            ops.vhull_carve_chunk(*axes, Pd, bits, hw, need, first, min(chunk, N - first), ws, total, out)

    for min_views in (None, 40 if args.views >= 40 else max(1, args.views - 1)):
        native, n_ms, n_lo, n_hi = timed(lambda: vhull._carve(ops.vhull_pack_masks(fmasks), hw, Pd, axes, args.batch_size, min_views), args.reps)
        _, c_ms, c_lo, c_hi = timed(lambda: chunks(0 if min_views is None else min_views), args.reps)
        row = {"min_views": min_views, "kept": int(native.shape[0]), "native_ms": round(n_ms, 3), "native_ms_range": [round(n_lo, 3), round(n_hi, 3)],
               "pack_ms": round(pack_ms, 3), "chunks_ms": round(c_ms, 3), "chunks_ms_range": [round(c_lo, 3), round(c_hi, 3)],
               "launch_series": -(-N // chunk), "nominal_gvoxel_views_per_s": round(N * args.views / n_ms / 1e6, 1)}
        if not args.native_only:
            ref, t_ms, t_lo, t_hi = timed(lambda: torch_carve(fmasks, Pd, axes, min_views), args.reps)
            row.update({"identical_to_torch": bool(torch.equal(native, ref)), "torch_ms": round(t_ms, 3),
                        "torch_ms_range": [round(t_lo, 3), round(t_hi, 3)], "torch_over_native": round(t_ms / n_ms, 2)})
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
