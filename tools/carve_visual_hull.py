#!/usr/bin/env python
"""Carve one visual-hull point cloud per frame from a scene's foreground masks and cameras (diffuman4d_amd/host/vhull.py), with
the argument names of the reference's scripts/preprocess/carve_visual_hull.py (the ``carve_vhull`` action of preprocess.sh).

  python tools/carve_visual_hull.py --fmasks_dir DATA/SCENE/fmasks --cameras_path DATA/SCENE/transforms.json \\
      --out_vhull_dir DATA/SCENE/surfs --sparse_pcd DATA/SCENE/sparse_pcd.ply

writes DATA/SCENE/surfs/{frame}.ply, DATA/SCENE/surfs_bounds.json and the first frame's cloud as sparse_pcd.ply.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def _range(text: str):
    """'0,None,1' (brackets optional) -> (0, None, 1)."""
    parts = [p.strip() for p in text.strip("()[] ").split(",")]
    if len(parts) != 3:
        raise argparse.ArgumentTypeError(f"expected begin,end,step, got {text!r}")
    return tuple(None if p in ("None", "none", "") else int(p) for p in parts)


def _bounds(text: str):
    parts = [float(p) for p in text.strip("()[] ").split(",")]
    if len(parts) != 6:
        raise argparse.ArgumentTypeError(f"expected xmin,xmax,ymin,ymax,zmin,zmax, got {text!r}")
    return tuple(parts)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--fmasks_dir", required=True, help="fmasks/{camera}/{frame}.png")
    ap.add_argument("--cameras_path", required=True, help="nerfstudio transforms.json")
    ap.add_argument("--out_vhull_dir", required=True, help="receives {frame}.ply; {out_vhull_dir}_bounds.json is written beside it")
    ap.add_argument("--camera_range", type=_range, default=(0, None, 1), help="begin,end,step over the sorted cameras")
    ap.add_argument("--frame_range", type=_range, default=(0, None, 1), help="begin,end,step over the sorted frames")
    ap.add_argument("--bounds", type=_bounds, default=(-3.0, 3.0, -3.0, 3.0, -3.0, 3.0), help="enlarge it if the result is empty")
    ap.add_argument("--voxel_size", type=float, default=0.025)
    ap.add_argument("--batch_size", type=float, default=1e6, help="upper bound on the voxels per launch series")
    ap.add_argument("--min_views", type=int, default=None, help="keep voxels seen by at least this many views (default: by all)")
    ap.add_argument("--sparse_pcd", default=None, help="also write the first frame's cloud here")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--host_threads", type=int, default=8, help="mask decode threads (at most 16)")
    ap.add_argument("--device_decode", action="store_true", help="decode the PNG masks on the GPU (host/pngdec.py): the same files are written")
    args = ap.parse_args(argv)
    from diffuman4d_amd.host import vhull
    res = vhull.carve_scene(args.fmasks_dir, args.cameras_path, args.out_vhull_dir, camera_range=args.camera_range,
                            frame_range=args.frame_range, bounds=args.bounds, voxel_size=args.voxel_size, batch_size=args.batch_size,
                            min_views=args.min_views, device=args.device, sparse_pcd_path=args.sparse_pcd, host_threads=args.host_threads,
                            **({"device_decode": True} if args.device_decode else {}))
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
