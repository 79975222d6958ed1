#!/usr/bin/env python
"""Triangulate a scene's 3-D skeletons from its per-view 2-D keypoints and cameras (diffuman4d_amd/host/triang.py), with the argument
names of the reference's scripts/preprocess/triangulate_skeleton.py (the ``triangulate_skeleton`` action of preprocess.sh).

  python tools/triangulate_skeleton.py --camera_path DATA/SCENE/transforms.json --kp2d_dir DATA/SCENE/poses_sapiens \\
      --out_kp3d_dir DATA/SCENE/poses_3d --out_pcd_dir DATA/SCENE/poses_pcd --out_kp2d_proj_dir DATA/SCENE/poses_2d

writes DATA/SCENE/poses_3d/{frame}.json, DATA/SCENE/poses_pcd/{frame}.ply and DATA/SCENE/poses_2d/{camera}/{frame}.json, and prints
one JSON line with counts.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def _numbers(kind, count=None):
    def parse(text: str):
        parts = [p.strip() for p in text.strip("()[] ").split(",") if p.strip()]
        if count is not None and len(parts) != count:
            raise argparse.ArgumentTypeError(f"expected {count} comma-separated values, got {text!r}")
        return [kind(p) for p in parts]
    return parse


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--camera_path", required=True, help="nerfstudio transforms.json")
    ap.add_argument("--kp2d_dir", required=True, help="poses_sapiens/{camera}/{frame}.json")
    ap.add_argument("--out_kp3d_dir", required=True, help="receives {frame}.json")
    ap.add_argument("--out_pcd_dir", default=None, help="receives {frame}.ply (the k points of each frame)")
    ap.add_argument("--out_kp2d_proj_dir", default=None, help="receives {camera}/{frame}.json with keypoints and keypoint_depths")
    ap.add_argument("--spa_label_range", type=_numbers(int, 3), default=None, help="begin,end,step over camera labels")
    ap.add_argument("--spa_label_proj_range", type=_numbers(int, 3), default=None, help="begin,end,step over the cameras to project into")
    ap.add_argument("--tem_label_range", type=_numbers(int, 3), default=None, help="begin,end,step over frame labels")
    ap.add_argument("--spa_labels", type=_numbers(int), default=None, help="camera labels, e.g. 0,4,8")
    ap.add_argument("--spa_labels_proj", type=_numbers(int), default=None, help="labels of the cameras to project into")
    ap.add_argument("--tem_labels", type=_numbers(int), default=None, help="frame labels")
    ap.add_argument("--kp2d_padding", type=_numbers(float, 2), default=None, help="x,y added to every 2-D keypoint")
    ap.add_argument("--intri_scale", type=float, default=None, help="multiplies the intrinsics (K[2, 2] stays 1)")
    ap.add_argument("--skip_exists", action="store_true", help="leave frames whose poses_3d file exists and parses")
    ap.add_argument("--num_workers", type=int, default=8, help="threads that read and write the JSON files (at most 16)")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    from diffuman4d_amd.host import triang
    res = triang.triangulate_skeleton(args.camera_path, args.kp2d_dir, args.out_kp3d_dir, out_pcd_dir=args.out_pcd_dir,
                                      out_kp2d_proj_dir=args.out_kp2d_proj_dir, spa_label_range=args.spa_label_range,
                                      spa_label_proj_range=args.spa_label_proj_range, tem_label_range=args.tem_label_range,
                                      spa_labels=args.spa_labels, spa_labels_proj=args.spa_labels_proj, tem_labels=args.tem_labels,
                                      kp2d_padding=args.kp2d_padding, intri_scale=args.intri_scale, skip_exists=args.skip_exists,
                                      num_workers=args.num_workers, device=args.device)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
