#!/usr/bin/env python
"""Predict per-view 2-D keypoints with a pose network the caller names (diffuman4d_amd/host/pose.py), with the argument names of the
reference's scripts/preprocess/predict_keypoints.py (the ``predict_keypoints`` action of preprocess.sh).

  python tools/predict_keypoints.py --images_dir DATA/SCENE/images --fmasks_dir DATA/SCENE/fmasks \\
      --out_kp2d_dir DATA/SCENE/poses_sapiens --sapiens_ckpt_path CKPT/sapiens_2b_coco_wholebody_..._torchscript.pt2

writes DATA/SCENE/poses_sapiens/{camera}/{frame}.json, which tools/triangulate_skeleton.py --kp2d_dir reads, and prints one JSON line
with counts.  The checkpoint is a local file and is never downloaded.  The person boxes: the whole image, the box of the foreground
mask with --bbox_source fmask, or, as in the reference, those of a person detector the caller names:

  ... --person_detector CKPT/rtmdet_dense.pt --bbox_source detector [--bbox_thr 0.3 --nms_thr 0.3 --det_shape 640,640]

a local TorchScript file that returns (boxes [n, A, 4], scores [n, A, C]) without NMS (diffuman4d_amd/host/detect.py).
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def _ints(text: str):
    return [int(p) for p in text.strip("()[] ").split(",") if p.strip()]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images_dir", required=True, help="searched for **/*.jpg and **/*.webp")
    ap.add_argument("--out_kp2d_dir", required=True, help="receives {camera}/{frame}.json")
    ap.add_argument("--fmasks_dir", default=None, help="searched for **/*.png; paired with the images by sorted index")
    ap.add_argument("--sapiens_ckpt_path", required=True, help="the pose checkpoint (torch.jit when the name contains _torchscript, else torch.export)")
    ap.add_argument("--detector_ckpt_path", default=None, help="refused: the reference's detector checkpoint needs mmdet (see --person_detector)")
    ap.add_argument("--person_detector", default=None, help="a person detector, a local TorchScript file; with --bbox_source detector")
    ap.add_argument("--det_shape", type=_ints, default=[640, 640], help="the detector's input height,width")
    ap.add_argument("--det_cat_id", type=int, default=0, help="the detector's class column of persons")
    ap.add_argument("--bbox_thr", type=float, default=0.3, help="detector score threshold (strict)")
    ap.add_argument("--nms_thr", type=float, default=0.3, help="detector NMS overlap threshold")
    ap.add_argument("--gpu_ids", type=_ints, default=None, help="e.g. 0,1 (default: every device)")
    ap.add_argument("--num_workers", type=int, default=4, help="threads that decode images and write the JSON files (at most 16)")
    ap.add_argument("--shape", type=_ints, default=[1024, 768], help="network input height,width")
    ap.add_argument("--heatmap_scale", type=int, default=4)
    ap.add_argument("--batch_size", type=int, default=4)
    ap.add_argument("--bbox_source", choices=("image", "fmask", "detector"), default="image")
    ap.add_argument("--no_skip_exists", action="store_true", help="predict again even where a file exists and parses")
    ap.add_argument("--device_decode", action="store_true", help="decode JPEG / PNG images and PNG masks on the GPU (the same files are written)")
    args = ap.parse_args(argv)
    if len(args.shape) != 2 or len(args.det_shape) != 2:
        ap.error("--shape and --det_shape take height,width")
    if (args.bbox_source == "detector") != bool(args.person_detector):
        ap.error("--bbox_source detector and --person_detector go together")
    detector = dict(person_detector=args.person_detector, det_shape=tuple(args.det_shape), det_cat_id=args.det_cat_id, bbox_thr=args.bbox_thr,
                    nms_thr=args.nms_thr) if args.person_detector else {}
    from diffuman4d_amd.host import pose
    res = pose.predict_keypoints(args.images_dir, args.out_kp2d_dir, args.fmasks_dir, args.sapiens_ckpt_path, args.detector_ckpt_path, args.gpu_ids,
                                 args.num_workers, shape=tuple(args.shape), heatmap_scale=args.heatmap_scale, batch_size=args.batch_size,
                                 skip_exists=not args.no_skip_exists, bbox_source=args.bbox_source,
                                 **({"device_decode": True} if args.device_decode else {}), **detector)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
