#!/usr/bin/env python
"""Preprocess one captured scene: the five actions of the reference's scripts/preprocess/preprocess.sh, in process, each by this
package's native stage, with the reference's action names, default order and default sub-directories of ``--data_dir``.

  python tools/preprocess.py --data_dir DATA/SCENE [--actions remove_background,carve_vhull,...] \\
      --matting_model_dir CKPT/BiRefNet --sapiens_ckpt_path CKPT/sapiens_..._torchscript.pt2 --palette palette.json \\
      [--person_detector CKPT/rtmdet_dense.pt --bbox_source detector [--bbox_thr 0.3 --nms_thr 0.3 --det_shape 640,640]]

  remove_background      images/ -> fmasks/                                   (tools/remove_background.py; needs --matting_model_dir)
  carve_vhull            fmasks/ + transforms.json -> surfs/, and surfs/000000.ply is copied to sparse_pcd.ply (tools/carve_visual_hull.py)
  predict_keypoints      images/ + fmasks/ -> poses_sapiens/                  (tools/predict_keypoints.py; needs --sapiens_ckpt_path)
  triangulate_skeleton   transforms.json + poses_sapiens/ -> poses_3d/, poses_pcd/, poses_2d/      (tools/triangulate_skeleton.py)
  draw_skeleton          poses_2d/ -> skeletons/                              (tools/draw_skeleton.py; needs --palette)
                         with --skeleton_from kp3d: poses_3d/ + transforms.json -> skeletons/, and no poses_2d/ is written

The two networks and the palette are the caller's files; nothing is downloaded.  An unknown action is an error before anything runs.
Prints one JSON line per action with the stage's counts.
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

ALL_ACTIONS = ("remove_background", "carve_vhull", "predict_keypoints", "triangulate_skeleton", "draw_skeleton")  # preprocess.sh:6


def _remove_background(*args, **kw):
    from diffuman4d_amd.host import matting
    return matting.remove_background(*args, **kw)


def _carve_vhull(*args, **kw):
    from diffuman4d_amd.host import vhull
    return vhull.carve_scene(*args, **kw)


def _predict_keypoints(*args, **kw):
    from diffuman4d_amd.host import pose
    return pose.predict_keypoints(*args, **kw)


def _triangulate_skeleton(*args, **kw):
    from diffuman4d_amd.host import triang
    return triang.triangulate_skeleton(*args, **kw)


def _draw_skeleton(*args, **kw):
    from diffuman4d_amd.host import skeleton
    return skeleton.draw_skeleton(*args, **kw)


# action -> the stage function it calls; every call goes through this dict (a test substitutes recorders)
STAGES = {"remove_background": _remove_background, "carve_vhull": _carve_vhull, "predict_keypoints": _predict_keypoints,
          "triangulate_skeleton": _triangulate_skeleton, "draw_skeleton": _draw_skeleton}


def parse_actions(text) -> list:
    """'a,b,c' -> ['a', 'b', 'c'] in the given order; nothing given: all five in the reference's order.  An unknown name: ValueError."""
    actions = [a.strip() for a in (text or "").split(",") if a.strip()] or list(ALL_ACTIONS)
    for act in actions:
        if act not in ALL_ACTIONS:
            raise ValueError(f"Invalid action: {act} (known: {', '.join(ALL_ACTIONS)})")
    return actions


def run(data_dir: str, actions, *, matting_model_dir=None, sapiens_ckpt_path=None, palette=None, batch_size: int = 8,
        device_png: bool = False, device_decode: bool = False, person_detector=None, bbox_source=None, bbox_thr=None, nms_thr=None,
        det_shape=None, skeleton_from: str = "kp2d", device_webp: bool = False) -> list:
    """Run `actions` on the scene under `data_dir` (preprocess.sh:31-77) -> [(action, what its stage returned)].  person_detector,
    bbox_source, bbox_thr, nms_thr, det_shape: handed to predict_keypoints when given.  skeleton_from="kp3d": triangulate_skeleton
    writes no poses_2d directory and draw_skeleton projects poses_3d into the cameras of transforms.json on the device (the same maps).
    device_webp: draw_skeleton encodes its maps on the device as lossless WebP (the files decode to exactly the maps)."""
    if skeleton_from not in ("kp2d", "kp3d"):
        raise ValueError(f"skeleton_from must be 'kp2d' or 'kp3d', got {skeleton_from!r}")
    d = str(data_dir)
    out = []
    for act in actions:
        if act == "remove_background":
            extra = {"device_png": True} if device_png else {}
            if device_decode:
                extra["device_decode"] = True
            res = STAGES[act](f"{d}/images", f"{d}/fmasks", model_name=matting_model_dir, batch_size=batch_size, **extra)
        elif act == "carve_vhull":
            res = STAGES[act](f"{d}/fmasks", f"{d}/transforms.json", f"{d}/surfs", **({"device_decode": True} if device_decode else {}))
            shutil.copyfile(f"{d}/surfs/000000.ply", f"{d}/sparse_pcd.ply")
        elif act == "predict_keypoints":
            extra = {"device_decode": True} if device_decode else {}
            extra.update({k: v for k, v in (("person_detector", person_detector), ("bbox_source", bbox_source), ("bbox_thr", bbox_thr),
                                            ("nms_thr", nms_thr), ("det_shape", det_shape)) if v is not None})
            res = STAGES[act](f"{d}/images", f"{d}/poses_sapiens", f"{d}/fmasks", sapiens_ckpt_path, **extra)
        elif act == "triangulate_skeleton":
            extra = {"out_kp2d_proj_dir": f"{d}/poses_2d"} if skeleton_from == "kp2d" else {}
            res = STAGES[act](f"{d}/transforms.json", f"{d}/poses_sapiens", f"{d}/poses_3d", out_pcd_dir=f"{d}/poses_pcd", **extra)
        elif skeleton_from == "kp3d":
            res = STAGES[act](None, f"{d}/skeletons", palette=palette, kp3d_dir=f"{d}/poses_3d", camera_path=f"{d}/transforms.json",
                              **({"device_webp": True} if device_webp else {}))
        else:
            res = STAGES[act](f"{d}/poses_2d", f"{d}/skeletons", palette=palette, **({"device_webp": True} if device_webp else {}))
        out.append((act, res))
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--data_dir", required=True, help="the scene: images/ and transforms.json, and what the earlier actions wrote")
    ap.add_argument("--actions", default=None, help=f"comma-separated, run in the given order (default: {','.join(ALL_ACTIONS)})")
    ap.add_argument("--matting_model_dir", default=None, help="remove_background: the matting network, a local directory")
    ap.add_argument("--sapiens_ckpt_path", default=None, help="predict_keypoints: the pose checkpoint, a local file")
    ap.add_argument("--person_detector", default=None, help="predict_keypoints: a person detector, a local TorchScript file; with --bbox_source detector")
    ap.add_argument("--bbox_source", choices=("image", "fmask", "detector"), default=None, help="predict_keypoints: where the person boxes come from (default: the whole image)")
    ap.add_argument("--bbox_thr", type=float, default=None, help="predict_keypoints with a detector: score threshold (default 0.3)")
    ap.add_argument("--nms_thr", type=float, default=None, help="predict_keypoints with a detector: NMS overlap threshold (default 0.3)")
    ap.add_argument("--det_shape", type=lambda t: tuple(int(p) for p in t.strip("()[] ").split(",")), default=None,
                    help="predict_keypoints with a detector: its input height,width (default 640,640)")
    ap.add_argument("--palette", default=None, help="draw_skeleton: JSON file with keypoint_colors, links and x_link_color")
    ap.add_argument("--batch_size", type=int, default=8, help="remove_background: images per batch (decrease it if memory runs out)")
    ap.add_argument("--device_png", action="store_true", help="remove_background: encode the mask PNG files on the GPU (same pixels, other bytes)")
    ap.add_argument("--device_decode", action="store_true", help="remove_background: decode baseline JPEG inputs on the GPU; carve_vhull: decode the PNG masks there; predict_keypoints: decode JPEG / PNG images and PNG masks there (same files written)")
    ap.add_argument("--skeleton_from", choices=("kp2d", "kp3d"), default="kp2d",
                    help="kp3d: triangulate_skeleton writes no poses_2d/ and draw_skeleton draws from poses_3d/ and transforms.json (the same maps)")
    ap.add_argument("--device_webp", action="store_true", help="draw_skeleton: encode the maps on the GPU as lossless WebP (the files decode to exactly the maps)")
    args = ap.parse_args(argv)
    try:
        actions = parse_actions(args.actions)
    except ValueError as e:
        ap.error(str(e))
    for act, flag in (("remove_background", "matting_model_dir"), ("predict_keypoints", "sapiens_ckpt_path"), ("draw_skeleton", "palette")):
        if act in actions and not getattr(args, flag):
            ap.error(f"{act} needs --{flag}")
    if "predict_keypoints" in actions and (args.bbox_source == "detector") != bool(args.person_detector):
        ap.error("--bbox_source detector and --person_detector go together")
    if not os.path.isdir(args.data_dir):
        ap.error(f"--data_dir {args.data_dir!r} is not a directory")
    for act, res in run(args.data_dir, actions, matting_model_dir=args.matting_model_dir, sapiens_ckpt_path=args.sapiens_ckpt_path,
                        palette=args.palette, batch_size=args.batch_size, device_png=args.device_png, device_decode=args.device_decode,
                        person_detector=args.person_detector, bbox_source=args.bbox_source, bbox_thr=args.bbox_thr, nms_thr=args.nms_thr,
                        det_shape=args.det_shape, skeleton_from=args.skeleton_from, device_webp=args.device_webp):
        print(json.dumps({"action": act, "result": res}, default=str))
    return 0


if __name__ == "__main__":
    sys.exit(main())
