#!/usr/bin/env python
"""Draw a scene's skeleton maps from its 2-D keypoints (diffuman4d_amd/host/skeleton.py), with the argument names of the reference's
scripts/preprocess/draw_skeleton.py (the ``draw_skeleton`` action of preprocess.sh) plus ``--palette``.

  python tools/draw_skeleton.py --kp2d_dir DATA/SCENE/poses_2d --out_kpmap_dir DATA/SCENE/skeletons --palette palette.json

reads DATA/SCENE/poses_2d/{camera}/{frame}.json, writes DATA/SCENE/skeletons/{camera}/{frame}.webp and prints one JSON line with
counts.  With ``--kp3d_dir DATA/SCENE/poses_3d --camera_path DATA/SCENE/transforms.json`` the maps come straight from the 3-D
keypoints, projected into the cameras on the device: no poses_2d directory is read (``--kp2d_dir`` is then not needed), and the files
are those drawn from the poses_2d that triangulate_skeleton writes.  With ``--device_webp`` the maps are encoded on the device as
lossless WebP and only the files' bytes come down.  The palette (keypoint colours, links, the colour of the two "x" links) is not part of this package: see
diffuman4d_amd.host.skeleton.load_palette for the file's layout.
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
    ap.add_argument("--kp2d_dir", default=None, help="poses_2d/{camera}/{frame}.json")
    ap.add_argument("--kp3d_dir", default=None, help="poses_3d/{frame}.json: draw from the 3-D keypoints instead (with --camera_path)")
    ap.add_argument("--camera_path", default=None, help="with --kp3d_dir: the scene's nerfstudio transforms.json")
    ap.add_argument("--intri_scale", type=float, default=None, help="with --kp3d_dir: scale of the intrinsics, as triangulate_skeleton takes it")
    ap.add_argument("--out_kpmap_dir", required=True, help="receives {camera}/{frame}{image_ext}")
    ap.add_argument("--kp2d_score_dir", default=None, help="files of the same names whose keypoint_scores replace the frames' own")
    ap.add_argument("--kp2d_canvas_shape", type=_numbers(int, 2), default=[1024, 1024], help="h,w of the image the keypoints refer to")
    ap.add_argument("--out_kpmap_shape", type=_numbers(int, 2), default=[1024, 1024], help="h,w of the maps (the longer side 256 .. 8192)")
    ap.add_argument("--spa_labels", type=_numbers(int), default=None, help="camera labels, e.g. 0,4,8 (default: the listing of kp2d_dir)")
    ap.add_argument("--tem_labels", type=_numbers(int), default=None, help="frame labels (default: the listing of the first camera)")
    ap.add_argument("--image_ext", default=".webp")
    ap.add_argument("--image_quality", type=int, default=85)
    ap.add_argument("--num_workers", type=int, default=16, help="threads that read the JSON files and encode the images (at most 16)")
    ap.add_argument("--skip_exists", action="store_true", help="leave files that exist and that Pillow verifies")
    ap.add_argument("--palette", required=True, help="JSON file with keypoint_colors, links and x_link_color")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--device_webp", action="store_true",
                    help="encode the maps on the GPU as lossless WebP: the files decode to exactly the maps; --image_ext must be .webp, --image_quality is ignored")
    args = ap.parse_args(argv)
    if (args.kp3d_dir is None) != (args.camera_path is None):
        ap.error("--kp3d_dir and --camera_path go together")
    if args.kp3d_dir is None and args.kp2d_dir is None:
        ap.error("one of --kp2d_dir and --kp3d_dir is required")
    from diffuman4d_amd.host import skeleton
    res = skeleton.draw_skeleton(args.kp2d_dir, args.out_kpmap_dir, kp2d_score_dir=args.kp2d_score_dir,
                                 kp2d_canvas_shape=tuple(args.kp2d_canvas_shape), out_kpmap_shape=tuple(args.out_kpmap_shape),
                                 spa_labels=args.spa_labels, tem_labels=args.tem_labels, image_ext=args.image_ext,
                                 image_quality=args.image_quality, num_workers=args.num_workers, skip_exists=args.skip_exists,
                                 palette=args.palette, device=args.device, kp3d_dir=args.kp3d_dir, camera_path=args.camera_path,
                                 intri_scale=args.intri_scale, device_webp=args.device_webp)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
