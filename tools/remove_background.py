#!/usr/bin/env python
"""Predict per-view foreground masks with a matting network the caller names (diffuman4d_amd/host/matting.py), with the argument names
of the reference's scripts/preprocess/remove_background.py (the ``remove_background`` action of preprocess.sh) plus
``--matting_model_dir``.

  python tools/remove_background.py --images_dir DATA/SCENE/images --out_fmasks_dir DATA/SCENE/fmasks --matting_model_dir CKPT/BiRefNet

writes DATA/SCENE/fmasks/{camera}/{frame}.png, which tools/carve_visual_hull.py --fmasks_dir and tools/predict_keypoints.py --fmasks_dir
read, and prints one JSON line with counts.  The network is a local directory in the Hugging Face layout and is never downloaded:
``--model_name`` is accepted for the reference's sake, but only where it names such a directory.
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
    ap.add_argument("--images_dir", required=True, help="searched for **/*{image_ext}")
    ap.add_argument("--out_fmasks_dir", required=True, help="receives {camera}/{frame}{mask_ext}")
    ap.add_argument("--out_images_alpha_dir", default=None, help="receives {camera}/{frame}.png, the image with the mask as its alpha")
    ap.add_argument("--model_name", default=None, help="a local directory (a hub name is refused: nothing is downloaded)")
    ap.add_argument("--matting_model_dir", default=None, help="the same, under this package's name; takes precedence")
    ap.add_argument("--image_ext", default=".webp")
    ap.add_argument("--mask_ext", default=".png")
    ap.add_argument("--rotate_clockwise", type=int, default=0, choices=(0, 90, 180, 270))
    ap.add_argument("--batch_size", type=int, default=8)
    ap.add_argument("--num_workers", type=int, default=4, help="threads that decode images and write the PNG files (at most 16)")
    ap.add_argument("--skip_exists", action="store_true", help="skip a batch whose masks all exist and verify")
    ap.add_argument("--gpu_ids", type=_ints, default=None, help="e.g. 0,1 (default: every device)")
    ap.add_argument("--image_size", type=_ints, default=[1024, 1024], help="network input height,width")
    ap.add_argument("--device_png", action="store_true",
                    help="encode the mask and RGBA PNG files on the GPU (host/png.py): same pixels as the default route, other bytes")
    ap.add_argument("--device_decode", action="store_true",
                    help="decode baseline JPEG inputs on the GPU (host/jpegdec.py): the same files are written")
    args = ap.parse_args(argv)
    if len(args.image_size) != 2:
        ap.error("--image_size takes height,width")
    model = args.matting_model_dir or args.model_name
    if not model:
        ap.error("name the matting network: --matting_model_dir (a local directory)")
    from diffuman4d_amd.host import matting
    res = matting.remove_background(args.images_dir, args.out_fmasks_dir, args.out_images_alpha_dir, model, args.image_ext, args.mask_ext,
                                    args.rotate_clockwise, args.batch_size, args.num_workers, args.skip_exists, args.gpu_ids,
                                    image_size=tuple(args.image_size), device_png=args.device_png,
                                    **({"device_decode": True} if args.device_decode else {}))
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
