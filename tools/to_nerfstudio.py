#!/usr/bin/env python
"""Export a result directory for 4DGS reconstruction with nerfstudio (diffuman4d_amd/host/nerfstudio.py), with the argument names of the
reference's scripts/nerfstudio/diffuman4d_to_nerfstudio.py plus ``--matting_model_dir`` and ``--device_png``.

  python tools/to_nerfstudio.py --data_dir DATA/SCENE --result_dir RESULTS/SCENE --input_cameras 01,13,25,37 \\
      --matting_model_dir CKPT/BiRefNet [--device_png]

writes RESULTS/SCENE/transforms.json, transforms_input.json (with --input_cameras), sparse_pcd.ply, fmasks/{camera}/{frame}.png and
images_alpha/{camera}/{frame}.png, and prints one JSON line with counts.  The matting network is a local directory in the Hugging Face
layout and is never downloaded.  ``--device_png`` encodes the PNG files on the GPU: the same pixels as without it, other bytes.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def _labels(text: str):
    return [p.strip() for p in text.strip("()[] ").split(",") if p.strip()]


def _ints(text: str):
    return [int(p) for p in _labels(text)]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--data_dir", required=True, help="the scene: transforms.json and sparse_pcd.ply")
    ap.add_argument("--result_dir", required=True, help="the sampler's output directory: images/{camera}/{frame}.jpg")
    ap.add_argument("--input_cameras", type=_labels, default=None, help="camera labels of the input views, e.g. 01,13,25,37")
    ap.add_argument("--matting_model_dir", required=True, help="the matting network, a local directory (nothing is downloaded)")
    ap.add_argument("--device_png", action="store_true", help="encode the mask and RGBA PNG files on the GPU")
    ap.add_argument("--device_decode", action="store_true", help="decode the result JPEG files on the GPU (the same files are written)")
    ap.add_argument("--batch_size", type=int, default=4)
    ap.add_argument("--gpu_ids", type=_ints, default=None, help="e.g. 0,1 (default: every device)")
    ap.add_argument("--skip_exists", action="store_true", help="skip a batch whose masks all exist and verify")
    args = ap.parse_args(argv)
    from diffuman4d_amd.host.nerfstudio import diffuman4d_to_nerfstudio
    res = diffuman4d_to_nerfstudio(args.data_dir, args.result_dir, args.input_cameras, matting_model_dir=args.matting_model_dir,
                                   batch_size=args.batch_size, device_png=args.device_png, gpu_ids=args.gpu_ids, skip_exists=args.skip_exists,
                                   **({"device_decode": True} if args.device_decode else {}))
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
