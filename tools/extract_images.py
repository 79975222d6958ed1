#!/usr/bin/env python
"""Rectify raw DNA-Rendering captures into ``images/{cam}/{frame}.webp`` (diffuman4d_amd/host/rectify.py): colour correction,
undistortion, area resize and crop on the GPU, with the argument names of the reference's scripts/download/extract_dnar_images.py
``extract_images``.

  python tools/extract_images.py --raw_images_dir RAW --cameras_json CAMS.json --out_images_dir DATA/SCENE/images
  python tools/extract_images.py --smc SCENE.smc --cameras_json CAMS.json --out_images_dir DATA/SCENE/images --device_decode

``--raw_images_dir`` holds ``{cam}/{frame}.*`` (encoded files); ``--smc`` reads the colour streams of an ``.smc`` file and needs h5py.
``--cameras_json``: ``{cam_label: {K, D, ccm, K_undist, H_undist, W_undist, H, W}}`` (DESIGN.md "Raw-capture rectification").  Prints one
JSON line of counts.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def _ints(text: str):
    return [int(p) for p in text.strip("()[] ").split(",") if p.strip()]


def raw_frames(raw_images_dir: str):
    """[(cam_label, frame_label, path)] of ``{cam}/{frame}.*`` under `raw_images_dir`, sorted."""
    out = []
    for cam in sorted(os.listdir(raw_images_dir)):
        sub = os.path.join(raw_images_dir, cam)
        if os.path.isdir(sub):
            out += [(cam, os.path.splitext(name)[0], os.path.join(sub, name)) for name in sorted(os.listdir(sub)) if not name.startswith(".")]
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--smc", default=None, help="an .smc file (needs h5py)")
    src.add_argument("--raw_images_dir", default=None, help="holds {cam}/{frame}.* encoded frames")
    ap.add_argument("--cameras_json", required=True, help="{cam: {K, D, ccm, K_undist, H_undist, W_undist, H, W}}")
    ap.add_argument("--out_images_dir", required=True, help="receives {cam}/{frame}{image_ext}")
    ap.add_argument("--image_ext", default=".webp")
    ap.add_argument("--image_quality", type=int, default=85)
    ap.add_argument("--batch_size", type=int, default=8)
    ap.add_argument("--num_workers", type=int, default=12, help="threads that read, decode and save (at most 16)")
    ap.add_argument("--gpu_ids", type=_ints, default=None, help="e.g. 0,1 (default: every device)")
    ap.add_argument("--skip_exists", action="store_true", help="keep an output file that exists and verifies (off by default here, as in this package's other tools: existing files are "
                         "overwritten; the function and the reference default to skipping)")
    ap.add_argument("--device_decode", action="store_true", help="decode baseline JPEG and 8-bit PNG sources on the GPU: the same files are written")
    args = ap.parse_args(argv)
    if args.batch_size < 1:
        ap.error("--batch_size must be at least 1")
    if not os.path.isfile(args.cameras_json):
        ap.error(f"--cameras_json {args.cameras_json}: no such file")
    from diffuman4d_amd.host import rectify
    if args.smc is not None:
        frames = rectify.SmcFrames(args.smc)
    else:
        if not os.path.isdir(args.raw_images_dir):
            ap.error(f"--raw_images_dir {args.raw_images_dir}: no such directory")
        frames = raw_frames(args.raw_images_dir)
    try:
        res = rectify.extract_images(frames, args.cameras_json, args.out_images_dir, args.image_ext, args.image_quality, args.skip_exists,
                                     args.num_workers, batch_size=args.batch_size, gpu_ids=args.gpu_ids, device_decode=args.device_decode)
    finally:
        if args.smc is not None:
            frames.release()
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
