"""The nerfstudio export of a result directory: the reference's ``to_nerfstudio`` step
(scripts/nerfstudio/diffuman4d_to_nerfstudio.py), the third default step of ``inference.py`` after sampling and evaluating.  It writes
what 4DGS reconstruction reads from the sampled views:

  * ``transforms.json`` / ``transforms_input.json`` (``results.write_nerfstudio_transforms``);
  * ``sparse_pcd.ply``, copied from the scene;
  * ``fmasks/{camera}/{frame}.png`` and ``images_alpha/{camera}/{frame}.png`` of every result image
    (``matting.remove_background`` over ``{result_dir}/images/**/*.jpg``).

The matting network is the caller's: a local directory or a callable.  It is never downloaded.
"""
from __future__ import annotations

import logging
import os
import shutil
from typing import Callable, Optional, Sequence

from .matting import load_matting_model, remove_background
from .results import write_nerfstudio_transforms

log = logging.getLogger(__name__)


def diffuman4d_to_nerfstudio(data_dir: str, result_dir: str, input_cameras: Optional[Sequence[str]] = None, *,
                             matting_model_dir: Optional[str] = None, matting_model: Optional[Callable] = None, batch_size: int = 4,
                             device_png: bool = False, gpu_ids: Optional[Sequence[int]] = None, skip_exists: bool = False,
                             device_decode: bool = False) -> dict:
    """`data_dir` (the scene: ``transforms.json``, ``sparse_pcd.ply``) + `result_dir` (``images/{camera}/{frame}.jpg``) -> the camera
    files, the point cloud, the foreground masks and the RGBA images in `result_dir`; the reference's arguments in its names and order.

    Where this differs from the reference:
      * it hard-codes a hub name for the matting network; here the network is `matting_model_dir` (a local directory in the Hugging
        Face layout, ``matting.load_matting_model``) or `matting_model` (any callable, ``matting.remove_background``).  A name that is
        not a local directory raises FileNotFoundError before anything is written;
      * it raises NameError when `input_cameras` is None; here ``transforms_input.json`` is simply not written in that case.
    device_png: encode the mask and RGBA PNG files on the device (``remove_background(device_png=True)``): same pixels, other bytes.
    device_decode: decode the result JPEG files on the device instead of in Pillow (``remove_background(device_decode=True)``): the
    same files are written.
    -> the counts of ``remove_background``."""
    if matting_model is None:
        if not matting_model_dir:
            raise ValueError("name the matting network: matting_model_dir (a local directory) or matting_model (a callable)")
        if not os.path.isdir(matting_model_dir):
            load_matting_model(matting_model_dir, "cpu")  # raises FileNotFoundError: a hub name is refused before anything is written
    write_nerfstudio_transforms(data_dir, result_dir, input_cameras)
    log.info("Saved nerfstudio cameras to %s/transforms.json%s", result_dir, "" if input_cameras is None else " and transforms_input.json")
    shutil.copy(f"{data_dir}/sparse_pcd.ply", f"{result_dir}/sparse_pcd.ply")
    log.info("Saved point cloud to %s/sparse_pcd.ply", result_dir)
    counts = remove_background(images_dir=f"{result_dir}/images", out_fmasks_dir=f"{result_dir}/fmasks",
                               out_images_alpha_dir=f"{result_dir}/images_alpha", model_name=matting_model_dir, image_ext=".jpg",
                               mask_ext=".png", rotate_clockwise=0, batch_size=batch_size, skip_exists=skip_exists, gpu_ids=gpu_ids,
                               matting_model=matting_model, device_png=device_png, **({"device_decode": True} if device_decode else {}))
    log.info("Saved foreground masks to %s/fmasks", result_dir)
    return counts
