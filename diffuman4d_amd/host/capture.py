"""``SpaTemDataset`` for captured scenes: nerfstudio cameras, Pillow decode on the host, crop + resize on the device.

Same constructor keywords and ``get_item`` dict as the reference's dataset (``src/data/spatem_dataset.py``), built from its
behaviour.  What the reference does per frame -- decode, crop to the mask's square box, Pillow's bicubic resize of image, mask and
skeleton, ``to_tensor``, ``* 2 - 1`` and the white-background blend -- is split here:

  * host, in a thread pool (Pillow releases the GIL while it decodes): decode, the mask's bounding box and the crop box, the
    ``has_gt_target=False`` masks, the checks, and Pillow's coefficient tables (float64, once per distinct size pair per task);
  * device, two launches per task (``dm4d_capture_crop_resize_f32``): the resize itself, bit-exact with Pillow, and the fp32 epilogue.

Every task's uint8 planes, tables and frame descriptors go into one pinned staging buffer and up in one copy.  ``pixel_values``
and ``skeletons`` come back as fp32 NCHW tensors on ``device``; cameras, Pluecker maps and masks stay on the host.

Offsets, the pinned buffer, its filling and the table / descriptor pack are host/staging.py's.

``skeleton_source="kp2d"`` (opt-in) reads no skeleton image: every frame's map is drawn on the device from its ``poses_2d`` keypoint
file (host/skeleton.py, ``dm4d_skeleton_draw_u8``) straight into the device staging buffer, and for ``has_gt_target=False`` targets
``dm4d_skeleton_box_mask_u8`` derives the box mask and the bounding box there as well; only the boxes (16 bytes per frame) come back.
``skeleton_source="kp3d"`` (opt-in) needs no ``poses_2d`` files either: the maps are projected from ``poses_3d`` into the scene's cameras,
planned and drawn on the device (``dm4d_skeleton_plan_kp3d``, ``dm4d_skeleton_draw_planned_u8``); the rest is the "kp2d" route's code.

``device_decode=True`` (opt-in, either skeleton source) moves the decode of JPEG and PNG files to the device as well: the pool reads
and probes the files (``_read``), host/jpegdec.py and host/pngdec.py decode them into the device staging buffer, and what the host
route takes from decoded pixels -- the crop box, the empty and 2 % checks, the ``has_gt_target=False`` box mask -- comes from
``dm4d_capture_plane_stats_u8`` (40 bytes per plane come back) and ``dm4d_capture_fill_rects_u8`` (``_settle_frames``,
``_resize_on_device_decoded``).  Files the decoders do not take (WebP, progressive JPEG, ...) are decoded by Pillow as before, inside
the same call.  The sample and every exception are the flag-off call's.

``device_cache=True`` (opt-in, any route) keeps every resized frame on the device as a *cell* of 8 bytes per pixel
(host/capture_cache.py, ``dm4d_capture_crop_resize_packed_u8``): a job visits each grid cell several times, and ``get_item`` then runs
the route above on the frames it has not seen only (``_load``; its ``ops.capture_crop_resize`` call is the one hook, ``_crop_resize``)
and builds all rows of the sample from cells with one ``dm4d_capture_unpack_cells_f32`` launch (``_load_cached``).
"""
from __future__ import annotations

import contextlib
import json
import logging
import math
import os
import threading
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from PIL import Image

from . import lib as _l
from . import ops
from .capture_cache import CellCache
from .codec import StagedFile, decode_staged, probe_file
from .dataset import plucker_maps, relative_poses
from .staging import Layout, fill, pack_meta, pinned, write_meta
from .resample import PRECISION_BITS, TableSet, bicubic_table  # noqa: F401  (tests and tools import the first and the last from here)

log = logging.getLogger(__name__)

FIELDS = ops.CAPTURE_FIELDS  # int64 fields of one frame descriptor: an alias of the one mirror in host/lib.py, not a second copy


# -- cameras ----------------------------------------------------------------------------------------------------------------------
def read_cameras(camera_path: str, normalize_scene: bool = True) -> Dict[str, Dict]:
    """nerfstudio ``transforms.json`` -> {camera_label: {K, pose, height, width}} with OpenCV axes and normalised positions, in the
    reference's float32 arithmetic (data/utils/camera_parser.py).  normalize_scene=False leaves the positions as the file gives them
    (parse_cameras(..., normalize_scene=False), what skeleton triangulation asks for)."""
    if os.path.isdir(camera_path) or camera_path.endswith(".yml"):
        raise NotImplementedError(f"EasyVolcap cameras are not supported ({camera_path}): give a nerfstudio transforms.json")
    if not camera_path.endswith(".json"):
        raise ValueError(f"camera file must be a nerfstudio transforms.json: {camera_path}")
    with open(camera_path) as f:
        tfs = json.load(f)
    labels, Ks, hws, poses = [], [], [], []
    for fr in tfs["frames"]:
        src = fr if all(k in fr for k in ("fl_x", "fl_y", "cx", "cy")) else tfs  # per-frame intrinsics, else the global ones
        Ks.append(torch.tensor([src["fl_x"], 0, src["cx"], 0, src["fl_y"], src["cy"], 0, 0, 1]).reshape(3, 3))
        hws.append((fr["h"], fr["w"]))
        pose = torch.tensor(fr["transform_matrix"])
        pose[:3, 1:3] *= -1  # OpenGL -> OpenCV camera axes
        poses.append(pose)
        labels.append(fr["camera_label"])
    poses = torch.stack(poses)
    # Scene normalisation.  The reference looks for f"{camera_path}/scene_norm.json", a path UNDER the JSON file, which therefore
    # never exists: its centre and scale always come from the bounding box of the camera positions, and so do ours.
    if normalize_scene:
        pos = poses[:, :3, 3]
        lo, hi = torch.min(pos, dim=0).values, torch.max(pos, dim=0).values
        center, scale = (lo + hi) / 2, 1 / torch.linalg.norm(hi - lo)
        poses[:, :3, 3] = (poses[:, :3, 3] - center) * scale
    return {lab: {"K": K, "pose": p, "height": hw[0], "width": hw[1]} for lab, K, hw, p in zip(labels, Ks, hws, poses)}


# -- masks and crops --------------------------------------------------------------------------------------------------------------
def mask_bbox(nonzero: np.ndarray) -> Optional[Tuple[int, int, int, int]]:
    """(xmin, ymin, xmax, ymax) one pixel outside the nonzero pixels of a [h, w] bool map, or None when there are none."""
    rows, cols = np.flatnonzero(nonzero.any(axis=1)), np.flatnonzero(nonzero.any(axis=0))
    if rows.size == 0 or cols.size == 0:
        return None
    return int(cols[0]) - 1, int(rows[0]) - 1, int(cols[-1]) + 1, int(rows[-1]) + 1


def crop_box(mask: np.ndarray, path: str = "") -> List[int]:
    """The square crop around the mask (crop_utils.py mask_crop_aspect_ratio with its defaults) -> [top, left, height, width, h, w];
    it may extend past the image.  The reference's padding is torch.randint(0, 1), always 0: no draw is made here."""
    h, w = mask.shape
    box = mask_bbox(mask != 0)
    if box is None:
        raise ValueError(f"foreground mask is empty: {path}")
    return _crop_from_bbox(box, h, w)


def _crop_from_bbox(box: Tuple[int, int, int, int], h: int, w: int) -> List[int]:
    """crop_box from the mask's (xmin, ymin, xmax, ymax) of mask_bbox and its size."""
    xmin, ymin, xmax, ymax = box
    xc, yc = (xmin + xmax) / 2, (ymin + ymax) / 2
    size = max(2 * max(yc - ymin, ymax - yc, (xc - xmin) * 1.0, (xmax - xc) * 1.0), 0.7 * h)
    cw = int(size / 1.0)
    x0, y0 = math.floor(xc - cw / 2), math.floor(yc - size / 2)
    x1, y1 = math.ceil(xc + cw / 2), math.ceil(yc + size / 2)
    return [y0, x0, y1 - y0, x1 - x0, h, w]


def skeleton_mask(skel: np.ndarray, path: str = "") -> np.ndarray:
    """crop_utils.py skeleton_to_mask in float32: channel mean of to_tensor, the padded box of its nonzero pixels set to 1, then
    mul(255) and a truncating byte() (to_pil_image).  [h, w, 3] uint8 -> [h, w] uint8."""
    h, w = skel.shape[:2]
    py, px = int(h * 0.03), int(w * 0.03)
    pt = int(py * 3)
    m = torch.from_numpy(np.array(skel)).permute(2, 0, 1).contiguous().to(torch.float32).div(255).mean(dim=0)
    box = mask_bbox(m.numpy() != 0)
    if box is None:
        raise ValueError(f"skeleton is empty, no mask can be made from it: {path}")
    xmin, ymin, xmax, ymax = box
    xmin, ymin, xmax, ymax = max(xmin - px, 0), max(ymin - pt, 0), min(xmax + px, w), min(ymax + py, h)
    m[ymin:ymax, xmin:xmax] = 1.0
    return m.mul(255).byte().numpy()


def skeleton_mask_pads(h: int, w: int) -> Tuple[int, int, int]:
    """skeleton_mask's paddings for an [h, w] map -> (pad_top, pad_bottom, pad_x), as dm4d_skeleton_box_mask_u8 takes them."""
    py, px = int(h * 0.03), int(w * 0.03)
    return int(py * 3), py, px


def skeleton_mask_rect(box: Sequence[int], h: int, w: int) -> Tuple[int, int, int, int]:
    """skeleton_mask is a filled rectangle: from (first column, first row, last column, last row) of the pixels with a non-zero
    channel -> (c0, r0, c1, r1), the mask is 255 on rows r0 .. r1 - 1 and columns c0 .. c1 - 1 and 0 elsewhere.  (The float32 channel
    mean is non-zero exactly where a channel is, and mul(255).byte() of a mean outside the box, where every channel is 0, is 0.)"""
    fc, fr, lc, lr = (int(v) for v in box)
    pt, py, px = skeleton_mask_pads(h, w)
    return max(fc - 1 - px, 0), max(fr - 1 - pt, 0), min(lc + 1 + px, w), min(lr + 1 + py, h)


def _sum_mean_at_most(total: int, size: int, limit: float) -> Optional[bool]:
    """_mask_mean_at_most from the sum of the mask's `size` bytes alone, or None where the exact mean is so close to `limit` that the
    float32 mean decides."""
    exact = float(total) / (255.0 * size)
    return exact <= limit if abs(exact - limit) > 1e-4 else None


def _mask_mean_at_most(mask: np.ndarray, limit: float) -> bool:
    """TF.to_tensor(mask).mean() <= limit, decided exactly: the float32 mean only where the exact mean is close to `limit`."""
    decided = _sum_mean_at_most(int(mask.sum(dtype=np.int64)), mask.size, limit)
    if decided is not None:
        return decided
    return bool(torch.from_numpy(mask).to(torch.float32).div(255).mean() <= limit)


def _open(path: str, mode: str) -> np.ndarray:
    with Image.open(path) as im:
        if im.mode != mode:
            raise ValueError(f"{path}: image mode {im.mode!r}, expected {mode!r} (no conversion is made: it would change values)")
        return np.asarray(im)


# -- device_decode=True: files that may decode on the device, and the checks that then wait for their statistics ----------------------
def _read(path: str, mode: str):
    """_open for a frame whose files may decode on the device: a JPEG or PNG file the decoders take (host/jpegdec.py, host/pngdec.py
    ``probe``) -> a codec.StagedFile, its mode checked on the plan with _open's error; any other file -> _open's pixels, as ever."""
    from . import jpegdec, pngdec
    f = probe_file(path, (jpegdec, pngdec))
    if f is None:
        return _open(path, mode)
    if f.mode != mode:
        raise ValueError(f"{path}: image mode {f.mode!r}, expected {mode!r} (no conversion is made: it would change values)")
    return f


def _hw(a) -> Tuple[int, int]:
    """(h, w) of a decoded plane or of a StagedFile."""
    return (a.h, a.w) if isinstance(a, StagedFile) else (int(a.shape[0]), int(a.shape[1]))


def _settle_frame(fr: Dict, row: Sequence[int]) -> None:
    """What _load_frame / _load_frame_kp2d do once a frame's pixels are known, from `row` = {first column, first row, last column, last
    row, sum} (dm4d_capture_plane_stats_u8) of the frame's mask or, for a has_gt_target=False target, of its skeleton map -- in their
    order and with their errors: the empty check, then fr["crop"] (and fr["rect"], the target's mask rectangle), the size assertion,
    the 2 % assertion."""
    fc, fr_, lc, lr, total = (int(v) for v in row)
    if fr["mask"] is None:  # the skeleton serves as image, its box as mask
        if lc < 0:
            raise ValueError(f"skeleton is empty, no mask can be made from it: {fr['path']}")
        h, w = fr["hw"]
        c0, r0, c1, r1 = fr["rect"] = skeleton_mask_rect((fc, fr_, lc, lr), h, w)
        fr["crop"] = _crop_from_bbox((c0 - 1, r0 - 1, c1, r1), h, w)  # mask_bbox of the rectangle
        return
    if lc < 0:
        raise ValueError(f"foreground mask is empty: {fr['img_path']}")
    h, w = _hw(fr["mask"])
    fr["crop"] = _crop_from_bbox((fc - 1, fr_ - 1, lc + 1, lr + 1), h, w)
    isz, msz, ssz = ((s[1], s[0]) for s in (_hw(fr["img"]), (h, w), fr["hw"]))  # PIL's (w, h)
    if not (isz == msz == ssz):
        raise AssertionError(f"Error: image size: {isz} != fmask size: {msz} != skeleton size: {ssz}")
    if fr["check"]:
        decided = _sum_mean_at_most(total, h * w, 0.02)
        if decided is None:  # too close to the limit for the sum to say: this one mask is decoded on the host
            mask = _open(fr["mask"].path, "L") if isinstance(fr["mask"], StagedFile) else fr["mask"]
            decided = _mask_mean_at_most(mask, 0.02)
        if decided:
            raise AssertionError("Error: foreground mask < 2%. Please check the data.")


def _settle_frames(frames: List, rows: Dict[int, Sequence[int]]) -> None:
    """_settle_frame over a task's frames in label order, so that the error raised is the first bad frame's.  An entry of `frames`
    that is an exception is a frame whose files could not be read: it is raised when its turn comes."""
    for i, fr in enumerate(frames):
        if isinstance(fr, BaseException):
            raise fr
        _settle_frame(fr, rows[i])


def _intrinsic(K: torch.Tensor, crop: List[int], height: int) -> torch.Tensor:
    """K of the cropped and resized view (spatem_dataset.py transform_intrinsic): float32, the scale multiplied as a scalar."""
    top, left, ch = crop[0], crop[1], crop[2]
    K = K.clone()
    K[0, 2] = K[0, 2] - left
    K[1, 2] = K[1, 2] - top
    K = K * (height / ch)
    K[2, 2] = 1.0
    return K


def _cell_rows(rows: List[List[int]], device: torch.device) -> Tuple[torch.Tensor, torch.Tensor]:
    """Cell descriptors (include/dm4d.h) -> (their int64 [n, CAPTURE_CELL_FIELDS] host copy in a pinned buffer, the copy on `device`,
    queued on the current stream by staging.pack_meta: nothing waits for it).  The caller keeps both until it has synchronised."""
    desc = np.asarray(rows, dtype=np.int64).reshape(-1, _l.CAPTURE_CELL_FIELDS)
    dev, host, _, _, off = pack_meta(None, desc, device)
    view = lambda t: t[off: off + desc.nbytes].view(torch.int64).reshape(desc.shape)  # noqa: E731
    return view(host), view(dev)


SKELETON_SOURCES = ("files", "kp2d", "kp3d")
KP2D_PATH_PAT = "{data_dir}/{scene_label}/poses_2d/{spa_label}/{tem_label}.json"
KP3D_PATH_PAT = "{data_dir}/{scene_label}/poses_3d/{tem_label}.json"


class SpaTemDataset:
    """Captured-scene dataset with the reference's ``SpaTemDataset`` keywords and ``get_item`` contract.

    Extension keywords: ``plucker`` ("host": full-resolution fp32 Pluecker maps, as the reference; "cameras": ``None`` and the
    pipeline evaluates the rays on the device, as ``SyntheticSpaTemDataset``), ``device`` (where ``pixel_values`` / ``skeletons``
    land; default: the calling thread's current HIP device), ``decode_threads`` (Pillow decode pool).

    ``skeleton_source``: "files" reads ``skeleton_path_pat`` (the reference's route); "kp2d" draws every skeleton map on the device
    from ``kp2d_path_pat`` (and the score override ``kp2d_score_path_pat``, the reference's ``draw_skeleton(kp2d_score_dir=...)``) with
    ``palette`` (a path or a Palette, as ``skeleton.load_palette`` takes it), exactly as ``skeleton.draw_skeleton_maps([kp2d_path],
    [score_path], kp2d_canvas_shape or the camera's (height, width), (h, w), palette=palette)[0]`` with (h, w) the decoded image's size
    or, for a frame that loads none, the camera's.  No skeleton file is read and no map crosses PCIe.  The result equals the file
    route's on skeleton files that hold those maps losslessly; it differs from it on lossy files by exactly the codec's loss.
    "kp3d" needs no ``poses_2d`` directory either: a task reads each distinct frame's ``kp3d_path_pat`` file (``poses_3d``) once, and
    the maps are projected into the scene's cameras (``triang.scene_cameras``, uploaded once per scene), planned and drawn on the device
    (``skeleton.plan_and_draw``); ``kp2d_score_path_pat``, ``kp2d_canvas_shape`` and ``palette`` as for "kp2d".  Sample and exceptions are
    those of "kp2d" on the ``poses_2d`` files ``triang.triangulate_skeleton`` writes from the same poses and cameras.

    ``device_decode``: baseline JPEG and 8-bit PNG files (images, masks, skeleton files) are decoded on the device instead of by
    Pillow in the pool; needs a HIP device (Dm4dError otherwise).  ``get_item`` returns and raises what it does without the flag;
    ``decode_stats`` ("device", "pillow", "bytes_uploaded", as ``codec.decode_batch`` counts them) is added to by every call.

    ``device_cache``: every frame ``get_item`` resizes stays on its device as a cell of ``height * width * 8`` bytes, up to
    ``device_cache_bytes`` per device (no eviction: cells beyond the budget are loaded again each time), keyed by (device index,
    scene_label, spa_label, tem_label, the camera is an input camera).  A later call that needs the frame opens none of its files;
    ``decode_stats`` counts the files actually decoded.  ``get_item`` returns and raises what it does without the flag.  Files that
    change on disk during a job are NOT noticed: call ``clear_device_cache()`` (between calls, not during one) to forget every cell.
    ``cache_stats``: "hits", "misses", "unretained" (cells the budget did not cover), "cells" and "bytes" held, over all devices."""

    def __init__(self, data_dir: str, camera_path_pat: str = "{data_dir}/{scene_label}/transforms.json",
                 image_path_pat: str = "{data_dir}/{scene_label}/images/{spa_label}/{tem_label}.webp",
                 fmask_path_pat: str = "{data_dir}/{scene_label}/fmasks/{spa_label}/{tem_label}.png",
                 skeleton_path_pat: str = "{data_dir}/{scene_label}/skeletons/{spa_label}/{tem_label}.webp",
                 scene_label: Optional[str] = None, height: int = 1024, width: int = 1024, has_gt_target: bool = True,
                 plucker: str = "host", device=None, decode_threads: int = 8, skeleton_source: str = "files",
                 kp2d_path_pat: str = KP2D_PATH_PAT, kp2d_score_path_pat: Optional[str] = None,
                 kp2d_canvas_shape: Optional[Tuple[int, int]] = None, kp3d_path_pat: str = KP3D_PATH_PAT, *, device_cache: bool = False,
                 device_cache_bytes: int = 16 << 30, palette=None, device_decode: bool = False):
        if plucker not in ("host", "cameras"):
            raise ValueError("plucker must be 'host' or 'cameras'")
        self.device_cache, self.device_cache_bytes = bool(device_cache), int(device_cache_bytes)
        if self.device_cache_bytes < 0:
            raise ValueError(f"device_cache_bytes must not be negative, got {device_cache_bytes}")
        self._caches: Dict[torch.device, CellCache] = {}  # device_cache=True: one per device, created when first asked for
        self.device_decode = bool(device_decode)
        if self.device_decode:  # there is no CPU path: the planes are decoded where the resize reads them
            _l.hip_device("cuda" if device is None else device, "SpaTemDataset(device_decode=True)")
        self.decode_stats = {"device": 0, "pillow": 0, "bytes_uploaded": 0}  # device_decode=True: added to by every get_item
        self._stats_lock = threading.Lock()
        if skeleton_source not in SKELETON_SOURCES:
            raise ValueError(f"skeleton_source must be one of {SKELETON_SOURCES}, got {skeleton_source!r}")
        self.skeleton_source, self.kp2d_path_pat, self.kp2d_score_path_pat = skeleton_source, kp2d_path_pat, kp2d_score_path_pat
        self.kp2d_canvas_shape = None if kp2d_canvas_shape is None else tuple(int(v) for v in kp2d_canvas_shape)
        self.kp3d_path_pat = kp3d_path_pat
        self.palette = self._plan_tables = None
        self._drawn = skeleton_source in ("kp2d", "kp3d")  # the maps are drawn on the device; "kp3d": planned there as well
        self._scene_cams: Dict = {}                         # "kp3d": (scene_label, device) -> (camera labels, K and T on the device)
        if self._drawn:
            from . import skeleton as _sk  # here, not at the top: host/skeleton.py imports host/triang.py, which imports this module
            if palette is None:
                raise ValueError(f"skeleton_source={skeleton_source!r} needs palette=: a path or a Palette, as skeleton.load_palette takes it (no colour "
                                 f"or link table is part of this package); {_sk.PALETTE_HELP}")
            if self.kp2d_canvas_shape is not None and (len(self.kp2d_canvas_shape) != 2 or min(self.kp2d_canvas_shape) < 1):
                raise ValueError(f"kp2d_canvas_shape must be (height, width), got {kp2d_canvas_shape!r}")
            self._sk, self.palette = _sk, _sk.load_palette(palette)
            if skeleton_source == "kp3d":
                self._plan_tables = _sk.plan_tables(self.palette)
        if width % 4 != 0:
            raise ValueError(f"width must be a multiple of 4 (dm4d_capture_crop_resize_f32), got {width}")
        self.data_dir = os.path.expandvars(data_dir) if "$" in data_dir else data_dir
        self.camera_path_pat, self.image_path_pat = camera_path_pat, image_path_pat
        self.fmask_path_pat, self.skeleton_path_pat = fmask_path_pat, skeleton_path_pat
        self.scene_label = "" if scene_label is None else scene_label
        self.height, self.width, self.has_gt_target = height, width, has_gt_target
        self.plucker, self.device, self.decode_threads = plucker, device, max(1, int(decode_threads))
        camera_path = self.camera_path_pat.format(data_dir=self.data_dir, scene_label=self.scene_label)
        self.cameras = {self.scene_label: read_cameras(camera_path)}
        self._pool = ThreadPoolExecutor(max_workers=self.decode_threads, thread_name_prefix="dm4d-decode")
        self._tls = threading.local()

    def get_file_path(self, pat: str, scene_label: str, spa_label: str, tem_label: str) -> str:
        return pat.format(data_dir=self.data_dir, scene_label=scene_label, spa_label=spa_label, tem_label=tem_label)

    def nearest_input_camera(self, cam: int, input_cams: Sequence[int]) -> int:
        """Integer-label form of the temporal conditioning-camera choice (runner.DistributedSamplingRunner asks for it)."""
        labels = [f"{c:02d}" for c in input_cams]
        return int(self._nearest(self.cameras[self.scene_label], f"{cam:02d}", labels))

    @staticmethod
    def _nearest(cameras: Dict, target: str, inputs: Sequence[str]) -> str:
        """The input camera nearest to `target`: distances between normalised absolute positions (before relative poses)."""
        pos = torch.stack([cameras[target]["pose"]] + [cameras[c]["pose"] for c in inputs])[:, :3, 3]
        return inputs[torch.argmin(torch.norm(pos[1:] - pos[:1], dim=1)).item()]

    # -- host half of one frame ----------------------------------------------------------------------------------------------
    def _load_frame(self, label, input_spa_labels) -> Dict:
        scene_label, spa, tem = label
        skel_path = self.get_file_path(self.skeleton_path_pat, scene_label, spa, tem)
        skel = _open(skel_path, "RGB")
        if not self.has_gt_target and spa not in input_spa_labels:  # the skeleton serves as image, its box as mask
            img, img_path, mask = None, skel_path, skeleton_mask(skel, skel_path)
        else:
            img_path = self.get_file_path(self.image_path_pat, scene_label, spa, tem)
            fmask_path = self.get_file_path(self.fmask_path_pat, scene_label, spa, tem)
            img, mask = _open(img_path, "RGB"), _open(fmask_path, "L")
        crop = crop_box(mask, img_path)
        size = lambda a: (a.shape[1], a.shape[0])  # PIL's (w, h)
        isz = size(skel if img is None else img)
        if not (isz == size(mask) == size(skel)):
            raise AssertionError(f"Error: image size: {isz} != fmask size: {size(mask)} != skeleton size: {size(skel)}")
        if self.has_gt_target and spa in input_spa_labels and _mask_mean_at_most(mask, 0.02):
            raise AssertionError("Error: foreground mask < 2%. Please check the data.")
        return {"img": img, "mask": mask, "skel": skel, "crop": crop}

    # -- skeleton_source="kp2d": the host half of one frame -------------------------------------------------------------------
    def _load_frame_kp2d(self, label, input_spa_labels) -> Dict:
        """As _load_frame, without a skeleton image: the frame's draw plan instead.  A has_gt_target=False target has no mask and
        no crop yet: both come from its map on the device (_resize_on_device_kp2d)."""
        scene_label, spa, tem = label
        sk, cam = self._sk, self.cameras[scene_label][spa]
        kp_path = self.get_file_path(self.kp2d_path_pat, scene_label, spa, tem)
        inst = sk._read_instance(kp_path)
        score = None if self.kp2d_score_path_pat is None else sk._read_instance(self.get_file_path(self.kp2d_score_path_pat, scene_label, spa, tem))
        if not self.has_gt_target and spa not in input_spa_labels:
            img, mask, img_path, hw = None, None, kp_path, (int(cam["height"]), int(cam["width"]))
        else:
            img_path = self.get_file_path(self.image_path_pat, scene_label, spa, tem)
            fmask_path = self.get_file_path(self.fmask_path_pat, scene_label, spa, tem)
            img, mask = _open(img_path, "RGB"), _open(fmask_path, "L")
            hw = img.shape[:2]
        sk._check_out_shape(hw)
        canvas = self.kp2d_canvas_shape or (int(cam["height"]), int(cam["width"]))
        plan = sk.plan_draw_calls(inst, score, (canvas, hw), self.palette)
        fr = {"img": img, "mask": mask, "plan": plan, "crop": None, "path": kp_path}
        if mask is not None:
            fr["crop"] = crop_box(mask, img_path)
            size = lambda a: (a.shape[1], a.shape[0])  # PIL's (w, h)
            if not (size(img) == size(mask) == plan.out_size):
                raise AssertionError(f"Error: image size: {size(img)} != fmask size: {size(mask)} != skeleton size: {plan.out_size}")
            if self.has_gt_target and spa in input_spa_labels and _mask_mean_at_most(mask, 0.02):
                raise AssertionError("Error: foreground mask < 2%. Please check the data.")
        return fr

    # -- skeleton_source="kp3d": the scene's cameras, a task's poses, the host half of one frame ---------------------------------------
    def _cameras_on_device(self, scene_label: str, device: torch.device):
        """(camera labels, K fp64 [m, 3, 3], T fp64 [m, 4, 4] on `device`) of the scene as triangulate_skeleton builds them
        (triang.scene_cameras: not normalised, float32 inverse), uploaded once per scene and device."""
        key = (scene_label, str(device))
        with self._stats_lock:
            if key not in self._scene_cams:
                from . import triang
                labels = sorted(self.cameras[scene_label])
                Ks, Ts = triang.scene_cameras(self.camera_path_pat.format(data_dir=self.data_dir, scene_label=scene_label), labels)
                self._scene_cams[key] = (labels, torch.from_numpy(Ks).to(device), torch.from_numpy(Ts).to(device))
            return self._scene_cams[key]

    def _read_poses(self, labels) -> Dict:
        """{(scene_label, tem_label): fp64 [k, 3] | the exception reading raised} for the distinct frames of a task: one read each."""
        keys = list(dict.fromkeys((scene_label, tem) for scene_label, _, tem in labels))

        def read(key):
            try:
                return self._sk.read_kp3d(self.get_file_path(self.kp3d_path_pat, key[0], "", key[1]))
            except Exception as e:  # noqa: BLE001  (raised when the first frame that needs the file has its turn)
                return e
        return dict(zip(keys, self._pool.map(read, keys)))

    def _kp3d_pose_and_score(self, label, poses: Dict):
        """The frame's pose (what reading it raised is raised here, at the frame's turn) and its score override, read as "kp2d" reads
        its two keypoint files: before the images."""
        scene_label, spa, tem = label
        if isinstance(poses[scene_label, tem], BaseException):
            raise poses[scene_label, tem]
        score = None
        if self.kp2d_score_path_pat is not None:
            score = self._sk._read_scores(self.get_file_path(self.kp2d_score_path_pat, scene_label, spa, tem))
        return poses[scene_label, tem], score

    def _kp3d_job(self, kp3d: np.ndarray, score, canvas, hw):
        """What plan_draw_calls checks before it looks at a keypoint, with its errors, -> the frame's skeleton.Kp3dJob (frame and camera
        are indices that _kp3d_draw fills in)."""
        if len(self.palette.keypoint_colors) != len(kp3d):
            raise ValueError(f"the length of kpt_color ({len(self.palette.keypoint_colors)}) does not matches that of keypoints ({len(kp3d)})")
        return self._sk.Kp3dJob(-1, -1, self._sk.map_params((canvas, hw)), score)

    def _load_frame_kp3d(self, label, input_spa_labels, poses: Dict):
        """_load_frame_kp2d with the plan left to the device, in its order: what it raises before plan_draw_calls looks at a keypoint
        is returned (not raised); what it raises afterwards -- the crop, the size and the 2 % checks -- is kept in fr["late"].  The
        errors in between are the device's (skeleton.plan_error); _resize_on_device_kp2d raises the three in the order of "kp2d"."""
        scene_label, spa, tem = label
        sk, cam = self._sk, self.cameras[scene_label][spa]
        try:
            kp3d, score = self._kp3d_pose_and_score(label, poses)
            kp_path = self.get_file_path(self.kp3d_path_pat, scene_label, spa, tem)
            if not self.has_gt_target and spa not in input_spa_labels:
                img, mask, img_path, hw = None, None, kp_path, (int(cam["height"]), int(cam["width"]))
            else:
                img_path = self.get_file_path(self.image_path_pat, scene_label, spa, tem)
                fmask_path = self.get_file_path(self.fmask_path_pat, scene_label, spa, tem)
                img, mask = _open(img_path, "RGB"), _open(fmask_path, "L")
                hw = img.shape[:2]
            sk._check_out_shape(hw)
            canvas = self.kp2d_canvas_shape or (int(cam["height"]), int(cam["width"]))
            plan = self._kp3d_job(kp3d, score, canvas, hw)
        except Exception as e:  # noqa: BLE001  (kept for its turn in label order)
            return e
        fr = {"img": img, "mask": mask, "plan": plan, "crop": None, "path": kp_path, "label": label, "late": None, "kp3d": kp3d}
        try:
            if mask is not None:
                fr["crop"] = crop_box(mask, img_path)
                size = lambda a: (a.shape[1], a.shape[0])  # PIL's (w, h)
                if not (size(img) == size(mask) == plan.out_size):
                    raise AssertionError(f"Error: image size: {size(img)} != fmask size: {size(mask)} != skeleton size: {plan.out_size}")
                if self.has_gt_target and spa in input_spa_labels and _mask_mean_at_most(mask, 0.02):
                    raise AssertionError("Error: foreground mask < 2%. Please check the data.")
        except Exception as e:  # noqa: BLE001
            fr["late"] = e
        return fr

    def _plan_errors(self, frames: List[Dict], status) -> List:
        """`status` of _kp2d_draw read back (the one read-back of a task's plans; waits for the stream) -> per frame the ValueError
        plan_draw_calls raises for it, or None."""
        if status is None:
            return [None] * len(frames)
        order, st = status
        flags = st[:, 0].cpu().tolist()
        errs: List = [None] * len(frames)
        for i, f in zip(order, flags):
            errs[i] = self._sk.plan_error(f, self._plan_tables)
        return errs

    # -- device_decode=True: the host half of one frame, for both skeleton sources -------------------------------------------------
    def _load_frame_deferred(self, label, input_spa_labels, poses: Optional[Dict] = None):
        """_load_frame / _load_frame_kp2d up to the pixels: the frame's files are read and probed (_read), not decoded, in the same
        order; the crop and the checks that need pixels wait for _settle_frame.  fr["hw"]: the (h, w) of the frame's skeleton map.
        What reading raises is returned, not raised: _settle_frames raises it when the frame's turn comes."""
        scene_label, spa, tem = label
        kp2d, kp3d = self._drawn, self.skeleton_source == "kp3d"
        target = not self.has_gt_target and spa not in input_spa_labels
        fr = {"img": None, "mask": None, "skel": None, "plan": None, "crop": None, "check": self.has_gt_target and spa in input_spa_labels,
              "label": label}
        try:
            if kp3d:
                sk, cam = self._sk, self.cameras[scene_label][spa]
                fr["kp3d"], score = self._kp3d_pose_and_score(label, poses)
                fr["path"] = fr["img_path"] = self.get_file_path(self.kp3d_path_pat, scene_label, spa, tem)
                hw = (int(cam["height"]), int(cam["width"]))
            elif kp2d:
                sk, cam = self._sk, self.cameras[scene_label][spa]
                fr["path"] = fr["img_path"] = self.get_file_path(self.kp2d_path_pat, scene_label, spa, tem)
                inst = sk._read_instance(fr["path"])
                score = None if self.kp2d_score_path_pat is None else sk._read_instance(self.get_file_path(self.kp2d_score_path_pat, scene_label, spa, tem))
                hw = (int(cam["height"]), int(cam["width"]))
            else:
                fr["path"] = fr["img_path"] = self.get_file_path(self.skeleton_path_pat, scene_label, spa, tem)
                fr["skel"] = _read(fr["path"], "RGB")
                fr["hw"] = _hw(fr["skel"])
            if not target:
                fr["img_path"] = self.get_file_path(self.image_path_pat, scene_label, spa, tem)
                fr["img"] = _read(fr["img_path"], "RGB")
                fr["mask"] = _read(self.get_file_path(self.fmask_path_pat, scene_label, spa, tem), "L")
            if kp2d:
                if not target:
                    hw = _hw(fr["img"])
                sk._check_out_shape(hw)
                canvas = self.kp2d_canvas_shape or (int(cam["height"]), int(cam["width"]))
                fr["plan"] = self._kp3d_job(fr["kp3d"], score, canvas, hw) if kp3d else sk.plan_draw_calls(inst, score, (canvas, hw), self.palette)
                fr["hw"] = (fr["plan"].out_size[1], fr["plan"].out_size[0])
        except Exception as e:  # noqa: BLE001  (kept for its turn in label order)
            return e
        return fr

    # -- tables and descriptors of a task whose crops are known ----------------------------------------------------------------
    def _tables(self, frames: List[Dict]) -> Tuple[Dict[Tuple[int, int], Tuple[int, int]], np.ndarray]:
        """Pillow's coefficient tables of every distinct (crop size, output size) pair -> ({pair: (offset in int32 units, ksize)},
        the int32 array that holds them)."""
        ts = TableSet()
        for fr in frames:
            ts.add(fr["crop"][3], self.width)
            ts.add(fr["crop"][2], self.height)
        return ts.tables, ts.array()

    def _descriptors(self, frames: List[Dict], plane_offs, shapes, tables, tab: np.ndarray) -> np.ndarray:
        """int64 [n, FIELDS] frame descriptors (include/dm4d.h): plane_offs = (image, mask, skeleton) byte offsets per frame, image None
        where the skeleton serves as image; shapes = the (h, w) of each frame's planes."""
        H, W = self.height, self.width
        desc = np.zeros((len(frames), FIELDS), dtype=np.int64)
        scratch = Layout()  # the device scratch of the horizontal pass: one region per frame
        for i, (fr, (oi, om, os_), (sh, sw)) in enumerate(zip(frames, plane_offs, shapes)):
            top, left, ch, cw = fr["crop"][:4]
            htab, hk = tables[(cw, W)]
            vtab, vk = tables[(ch, H)]
            vb = tab[vtab: vtab + 2 * H].reshape(H, 2)
            y_first, y_last = int(vb[0, 0]), int(vb[-1, 0] + vb[-1, 1])  # crop rows the vertical windows read
            desc[i] = [os_ if oi is None else oi, om, os_, sh, sw, top, left, ch, cw, htab, hk, vtab, vk,
                       scratch.add((y_last - y_first) * W * 8), y_first, y_last - y_first]
        return desc

    def _resize_on_device_kp2d(self, frames: List[Dict], device: torch.device, pending: Optional[BaseException] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """The device half in "kp2d" mode; fills in the crop of every has_gt_target=False target.  Staging buffer on the device:

            [per group: n x h x w x 3 skeleton planes, tight | per group: one h x w mask per target | image planes and decoded masks]

        The first two parts exist on the device only; the third goes up from the pinned buffer in one copy, queued while the device
        draws.  Every size in it is known before the targets' crops are.  Tables and descriptors depend on those crops: they go up
        afterwards in a small buffer of their own (the library takes them by pointer, they need not lie in the staging buffer).

        "kp3d": `frames` are the frames before the first one that _load_frame_kp3d returned an exception for, `pending` is that
        exception.  The errors come in the order of "kp2d", whose loader raises at the first bad frame: per frame the plan's error
        (read back from the device after the draw was queued), then what the loader kept in fr["late"]; then `pending`; and only then
        the targets' empty maps."""
        H, W = self.height, self.width
        n = len(frames)
        cur, skel_offs, mask_offs, regions = self._kp2d_regions(frames)
        lay = Layout(cur)
        file_off = lay.total  # where the planes that come from files start
        file_offs = [[None if fr[name] is None else lay.add(fr[name].size) for name in ("img", "mask")] for fr in frames]
        total = lay.total

        on_gpu = device.type == "cuda"
        blob = pinned(total - file_off, device)
        st = self._stream(device) if on_gpu else None
        with (torch.cuda.device(device) if on_gpu else contextlib.nullcontext()), (torch.cuda.stream(st) if on_gpu else contextlib.nullcontext()):
            dev_blob = torch.empty(total, dtype=torch.uint8, device=device)
            boxes, status = self._kp2d_draw(frames, regions, dev_blob)
            # the image planes go into the pinned buffer, and up, while the device draws
            jobs = [(o - file_off, fr[name]) for fr, offs in zip(frames, file_offs) for o, name in zip(offs, ("img", "mask")) if o is not None]
            fill(blob.numpy(), jobs, self._pool)
            if total > file_off:
                dev_blob[file_off:].copy_(blob, non_blocking=True)
            for fr, err in zip(frames, self._plan_errors(frames, status)):
                if err is not None or fr.get("late") is not None:
                    raise err if err is not None else fr["late"]
            if pending is not None:
                raise pending
            for idx, h, w, b in boxes:  # 16 bytes per target; .cpu() waits for the stream
                for i, box in zip(idx, b.cpu().tolist()):
                    if box[2] < 0:
                        raise ValueError(f"skeleton is empty, no mask can be made from it: {frames[i]['path']}")
                    c0, r0, c1, r1 = skeleton_mask_rect(box, h, w)
                    frames[i]["crop"] = _crop_from_bbox((c0 - 1, r0 - 1, c1, r1), h, w)  # mask_bbox of the rectangle
            tables, tab = self._tables(frames)
            shapes = [(fr["plan"].out_size[1], fr["plan"].out_size[0]) for fr in frames]
            plane_offs = [(oi, mask_offs[i] if om is None else om, skel_offs[i]) for i, (oi, om) in enumerate(file_offs)]
            desc = self._descriptors(frames, plane_offs, shapes, tables, tab)
            meta_dev, meta, tab_off, tab_len, desc_off = pack_meta(tab, desc, device)
            pix, skel = self._crop_resize(dev_blob, meta, n, desc_off, tab_off, tab_len, meta=meta_dev)
        if on_gpu:
            st.synchronize()  # as _resize_on_device: the tensors are complete when handed over, the pinned buffers may be released
        return pix, skel

    def _kp2d_regions(self, frames: List[Dict]):
        """Where the drawn maps and the targets' masks of a "kp2d" task lie in the device staging buffer -> (the bytes they take, skeleton
        offsets per frame, mask offsets per frame (None: the frame's mask comes from a file), regions = [frame indices, number of
        targets among them, h, w, maps' offset, masks' offset or None] per group)."""
        n = len(frames)
        # groups of one canvas shape and one map size; the targets (whose maps feed dm4d_skeleton_box_mask_u8) come first in each
        groups: Dict[Tuple, List[int]] = {}
        for i, fr in enumerate(frames):
            groups.setdefault((fr["plan"].canvas_shape, fr["plan"].out_size), []).append(i)
        cur, skel_offs, mask_offs, regions = 0, [None] * n, [None] * n, []
        for (_, (w, h)), idx in groups.items():
            idx = [i for i in idx if frames[i]["mask"] is None] + [i for i in idx if frames[i]["mask"] is not None]
            for k, i in enumerate(idx):
                skel_offs[i] = cur + k * h * w * 3
            regions.append([idx, sum(frames[i]["mask"] is None for i in idx), h, w, cur, None])
            cur += len(idx) * h * w * 3
        for reg in regions:
            idx, n_targets, h, w = reg[:4]
            if n_targets:
                reg[5] = cur
                for k, i in enumerate(idx[:n_targets]):
                    mask_offs[i] = cur + k * h * w
                cur += n_targets * h * w
        return cur, skel_offs, mask_offs, regions

    def _kp2d_draw(self, frames: List[Dict], regions, dev_blob: torch.Tensor):
        """Draw every group's maps into `dev_blob` and derive the targets' boxes and box masks there, on the current stream ->
        ([(target frame indices, h, w, their device int32 [n, 4] boxes)], "kp3d": (the frame index of every planned job, the plans'
        device int32 [n, 2] status) | None)."""
        boxes, status = [], None
        if self.skeleton_source == "kp3d" and regions:
            status = self._kp3d_draw(frames, regions, dev_blob)
        for idx, nt, h, w, start, mask_start in regions:
            maps = dev_blob[start: start + len(idx) * h * w * 3].view(len(idx), h, w, 3)
            if status is None:
                self._sk.draw_plans_into([frames[i]["plan"] for i in idx], maps)
            if nt:
                masks = dev_blob[mask_start: mask_start + nt * h * w].view(nt, h, w)
                boxes.append((idx[:nt], h, w, ops.skeleton_box_mask(maps[:nt], skeleton_mask_pads(h, w), masks=masks)[0]))
        return boxes, status

    def _kp3d_draw(self, frames: List[Dict], regions, dev_blob: torch.Tensor):
        """One plan launch for the task's frames (its distinct poses go up here, the jobs with them; the cameras are on the device
        already) and one draw launch per region, into the regions' maps -> (the frame index of every job, the status on the device)."""
        sk, dev = self._sk, dev_blob.device
        order = [i for reg in regions for i in reg[0]]
        scene_label = frames[order[0]]["label"][0]
        cam_labels, K_d, T_d = self._cameras_on_device(scene_label, dev)
        pose_of = {}  # a task's distinct frames: one pose each
        for i in order:
            pose_of.setdefault(frames[i]["label"][2], frames[i]["kp3d"])
        tems = list(pose_of)
        scene = sk.DeviceScene(torch.from_numpy(np.stack(list(pose_of.values()))).to(dev), K_d, T_d)
        jobs = [frames[i]["plan"]._replace(frame=tems.index(frames[i]["label"][2]), camera=cam_labels.index(frames[i]["label"][1])) for i in order]
        groups, first = [], 0
        for idx, _, h, w, start, _ in regions:
            groups.append((first, len(idx), dev_blob[start: start + len(idx) * h * w * 3].view(len(idx), h, w, 3)))
            first += len(idx)
        return order, sk.plan_and_draw(scene, jobs, groups, self._plan_tables)[1]

    def _resize_on_device_decoded(self, frames: List, device: torch.device, stats: Dict) -> Tuple[torch.Tensor, torch.Tensor]:
        """The device half with device_decode=True, for both skeleton sources; fills in every frame's crop.  Staging buffer on the device:

            ["kp2d": the drawn maps and the targets' masks, as in _resize_on_device_kp2d | "files": one h x w mask per target |
             planes Pillow decoded | planes the device decodes]

        Only the third part comes up from the pinned buffer, in one copy: the files the decoders did not take.  The fourth is decoded
        from the files' bytes (codec.decode_staged; a file its decoder refuses is decoded by Pillow after all).  One
        dm4d_capture_plane_stats_u8 launch over every mask and every skeleton map that serves as image, and its read-back of 40 bytes
        a plane, give _settle_frames what the host route takes from pixels; the files route's target masks are then filled by one
        dm4d_capture_fill_rects_u8 launch.  `frames` may hold exceptions (_load_frame_deferred): the frames before the first are
        checked, then it is raised."""
        H, W = self.height, self.width
        kp2d = self._drawn
        live = frames[: next((i for i, fr in enumerate(frames) if isinstance(fr, BaseException)), len(frames))]
        n = len(live)
        if n == 0:
            _settle_frames(frames, {})
        if kp2d:
            cur, skel_offs, mask_offs, regions = self._kp2d_regions(live)
            lay = Layout(cur)
        else:
            lay, regions = Layout(), []
            mask_offs = [lay.add(fr["hw"][0] * fr["hw"][1]) if fr["mask"] is None else None for fr in live]
        files = [(i, name, fr[name]) for i, fr in enumerate(live) for name in ("img", "mask", "skel") if fr[name] is not None]
        offs, lo = {}, lay.total
        for i, name, a in files:
            if not isinstance(a, StagedFile):
                offs[i, name] = lay.add(a.size)
        hi = lay.total
        for i, name, a in files:
            if isinstance(a, StagedFile):
                offs[i, name] = lay.add(a.nbytes)
        blob = pinned(hi - lo, device)
        on_gpu = device.type == "cuda"  # as in _resize_on_device_kp2d: without a device the ops calls decide (the tests' stand-ins)
        st = self._stream(device) if on_gpu else None
        with (torch.cuda.device(device) if on_gpu else contextlib.nullcontext()), (torch.cuda.stream(st) if on_gpu else contextlib.nullcontext()):
            dev_blob = torch.empty(max(lay.total, 16), dtype=torch.uint8, device=device)
            boxes, status = self._kp2d_draw(live, regions, dev_blob)
            hosted = [(offs[i, name] - lo, a) for i, name, a in files if not isinstance(a, StagedFile)]
            fill(blob.numpy(), hosted, self._pool)
            if hi > lo:
                dev_blob[lo:hi].copy_(blob, non_blocking=True)
            stats["pillow"] += len(hosted)
            stats["bytes_uploaded"] += sum(a.size for _, a in hosted)
            staged = [(offs[i, name], a, a.plan.bytes_per_pixel) for i, name, a in files if isinstance(a, StagedFile)]
            if staged:
                decode_staged(staged, dev_blob, lambda f: _open(f.path, f.mode), stats)
            planes = [(i, offs[i, "mask"], *_hw(fr["mask"]), 1) for i, fr in enumerate(live) if fr["mask"] is not None]
            if not kp2d:
                planes += [(i, offs[i, "skel"], *fr["hw"], 3) for i, fr in enumerate(live) if fr["mask"] is None]
            rows = {}
            if planes:
                desc = np.zeros((len(planes), _l.CAPTURE_PLANE_FIELDS), dtype=np.int64)
                desc[:, :4] = [p[1:] for p in planes]
                meta_dev, meta, _, _, desc_off = pack_meta(None, desc, device)
                out = ops.capture_plane_stats(dev_blob, meta_dev, meta, len(planes), desc_off).cpu().tolist()  # waits for the stream
                rows = {p[0]: r for p, r in zip(planes, out)}
            for idx, _, _, b in boxes:  # "kp2d": 16 bytes per target
                rows.update({i: box + [0] for i, box in zip(idx, b.cpu().tolist())})
            bad = next(((i, e) for i, e in enumerate(self._plan_errors(live, status)) if e is not None), None)
            if bad is not None:  # "kp3d": the plan's error takes the frame's turn, as the loader's does for "kp2d"
                frames = frames[:bad[0]] + [bad[1]]
            _settle_frames(frames, rows)
            rects = [(mask_offs[i], *fr["hw"], *fr["rect"]) for i, fr in enumerate(live) if fr["mask"] is None and not kp2d]
            if rects:
                desc = np.zeros((len(rects), _l.CAPTURE_RECT_FIELDS), dtype=np.int64)
                desc[:, :7] = rects
                rect_dev, rect_meta, _, _, desc_off = pack_meta(None, desc, device)
                ops.capture_fill_rects(dev_blob, rect_dev, rect_meta, len(rects), desc_off)
            tables, tab = self._tables(live)
            plane_offs = [(offs.get((i, "img")), offs.get((i, "mask"), mask_offs[i]), skel_offs[i] if kp2d else offs[i, "skel"])
                          for i in range(n)]
            desc = self._descriptors(live, plane_offs, [fr["hw"] for fr in live], tables, tab)
            meta_dev, meta, tab_off, tab_len, desc_off = pack_meta(tab, desc, device)
            pix, skel = self._crop_resize(dev_blob, meta, n, desc_off, tab_off, tab_len, meta=meta_dev)
        if on_gpu:
            st.synchronize()  # as _resize_on_device: the tensors are complete when handed over, the pinned buffers may be released
        return pix, skel

    def _device(self) -> torch.device:
        device = torch.device(self.device) if self.device is not None else torch.device("cuda", torch.cuda.current_device())
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        return device

    def _stream(self, device: torch.device):
        st = getattr(self._tls, "stream", None)
        if st is None or st.device != device:
            st = self._tls.stream = torch.cuda.Stream(device=device)
        return st

    def _resize_on_device(self, frames: List[Dict], device: torch.device) -> Tuple[torch.Tensor, torch.Tensor]:
        """Pack planes, tables and descriptors into one staging buffer, upload it, launch; -> (pixel_values, skeletons)."""
        H, W = self.height, self.width
        tables, tab = self._tables(frames)
        # layout: [frame planes | tables | descriptors], every region 16-byte aligned
        lay = Layout()  # None: a has_gt_target=False target, whose image IS the skeleton
        plane_offs = [[None if fr[name] is None else lay.add(fr[name].size) for name in ("img", "mask", "skel")] for fr in frames]
        tab_off = lay.add(tab.nbytes)
        desc_off = lay.add(len(frames) * FIELDS * 8)
        desc = self._descriptors(frames, plane_offs, [fr["skel"].shape[:2] for fr in frames], tables, tab)
        blob = pinned(lay.total, device)
        jobs = [(o, fr[n]) for fr, offs in zip(frames, plane_offs) for o, n in zip(offs, ("img", "mask", "skel")) if o is not None]
        fill(blob.numpy(), jobs, self._pool)
        write_meta(blob.numpy(), tab, tab_off, desc, desc_off)
        if device.type != "cuda":  # no device: the ops call decides (it refuses host tensors -- there is no CPU fallback)
            return self._crop_resize(blob, blob, len(frames), desc_off, tab_off, tab.size)
        st = self._stream(device)
        with torch.cuda.device(device), torch.cuda.stream(st):
            dev_blob = blob.to(device, non_blocking=True)
            pix, skel = self._crop_resize(dev_blob, blob, len(frames), desc_off, tab_off, tab.size)
        # get_item may run on a loader thread whose consumer is another stream (runner.run_round_pipelined): the tensors are
        # complete when they are handed over, and the pinned buffer may be released.  This stalls the loader thread only.
        st.synchronize()
        return pix, skel

    # -- the route of a list of frames: load, crop, resize ---------------------------------------------------------------------------
    def _load(self, labels: List[Tuple[str, str, str]], input_spa_labels: List[str]):
        """Load and resize the frames `labels` name, by the route the constructor chose -> (crops, pixel_values, skeletons).  It raises
        what the first bad frame in label order raises."""
        kp3d_files = self._read_poses(labels) if self.skeleton_source == "kp3d" else None
        if self.device_decode:  # every crop comes from the device: the resize runs before the bookkeeping
            frames = list(self._pool.map(lambda lab: self._load_frame_deferred(lab, input_spa_labels, kp3d_files), labels))
            stats = {"device": 0, "pillow": 0, "bytes_uploaded": 0}
            try:
                pixel_values, skeletons = self._resize_on_device_decoded(frames, self._device(), stats)
            finally:
                with self._stats_lock:
                    for k, v in stats.items():
                        self.decode_stats[k] += v
        elif self.skeleton_source == "kp3d":  # as "kp2d"; the plans' errors come back from the device with the targets' boxes
            frames = list(self._pool.map(lambda lab: self._load_frame_kp3d(lab, input_spa_labels, kp3d_files), labels))
            bad = next((i for i, fr in enumerate(frames) if isinstance(fr, BaseException)), len(frames))
            if bad == 0:
                raise frames[0]
            pixel_values, skeletons = self._resize_on_device_kp2d(frames[:bad], self._device(), frames[bad] if bad < len(frames) else None)
        elif self.skeleton_source == "kp2d":  # the targets' crops come from the device: the resize runs before the bookkeeping
            frames = list(self._pool.map(lambda lab: self._load_frame_kp2d(lab, input_spa_labels), labels))
            pixel_values, skeletons = self._resize_on_device_kp2d(frames, self._device())
        else:
            frames = list(self._pool.map(lambda lab: self._load_frame(lab, input_spa_labels), labels))
            pixel_values, skeletons = self._resize_on_device(frames, self._device())
        return [fr["crop"] for fr in frames], pixel_values, skeletons

    def _crop_resize(self, blob: torch.Tensor, blob_host: torch.Tensor, n: int, desc_off: int, tab_off: int, tab_len: int,
                     meta: Optional[torch.Tensor] = None):
        """Where every route hands its staging buffer to the device: ops.capture_crop_resize -> (pixel_values, skeletons); under
        _load_cached the packed form instead, into the cells that call named for these `n` frames -> (None, None)."""
        sink = getattr(self._tls, "sink", None)
        extra = {} if meta is None else {"meta": meta}  # the "files" route has no meta, and says nothing of it
        if sink is None:
            return ops.capture_crop_resize(blob, blob_host, n, desc_off, tab_off, tab_len, self.height, self.width, **extra)
        if n != len(sink["cells"]):
            raise RuntimeError(f"SpaTemDataset: {n} frames reached the resize, {len(sink['cells'])} cells were named for them")
        rows, rows_dev = sink["rows"] = _cell_rows([[slab.data_ptr(), slab.numel(), off, 0] for slab, off in sink["cells"]], blob.device)
        ops.capture_crop_resize_packed(blob, blob_host, n, desc_off, tab_off, tab_len, self.height, self.width, rows, rows_dev, **extra)
        if blob.is_cuda:
            sink["event"] = torch.cuda.Event()
            sink["event"].record()
        sink["packed"] = True
        return None, None

    # -- device_cache=True ------------------------------------------------------------------------------------------------------------
    def _cache(self, device: torch.device) -> CellCache:
        with self._stats_lock:
            if device not in self._caches:
                self._caches[device] = CellCache(device, self.height * self.width * 8, self.device_cache_bytes)
            return self._caches[device]

    @property
    def cache_stats(self) -> Dict[str, int]:
        with self._stats_lock:
            caches = list(self._caches.values())
        total = {"hits": 0, "misses": 0, "unretained": 0, "cells": 0, "bytes": 0}
        for c in caches:
            for k, v in c.stats.items():
                total[k] += v
        return total

    def clear_device_cache(self) -> None:
        """Forget every cell and give the slabs back (CellCache.clear: the device is synchronised first).  Between get_item calls."""
        with self._stats_lock:
            caches = list(self._caches.values())
        for c in caches:
            c.clear()

    def _load_owned(self, cache: CellCache, owned: List, label_of: Dict, input_spa_labels: List[str], got: Dict) -> None:
        """_load on the frames of the keys this call owns, packed into cells of the cache -- or of a slab of this call's own for the
        cells the budget does not cover -- then published, or abandoned if anything was raised.  got[key] = (slab, offset, crop, None)."""
        sink = None
        try:
            cells = cache.reserve(owned)
            spare = sum(c is None for c in cells)
            if spare:
                own = torch.empty(spare * cache.cell_bytes, dtype=torch.uint8, device=cache.device)
                at = iter(range(0, own.numel(), cache.cell_bytes))
                cells = [(own, next(at)) if c is None else c for c in cells]
                retained = [c[0] is not own for c in cells]
            else:
                retained = [True] * len(cells)
            sink = self._tls.sink = {"cells": cells, "event": None, "packed": False}
            try:
                crops, _, _ = self._load([label_of[k] for k in owned], input_spa_labels)
            finally:
                self._tls.sink = None
            if not sink["packed"]:
                raise RuntimeError("SpaTemDataset: the route returned without reaching the resize")
        except BaseException:
            if sink is not None and sink["event"] is not None:
                sink["event"].synchronize()  # the pack was queued before the route raised: its cells are free only once it has run
            cache.abandon(owned)
            raise
        for k, (slab, off), crop, keep in zip(owned, cells, crops, retained):
            got[k] = (slab, off, crop, None)
            if keep:
                cache.publish(k, list(crop), sink["event"])
            else:
                cache.abandon([k])

    def _load_cached(self, labels: List[Tuple[str, str, str]], input_spa_labels: List[str]):
        """_load through the cell cache: the route runs on the frames no earlier call left a cell of (in label order, so that the
        first bad frame among them is the first bad frame: hits never raised), and one unpack launch writes all rows, hits and fresh
        cells alike.  The claim protocol is capture_cache.py's: what this call owns is published or abandoned before it waits.
        Which exception is raised: the flag-off call's whenever this call owns all its misses (every serial use).  When another thread
        holds some of this call's keys pending, the frames this call owns are loaded first and the others' only if their owner
        abandoned them: of two bad frames the one raised may then be the later one in label order."""
        device = self._device()
        cache = self._cache(device)
        keys = [(device.index, scene_label, spa, tem, spa in input_spa_labels) for scene_label, spa, tem in labels]
        label_of = dict(zip(keys, labels))
        got: Dict = {}  # key -> (slab, offset, crop, the event to wait for | None)
        on_gpu = device.type == "cuda"
        st = self._stream(device) if on_gpu else None
        with (torch.cuda.device(device) if on_gpu else contextlib.nullcontext()), (torch.cuda.stream(st) if on_gpu else contextlib.nullcontext()):
            todo = list(label_of)
            while todo:
                hits, owned, todo = cache.claim(todo)
                got.update({c.key: (c.slab, c.offset, c.meta, c.event) for c in hits})
                if owned:
                    self._load_owned(cache, owned, label_of, input_spa_labels, got)
                if todo:
                    cache.wait(todo)
            for ev in {id(e): e for _, _, _, e in got.values() if e is not None}.values():
                st.wait_event(ev)
            rows, rows_dev = _cell_rows([[got[k][0].data_ptr(), got[k][0].numel(), got[k][1], r] for r, k in enumerate(keys)], device)
            pixel_values, skeletons = ops.capture_unpack_cells(rows, rows_dev, len(keys), self.height, self.width)
        if on_gpu:
            st.synchronize()  # as _resize_on_device: the tensors are complete when handed over; a slab of this call's own may go
        return [list(got[k][2]) for k in keys], pixel_values, skeletons

    # -- the get_item contract (spatem_dataset.py:77-229) -------------------------------------------------------------------------
    def get_item(self, scene_label: str, spa_labels: List[str], tem_labels: List[str], input_spa_labels: List[str]) -> Dict:
        if len(spa_labels) > 1 and len(tem_labels) == 1:
            domain = "spatial"
        elif len(spa_labels) == 1 and len(tem_labels) > 1:
            domain = "temporal"
        else:
            raise ValueError(f"Error: invalid spa_labels and tem_labels: {spa_labels} and {tem_labels}")
        cameras = self.cameras[scene_label]
        if domain == "spatial":
            labels = [(scene_label, s, tem_labels[0]) for s in spa_labels]
        else:  # the nearest input camera's frames first, then the target's
            cams = [self._nearest(cameras, spa_labels[0], input_spa_labels)] + list(spa_labels)
            labels = [(scene_label, s, t) for s in cams for t in tem_labels]

        crops, pixel_values, skeletons = (self._load_cached if self.device_cache else self._load)(labels, input_spa_labels)
        Ks = torch.stack([_intrinsic(cameras[s]["K"], crop, self.height) for (_, s, _), crop in zip(labels, crops)])
        poses = relative_poses(torch.stack([cameras[s]["pose"] for _, s, _ in labels]))
        hws = [(cameras[s]["height"], cameras[s]["width"]) for _, s, _ in labels]

        n = len(labels)
        pl = plucker_maps(self.height, self.width, Ks, poses) if self.plucker == "host" else None
        cond_masks = torch.ones(n, 1, self.height, self.width)
        cond_masks[n // 2:] = 0.0
        lo, hi = -1.0 - 1e-6, 1.0 + 1e-6  # check_output; pixel_values / skeletons lie in [-1, 1] by construction
        if pl is not None and (lo > pl.min() or hi < pl.max()):
            raise ValueError(f"Error: plucker embeds are out of range: {pl.min()} < {lo} or {pl.max()} > {hi}")
        if lo > cond_masks.min() or hi < cond_masks.max():
            raise ValueError(f"Error: cond masks are out of range: {cond_masks.min()} < {lo} or {cond_masks.max()} > {hi}")
        return {"domain": domain, "labels": labels, "pixel_values": pixel_values, "plucker_embeds": pl, "skeletons": skeletons,
                "cond_masks": cond_masks, "Ks": Ks, "hws": hws, "crops": crops, "poses": poses}
