"""Raw-capture rectification: the reference's scripts/download/extract_dnar_images.py (``calc_unified_cameras``, ``calib_undist_image``,
``extract_images``), the step that turns raw 2448 x 2048 camera frames into the ``images/{cam}/{frame}.webp`` files everything else
reads.  The reference does the image arithmetic through torch on the GPU, EasyVolcap's ``colmap_undistort`` and ``cv2.resize``; here
one launch of csrc/rectify.hip does all four steps (colour table, undistortion, area resize, crop) for a batch of images of different
sizes and cameras, byte for byte the numpy definition tests/rectify_model.py (DESIGN.md "Raw-capture rectification").  None of COLMAP,
EasyVolcap and OpenCV is a dependency, and the distance of the definition to them is not measured.

  * ``calc_unified_cameras``, ``calib_undist_image``: the reference's names, argument order and arithmetic;
  * ``rectify_batch``: arrays + cameras -> uint8 device tensors, one ``dm4d_rectify_u8`` call per memory-budget chunk;
  * ``extract_images``: the stage (host/staging.py ``run_stage``): sources are read, probed or decoded in the pool's threads, staged as
    bytes, rectified, copied back once per batch and saved by the pool's threads;
  * ``SmcFrames``: the undecoded colour streams of an ``.smc`` file (needs ``h5py``).

There is no CPU path: a ``device`` that is not a HIP device is an error.
"""
from __future__ import annotations

import copy
import functools
import io
import itertools
import json
import os
import threading
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch
from PIL import Image

from . import codec as _codec
from . import lib as _l
from . import ops
from . import staging as _st

FIELDS = _l.RECTIFY_FIELDS
MAX_SCALE = _l.RECTIFY_MAX_SCALE
CAM_FLOATS = 16
STAGE_BYTES = 1 << 30  # device bytes (sources + results) of one dm4d_rectify_u8 call
WINDOW_BATCHES = 8      # batches per GPU that extract_images takes from `frames` at a time


# -- the reference's camera arithmetic ---------------------------------------------------------------------------------------------------
def calc_unified_cameras(cams, image_size=1024):
    """extract_dnar_images.py:20-86: every camera (labels sorted; index 0-47 the 5 MP cameras, 48-59 the 12 MP ones) is resized to
    the target focal length and cropped about its principal point -> a deep copy of `cams` whose entries have the new ``K``, ``H``,
    ``W`` and gain ``resized_wh`` = (w, h) and ``cropped_ltrb`` = (left, top, right, bottom).  An entry is a mapping with ``K`` (3 x 3
    array), ``H``, ``W``.  The reference's ``round`` / ``int`` rules, its asserts and its ``ValueError("Unknown camera id: ...")``."""
    cams = copy.deepcopy(cams)
    for cam_id, cam_label in enumerate(sorted(cams.keys())):
        cam = cams[cam_label]
        K, h, w = cam["K"], cam["H"], cam["W"]
        if 0 <= cam_id <= 47:
            tar_f, tar_h, tar_w = 2496 * (image_size / 1920), image_size, image_size
        elif 48 <= cam_id <= 59:
            tar_f = 3648 * (image_size / 1920)
            tar_h = tar_w = int(2880 * (image_size / 1920))
        else:
            raise ValueError(f"Unknown camera id: {cam_id}")
        # resize to the target focal length
        K = copy.deepcopy(K)
        scale_w, scale_h = tar_f / K[0, 0], tar_f / K[1, 1]
        resized_w, resized_h = int(round(w * scale_w)), int(round(h * scale_h))
        K[0, 0] *= scale_w
        K[0, 2] *= scale_w
        K[1, 1] *= scale_h
        K[1, 2] *= scale_h
        # crop about the principal point
        cx, cy = K[0, 2], K[1, 2]
        left, right = int(round(cx - tar_w // 2)), int(round(cx + tar_w // 2))
        top, bottom = int(round(cy - tar_h // 2)), int(round(cy + tar_h // 2))
        assert left >= 0 and right <= resized_w and top >= 0 and bottom <= resized_h
        K[0, 2], K[1, 2] = tar_w / 2, tar_h / 2
        assert K[0, 0] - tar_f < 1e-6 and K[1, 1] - tar_f < 1e-6 and K[0, 2] == tar_w / 2 and K[1, 2] == tar_h / 2
        cam["K"], cam["H"], cam["W"] = K, tar_h, tar_w
        cam["resized_wh"] = (resized_w, resized_h)
        cam["cropped_ltrb"] = (left, top, right, bottom)
    return cams


# -- tables (host) -----------------------------------------------------------------------------------------------------------------------
def colour_table(ccm_data) -> np.ndarray:
    """fp32 [3, 256]: what the reference's ``calib_color`` (extract_dnar_images.py:90-100) makes of every byte of every RGB channel,
    computed by torch CPU with the reference's own expression; `ccm_data` is [3, 3] with rows in B, G, R order, permuted with
    ``[2, 1, 0]`` as there."""
    ccm = np.asarray(ccm_data, dtype=np.float64)
    if ccm.shape != (3, 3):
        raise ValueError(f"ccm: expected [3, 3], got {ccm.shape}")
    x = torch.arange(256, dtype=torch.float32)[None, :, None, None].expand(1, 256, 1, 3)
    sol = torch.from_numpy(ccm).float()[None][:, [2, 1, 0], :]
    rs = (torch.stack([x ** 2, x, torch.ones_like(x)], dim=-1) * sol[:, None, None, :, :]).sum(dim=-1)
    return np.ascontiguousarray(rs[0].clamp(0, 255)[:, 0, :].t().numpy())


def area_table(n_in: int, n_out: int) -> Tuple[np.ndarray, int]:
    """The area-resize table of an axis n_in -> n_out as the library takes it -> (int32 words: n_out windows {first cell, taps} then
    n_out x k fp32 weights, k).  Output i covers [i s, (i + 1) s), s = n_in / n_out; a weight is fp32(overlap / s): the overlap in
    exact integers (units of 1 / n_out), the quotient in fp64.  s outside 1..MAX_SCALE is a ValueError (the reference only shrinks)."""
    n_in, n_out = int(n_in), int(n_out)
    if n_out < 1 or not (n_out <= n_in <= MAX_SCALE * n_out):
        raise ValueError(f"area resize {n_in} -> {n_out}: the scale is outside 1..{MAX_SCALE}")
    i = np.arange(n_out, dtype=np.int64)
    first = (i * n_in) // n_out
    end = -((-(i + 1) * n_in) // n_out)
    k = int((end - first).max())
    cell = first[:, None] + np.arange(k, dtype=np.int64)[None, :]
    overlap = np.minimum((i[:, None] + 1) * n_in, (cell + 1) * n_out) - np.maximum(i[:, None] * n_in, cell * n_out)
    wts = (np.clip(overlap, 0, None).astype(np.float64) / np.float64(n_in)).astype(np.float32)
    win = np.stack([first, end - first], axis=1).astype(np.int32)
    return np.concatenate([win.reshape(-1), wts.reshape(-1).view(np.int32)]), k


class Rectification:
    """Everything of one camera that does not depend on the frame: the colour table, the two area tables, the camera constants."""

    def __init__(self, K, D, ccm_data, resized_wh, cropped_ltrb, undist_K, undist_hw, source_hw=None):
        K, Ku = np.asarray(K, dtype=np.float64), np.asarray(undist_K, dtype=np.float64)
        D = np.asarray(D, dtype=np.float64).reshape(-1)
        if K.shape != (3, 3) or Ku.shape != (3, 3) or D.size < 5:
            raise ValueError("K, undist_K: expected [3, 3]; D: expected k1, k2, p1, p2, k3")
        self.uh, self.uw = int(undist_hw[0]), int(undist_hw[1])
        self.rw, self.rh = int(resized_wh[0]), int(resized_wh[1])
        _st.check_sizes([(self.uh, self.uw), (self.rh, self.rw)], _l.RECTIFY_MAX_SIDE, "undist_hw, resized_wh")
        left, top, right, bottom = (int(v) for v in cropped_ltrb)
        if not (0 <= left < right <= self.rw and 0 <= top < bottom <= self.rh):
            raise ValueError(f"cropped_ltrb {(left, top, right, bottom)} is empty or leaves the resized image {self.rw} x {self.rh}")
        self.top, self.left, self.ch, self.cw = top, left, bottom - top, right - left
        self.source_hw = None if source_hw is None else (int(source_hw[0]), int(source_hw[1]))
        self.htab, self.hk = area_table(self.uw, self.rw)
        self.vtab, self.vk = area_table(self.uh, self.rh)
        self.lut = colour_table(ccm_data)
        cam = np.zeros(CAM_FLOATS, dtype=np.float32)
        cam[:4] = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
        cam[4:9] = D[:5]
        cam[9:13] = Ku[0, 2], Ku[1, 2], 1.0 / Ku[0, 0], 1.0 / Ku[1, 1]  # the reciprocals in fp64, rounded once
        self.words = np.concatenate([self.htab, self.vtab, cam.view(np.int32)])
        self.out_bytes = self.ch * self.cw * 3


def load_cameras(cameras) -> Dict[str, Rectification]:
    """`cameras`: a dict or the path of a JSON file ``{cam_label: {K, D, ccm, K_undist, H_undist, W_undist, H, W}}`` (K, K_undist 3 x 3;
    D = k1, k2, p1, p2, k3; ccm 3 x 3 with rows in B, G, R order; H, W the raw frame; DESIGN.md "Raw-capture rectification") -> the
    Rectification of every camera.  The resize and the crop are ``calc_unified_cameras`` of the undistorted cameras, as in the
    reference, unless an entry names ``resized_wh`` and ``cropped_ltrb`` itself."""
    if not isinstance(cameras, dict):
        with open(os.fspath(cameras)) as f:
            cameras = json.load(f)
    need = ("K", "D", "ccm", "K_undist", "H_undist", "W_undist", "H", "W")
    for label, cam in cameras.items():
        missing = [k for k in need if k not in cam]
        if missing:
            raise ValueError(f"cameras[{label!r}]: missing {', '.join(missing)}")
    given = all("resized_wh" in c and "cropped_ltrb" in c for c in cameras.values())
    if not given:
        unified = calc_unified_cameras({label: {"K": np.array(c["K_undist"], dtype=np.float64), "H": int(c["H_undist"]), "W": int(c["W_undist"])}
                                        for label, c in cameras.items()})
    out = {}
    for label, c in cameras.items():
        src = c if given else unified[label]
        out[str(label)] = Rectification(c["K"], c["D"], c["ccm"], src["resized_wh"], src["cropped_ltrb"], c["K_undist"],
                                        (c["H_undist"], c["W_undist"]), (c["H"], c["W"]))
    return out


# -- one library call --------------------------------------------------------------------------------------------------------------------
def _source_size(src) -> Tuple[int, int]:
    return (int(src.h), int(src.w)) if isinstance(src, _codec.StagedFile) else (int(src.shape[0]), int(src.shape[1]))


def _pillow_rgb(data: bytes) -> np.ndarray:
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB"))


def _rectify_chunk(sources: Sequence, rects: Sequence[Rectification], dev: torch.device, pool: Optional[ThreadPoolExecutor],
                   stats: Optional[dict] = None):
    """One ``dm4d_rectify_u8`` call on the current stream.  A source is a uint8 [h, w, 3] array or a codec.StagedFile, which is decoded
    into its region on the device (a refused file takes the Pillow route) -> (the packed results on the device, their byte offsets,
    what the caller keeps referenced until it has synchronised the stream).  stats: "device", "pillow" and "bytes_uploaded" are added
    to: the source bytes that cross PCIe, i.e. the host-decoded pixels (padded to 16 bytes each), the file bytes of the staged files and
    the pixels of those a decoder refused."""
    n = len(sources)
    sizes = _st.check_sizes([_source_size(s) for s in sources], _l.RECTIFY_MAX_SIDE, "images")
    for k, (r, hw) in enumerate(zip(rects, sizes)):
        if r.source_hw is not None and r.source_hw != hw:
            raise ValueError(f"images[{k}]: {hw[1]} x {hw[0]} is not the camera's frame size {r.source_hw[1]} x {r.source_hw[0]}")
    # the host-decoded sources lie first and together: only they are uploaded as pixels; the regions of staged files follow them
    is_file = [isinstance(s, _codec.StagedFile) for s in sources]
    planes, outs = _st.Layout(), _st.Layout()
    src_off = [0] * n
    for k in [k for k in range(n) if not is_file[k]]:
        src_off[k] = planes.add(sizes[k][0] * sizes[k][1] * 3)
    host_bytes = planes.total
    for k in [k for k in range(n) if is_file[k]]:
        src_off[k] = planes.add(sizes[k][0] * sizes[k][1] * 3)
    desc = np.zeros((n, FIELDS), dtype=np.int64)
    words, where, used = [], {}, 0
    for k, (r, (h, w)) in enumerate(zip(rects, sizes)):
        if id(r) not in where:  # a camera's tables stand once in a call
            where[id(r)] = used
            words.append(r.words)
            used += r.words.size
        t = where[id(r)]
        desc[k, :17] = [src_off[k], h, w, r.uh, r.uw, r.rh, r.rw, r.top, r.left, r.ch, r.cw, t, r.hk, t + r.htab.size, r.vk,
                        t + r.htab.size + r.vtab.size, outs.add(r.out_bytes)]
    blob = torch.empty(planes.total, dtype=torch.uint8, device=dev)
    host = None
    if host_bytes:
        host = _st.pinned(host_bytes, dev)
        _st.fill(host.numpy(), [(src_off[k], s) for k, s in enumerate(sources) if not is_file[k]], pool)
        blob[:host_bytes].copy_(host, non_blocking=True)
    if stats is not None:
        stats["bytes_uploaded"] = stats.get("bytes_uploaded", 0) + host_bytes
    staged = [(src_off[k], s, 3) for k, s in enumerate(sources) if is_file[k]]
    if staged:
        _codec.decode_staged(staged, blob, lambda f: _pillow_rgb(f.data), stats)
    lut_host = _st.pinned(n * 3 * 256 * 4, dev)
    lut_host.numpy().view(np.float32).reshape(n, 3, 256)[:] = np.stack([r.lut for r in rects])
    lut = lut_host.to(dev, non_blocking=True).view(torch.float32).view(n, 3, 256)
    meta, meta_host, tab_off, tab_len, desc_off = _st.pack_meta(np.concatenate(words), desc, dev)
    out = ops.rectify(blob, meta, meta_host, n, desc_off, tab_off, tab_len, lut, outs.total)
    return out, [int(v) for v in desc[:, 16]], (host, lut_host, meta_host)


def _views(out: torch.Tensor, offsets: Sequence[int], rects: Sequence[Rectification]) -> List[torch.Tensor]:
    return [out[o: o + r.out_bytes].view(r.ch, r.cw, 3) for o, r in zip(offsets, rects)]


def rectify_batch(images: Sequence[np.ndarray], cameras: Sequence[Rectification], device, *, stage_bytes: int = STAGE_BYTES) -> List[torch.Tensor]:
    """uint8 [h, w, 3] RGB arrays and the Rectification of each -> uint8 [crop h, crop w, 3] tensors on `device`, byte for byte
    tests/rectify_model.py.  One ``dm4d_rectify_u8`` call per chunk of images whose sources and results stay within `stage_bytes`."""
    images, cameras = list(images), list(cameras)
    if len(images) < 1 or len(images) != len(cameras):
        raise ValueError("rectify_batch: one camera per image, at least one image")
    for k, a in enumerate(images):
        if not isinstance(a, np.ndarray) or a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
            raise ValueError(f"images[{k}]: expected a uint8 [h, w, 3] array")
    dev = _l.hip_device(device, "rectify_batch")
    needs = [a.shape[0] * a.shape[1] * 3 + r.out_bytes for a, r in zip(images, cameras)]
    result: List[torch.Tensor] = []
    with torch.cuda.device(dev):
        for first, last in _codec.chunks(needs, stage_bytes, 65535):
            out, offsets, keep = _rectify_chunk(images[first:last], cameras[first:last], dev, None)
            torch.cuda.current_stream().synchronize()  # the pinned buffers may go
            del keep
            result += _views(out, offsets, cameras[first:last])
    return result


def calib_undist_image(image, K, D, ccm_data, resized_wh, cropped_ltrb, *, undist_K, undist_hw, device=None):
    """extract_dnar_images.py:89-120 with its arguments in its order: an RGB uint8 [h, w, 3] array -> the colour-corrected,
    undistorted, resized (area) and cropped uint8 array, computed on `device` (None: the current HIP device).

    undist_K, undist_hw: the undistorted pinhole camera (3 x 3) and its image size (h, w).  The reference gets them from EasyVolcap's
    ``colmap_undistort``, i.e. COLMAP's ``UndistortCamera`` of (K, D), and its scenes ship the result as the ``colmap/dense`` model;
    deriving it from K and D is out of scope here, so the caller names it."""
    rect = Rectification(K, D, ccm_data, resized_wh, cropped_ltrb, undist_K, undist_hw)
    image = np.ascontiguousarray(image)
    return rectify_batch([image], [rect], "cuda" if device is None else device)[0].cpu().numpy()


# -- the stage ---------------------------------------------------------------------------------------------------------------------------
def _verifies(path: str) -> bool:
    try:
        with Image.open(path) as im:
            im.verify()
        return True
    except Exception:
        return False


def extract_images(frames: Iterable, cameras, out_images_dir: str, image_ext: str = ".webp", image_quality: int = 85, skip_exists: bool = True,
                   num_workers: int = 12, *, batch_size: int = 8, gpu_ids: Optional[Sequence[int]] = None, device_decode: bool = False) -> dict:
    """Rectify every frame of `frames` and write ``out_images_dir/{cam_label}/{frame_label}{image_ext}`` with
    ``Image.fromarray(a).save(path, quality=image_quality)``: extract_dnar_images.py:123-193 with its arguments in its names.

    frames: an iterable of (cam_label, frame_label, source), consumed lazily in windows of a few batches per GPU, so that an ``.smc``
    file's streams are never all in memory; a source is a path, the bytes of an encoded file, an RGB uint8 [h, w, 3] array, or a
    zero-argument callable that returns one of these, which a loader thread calls after the `skip_exists` check (what ``SmcFrames``
    yields: a frame that is skipped is never read).  cameras: see ``load_cameras``.  skip_exists: a file that exists is kept only if
    ``Image.open(path).verify()`` accepts it, and is removed and written again otherwise, as in the reference.  One worker thread per GPU
    id; reading, decoding and saving go through a pool of `num_workers` threads.

    device_decode: the loader threads only read and probe encoded sources (host/jpegdec.py, host/pngdec.py); the files the probes take
    upload their file bytes and are decoded into the staging buffer on the device, byte for byte Pillow's pixels; a file a decoder
    refuses, and whatever the probes do not take, is decoded by Pillow inside the same call.  The files written are the same.

    Returns counts: ``frames``, ``written``, ``skipped``, ``device_decoded``, ``pillow_decoded``, and ``bytes_uploaded``: the source
    bytes that crossed PCIe (decoded pixels, file bytes of device-decoded files; tables and descriptors are not counted)."""
    if batch_size < 1:
        raise ValueError("batch_size must be at least 1")
    rects = load_cameras(cameras)  # every scale and crop is checked here, before any device is touched
    counts = {"frames": 0, "written": 0, "skipped": 0, "device_decoded": 0, "pillow_decoded": 0, "bytes_uploaded": 0}
    lock = threading.Lock()
    n_gpus = len(gpu_ids) if gpu_ids is not None else max(1, torch.cuda.device_count())
    it = iter(frames)
    while True:
        window = [(str(c), str(f), s) for c, f, s in itertools.islice(it, WINDOW_BATCHES * n_gpus * batch_size)]
        if not window:
            return counts
        for c, _, _ in window:
            if c not in rects:
                raise ValueError(f"frames: camera {c!r} is not in cameras")
        counts["frames"] += len(window)
        counts["written"] += _extract_window(window, rects, counts, lock, out_images_dir, image_ext, image_quality, skip_exists, num_workers,
                                             batch_size, gpu_ids, device_decode)


def _extract_window(frames: List[Tuple[str, str, object]], rects: Dict[str, Rectification], counts: dict, lock, out_images_dir: str,
                    image_ext: str, image_quality: int, skip_exists: bool, num_workers: int, batch_size: int, gpu_ids, device_decode: bool) -> int:
    """One ``run_stage`` over the frames of a window of ``extract_images`` -> the number of files written; the other counts are added
    to `counts` under `lock`."""
    paths = [f"{out_images_dir}/{c}/{f}{image_ext}" for c, f, _ in frames]
    batches = [list(range(i, min(i + batch_size, len(frames)))) for i in range(0, len(frames), batch_size)]

    def pending(k: int) -> bool:
        if skip_exists and os.path.exists(paths[k]):
            if _verifies(paths[k]):
                return False
            os.remove(paths[k])
        return True

    def load(k: int):
        """-> (the source as the chunk takes it, whether Pillow decoded it)"""
        src = frames[k][2]
        if callable(src):
            src = src()
        if isinstance(src, np.ndarray):
            if src.dtype != np.uint8 or src.ndim != 3 or src.shape[2] != 3:
                raise ValueError(f"frames: the array of {frames[k][0]}/{frames[k][1]} is not uint8 [h, w, 3]")
            return src, False
        data = _codec.read_file(src)
        if device_decode:
            from . import jpegdec, pngdec
            f = _codec.probe_file(data, (jpegdec, pngdec))
            if f is not None and (f.mode == "RGB" or (f.mode == "L" and f.codec is jpegdec)):
                return f, False
        return _pillow_rgb(data), True

    def save(a: np.ndarray, path: str) -> None:
        _st.atomic_write(path, lambda tmp: Image.fromarray(a).save(tmp, quality=image_quality))

    def process_batch(_model, batch: List[int], dev: torch.device, pool: ThreadPoolExecutor) -> List:
        todo = [k for k, go in zip(batch, _st.pool_map(pool, pending, batch)) if go]
        with lock:
            counts["skipped"] += len(batch) - len(todo)
        if not todo:
            return []
        loaded = _st.pool_map(pool, load, todo)
        stats: dict = {}
        out, offsets, keep = _rectify_chunk([s for s, _ in loaded], [rects[frames[k][0]] for k in todo], dev, pool, stats)
        host = out.cpu().numpy()  # one copy per batch; synchronises: the pinned buffers may go
        del keep
        with lock:
            counts["device_decoded"] += stats.get("device", 0)
            counts["pillow_decoded"] += stats.get("pillow", 0) + sum(1 for _, by_pillow in loaded if by_pillow)
            counts["bytes_uploaded"] += stats.get("bytes_uploaded", 0)
        views = [host[o: o + rects[frames[k][0]].out_bytes].reshape(rects[frames[k][0]].ch, rects[frames[k][0]].cw, 3) for o, k in zip(offsets, todo)]
        return [pool.submit(save, a, paths[k]) for a, k in zip(views, todo)]

    return _st.run_stage("extract_images", gpu_ids, num_workers, "dm4d-rectify", batches, lambda dev: None, process_batch)


class SmcFrames:
    """The undecoded colour streams of a DNA-Rendering ``.smc`` file as ``extract_images`` takes them: iterating yields
    (``f"{cam:02d}"``, ``f"{frame:06d}"``, a callable that reads the bytes of the encoded frame) for every camera of `camera_ids` and
    every frame of the first of them, the reference's keys and labels (extract_dnar_images.py:150-152, 179-182); a stream is read from
    the file only when its callable is called (h5py serialises the reads of the loader threads).  Needs ``h5py``, which is imported
    here and nowhere else; this class has not been run against a real file.  ``release()`` closes the file."""

    def __init__(self, smc_path: str, cam_group: str = "Camera_5mp", camera_ids: Iterable[int] = range(48)):
        try:
            import h5py
        except ImportError as e:
            raise ImportError("SmcFrames reads .smc files through h5py, which is not installed") from e
        self.smc = h5py.File(os.fspath(smc_path), "r")
        self.cam_group, self.camera_ids = cam_group, [int(c) for c in camera_ids]

    def __iter__(self):
        group = self.smc[self.cam_group]
        frame_ids = sorted(int(k) for k in group[str(self.camera_ids[0])]["color"].keys())
        for cam in self.camera_ids:
            for frame in frame_ids:
                yield f"{cam:02d}", f"{frame:06d}", functools.partial(self._read, group[str(cam)]["color"], str(frame))

    @staticmethod
    def _read(streams, frame: str) -> bytes:
        return np.asarray(streams[frame][()]).tobytes()

    def release(self) -> None:
        self.smc.close()
