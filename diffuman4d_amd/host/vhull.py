"""Visual-hull carving: one point cloud per frame from a scene's foreground masks and cameras (``surfs/{frame}.ply``,
``surfs_bounds.json``, ``sparse_pcd.ply``).

The reference's ``scripts/preprocess/carve_visual_hull.py`` (the ``carve_vhull`` action of ``preprocess.sh``) with the same function
names and arguments, built from its behaviour.  What it does per batch of voxels with about twenty torch operators -- build the
centres, project them into every view in fp64, round, test the image range, gather the masks, count, compact -- runs here in three
launches per chunk of the grid (``dm4d_vhull_carve_chunk``: flags, a one-block scan, gather) on masks packed to bits.  The host
makes the grid axes, builds the cameras, decodes the PNG masks (frame ``t + 1`` in a thread pool while frame ``t`` carves) and
writes the PLY files.  With ``carve_scene(device_decode=True)`` the pool only reads the files and the device decodes the PNG masks
(``host/pngdec.py``) and packs them to bits, with the same files written.  There is no CPU path: a ``device`` that is not a HIP
device is an error.
"""
from __future__ import annotations

import json
import os
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from PIL import Image

from . import lib as _l
from . import ops
from .codec import decode_or_fallback, read_file
from .staging import MAX_HOST_THREADS  # noqa: F401  (importable from here as before)

PLY_HEADER = ("ply\n"
              "format binary_little_endian 1.0\n"
              "element vertex {n}\n"
              "property float x\n"
              "property float y\n"
              "property float z\n"
              "property uchar red\n"
              "property uchar green\n"
              "property uchar blue\n"
              "end_header\n")
PLY_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])


# -- files ------------------------------------------------------------------------------------------------------------------------
def load_binary_mask(path: str) -> torch.Tensor:
    """A foreground mask file -> [H, W] torch.bool, as the reference's ``to_tensor(Image.open(path)).squeeze(0) > 0.5`` gives it
    (carve_visual_hull.py:33-37): mode ``L`` is foreground where the value is >= 128 (127 / 255 < 0.5 < 128 / 255 in float32), mode
    ``1`` where the bit is set.  Any other mode raises ValueError: no conversion is made, it would change values."""
    with Image.open(path) as im:
        if im.mode == "L":
            return torch.from_numpy(np.asarray(im) >= 128)
        if im.mode == "1":
            return torch.from_numpy(np.asarray(im, dtype=bool).copy())
        raise ValueError(f"{path}: image mode {im.mode!r}, expected 'L' or '1'")


def save_pcd_ply(path: str, pts, colors=None) -> None:
    """Write a point cloud as binary little-endian PLY with the vertex properties ``float x, y, z; uchar red, green, blue`` (white
    when `colors` is None), creating parent directories (carve_visual_hull.py:40-73).  The header is spelled out in PLY_HEADER as
    ``plyfile`` writes it for this vertex array; ``plyfile`` is not a dependency of this project, and byte identity with its output
    has not been checked against an installed copy."""
    pts = np.asarray(pts.detach().cpu() if torch.is_tensor(pts) else pts)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError(f"pts: expected [N, 3], got {pts.shape}")
    vertex = np.empty(len(pts), dtype=PLY_VERTEX)
    vertex["x"], vertex["y"], vertex["z"] = pts[:, 0], pts[:, 1], pts[:, 2]
    if colors is None:
        vertex["red"] = vertex["green"] = vertex["blue"] = 255
    else:
        colors = np.asarray(colors.detach().cpu() if torch.is_tensor(colors) else colors)
        if colors.shape != pts.shape:
            raise ValueError(f"colors: expected {pts.shape}, got {colors.shape}")
        vertex["red"], vertex["green"], vertex["blue"] = colors[:, 0], colors[:, 1], colors[:, 2]
    parent = os.path.dirname(path)
    if parent:
        os.makedirs(parent, exist_ok=True)
    with open(path, "wb") as f:
        f.write(PLY_HEADER.format(n=len(pts)).encode("ascii"))
        f.write(vertex.tobytes())


# -- cameras ----------------------------------------------------------------------------------------------------------------------
def make_projection_matrix(K: torch.Tensor, R: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """K [B, 3, 3], R [B, 3, 3], t [B, 3] (world -> camera) -> P = K @ [R | t], [B, 3, 4] (carve_visual_hull.py:15-22)."""
    return K @ torch.cat([R, t.reshape(-1, 3, 1)], dim=-1)


def read_projections(cameras_path: str, cam_labels: Sequence[str]) -> torch.Tensor:
    """nerfstudio ``transforms.json`` -> P fp64 [len(cam_labels), 3, 4], one per selected camera, built as the reference builds it
    (carve_visual_hull.py:188-198): fp64 K from fl_x, fl_y, cx, cy; the camera-to-world matrix with its y and z columns negated
    (OpenGL -> OpenCV); its inverse; K @ [R | t].

    The reference takes every frame of the file, in file order, as the views, which is right only when the file lists exactly the
    selected cameras in sorted order.  Here the views are matched by ``camera_label`` when the frames carry one, and taken by
    position otherwise; a label that is missing, or a count that differs, raises ValueError."""
    if not cameras_path.endswith(".json"):
        raise NotImplementedError(f"EasyVolcap cameras are not supported ({cameras_path}): give a nerfstudio transforms.json")
    with open(cameras_path) as f:
        tf = json.load(f)["frames"]
    if tf and all("camera_label" in fr for fr in tf):
        by_label = {str(fr["camera_label"]): fr for fr in tf}
        missing = [c for c in cam_labels if c not in by_label]
        if missing:
            raise ValueError(f"cameras_path: {cameras_path} has no camera_label {missing} (it lists {sorted(by_label)})")
        tf = [by_label[c] for c in cam_labels]
    elif len(tf) != len(cam_labels):
        raise ValueError(f"cameras_path: {cameras_path} lists {len(tf)} frames without camera_label for {len(cam_labels)} selected "
                         "cameras; they can only be matched by position when the counts agree")
    B = len(tf)
    K = np.zeros((B, 3, 3), dtype=np.float64)
    cam2world = np.empty((B, 4, 4), dtype=np.float64)
    for i, fr in enumerate(tf):
        K[i, 0, 0], K[i, 1, 1], K[i, 0, 2], K[i, 1, 2], K[i, 2, 2] = fr["fl_x"], fr["fl_y"], fr["cx"], fr["cy"], 1.0
        cam2world[i] = np.asarray(fr["transform_matrix"], dtype=np.float64)
    cam2world[:, :3, 1] = -cam2world[:, :3, 1]  # OpenGL camera axes (y up, z backwards) -> OpenCV (y down, z forwards)
    cam2world[:, :3, 2] = -cam2world[:, :3, 2]
    world2cam = np.linalg.inv(cam2world)
    R = torch.from_numpy(world2cam[:, :3, :3].copy())
    t = torch.from_numpy(world2cam[:, :3, 3].copy())
    return make_projection_matrix(torch.from_numpy(K), R, t)


# -- carving ----------------------------------------------------------------------------------------------------------------------
def build_voxel_grid_linspaces(bounds, voxel_size) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The grid axes exactly as the reference makes them (carve_visual_hull.py:25-30): torch.arange(min, max, voxel_size) on the
    host, fp32 values and torch's own element count (it is not re-derived: arange(-0.1, 0.2, 0.1) has 4 elements)."""
    xmin, xmax, ymin, ymax, zmin, zmax = bounds
    return torch.arange(xmin, xmax, voxel_size), torch.arange(ymin, ymax, voxel_size), torch.arange(zmin, zmax, voxel_size)


def _check_args(fmasks, Ps, voxel_size, min_views) -> torch.Tensor:
    if not torch.is_tensor(fmasks) or fmasks.dim() != 3 or fmasks.dtype != torch.bool:
        raise ValueError(f"fmasks: expected a [B, H, W] torch.bool tensor, got {getattr(fmasks, 'dtype', type(fmasks))} "
                         f"{tuple(getattr(fmasks, 'shape', ()))}")
    if not torch.is_tensor(Ps) or Ps.dim() != 3 or tuple(Ps.shape[1:]) != (3, 4):
        raise ValueError(f"Ps: expected a [B, 3, 4] tensor, got {tuple(getattr(Ps, 'shape', ()))}")
    if Ps.dtype not in (torch.float64, torch.float32):
        raise ValueError(f"Ps: expected float64 (or float32, which is widened), got {Ps.dtype}")
    if fmasks.shape[0] != Ps.shape[0]:
        raise ValueError(f"fmasks / Ps: {fmasks.shape[0]} masks for {Ps.shape[0]} projection matrices")
    if fmasks.shape[0] < 1 or fmasks.shape[1] < 1 or fmasks.shape[2] < 1:
        raise ValueError(f"fmasks: empty shape {tuple(fmasks.shape)}")
    if not voxel_size > 0:
        raise ValueError(f"voxel_size: must be positive, got {voxel_size}")
    if min_views is not None and int(min_views) < 1:
        raise ValueError(f"min_views: must be at least 1 (or None for every view), got {min_views}")
    return Ps.to(torch.float64)


def _chunk_voxels(batch_size) -> int:
    """batch_size is an upper bound on the voxels per launch series: whole blocks, at least one, at most the library's limit."""
    blocks = max(1, min(int(batch_size), ops.VHULL_MAX_CHUNK) // ops.VHULL_BLOCK)
    return blocks * ops.VHULL_BLOCK


def _carve(bits: torch.Tensor, hw: Tuple[int, int], P: torch.Tensor, axes, batch_size, min_views, capacity: Optional[int] = None):
    """Device half of carve_visual_hull: `bits` packed masks, `P` fp64 [B, 3, 4] and `axes` fp32 on one HIP device -> [M, 3] fp32.

    The output is sized before the count is known: room for max(2^20, N / 16) points (at most N).  The library counts every kept
    point and writes those that fit; the host reads the count once, and only if the hull was larger than the room is the frame
    carved again into a buffer of exactly that many points, without a second read (the count is a pure function of the inputs)."""
    xs, ys, zs = axes
    N = xs.numel() * ys.numel() * zs.numel()
    chunk = _chunk_voxels(batch_size)
    need = 0 if min_views is None else int(min_views)
    dev = bits.device
    ws = ops.vhull_ws(min(chunk, N), dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    capacity = min(N, max(1 << 20, N // 16)) if capacity is None else min(N, int(capacity))

    def run(cap: int) -> torch.Tensor:
        out = torch.empty((cap, 3), dtype=torch.float32, device=dev)
        total.zero_()
        for first in range(0, N, chunk):
            ops.vhull_carve_chunk(xs, ys, zs, P, bits, hw, need, first, min(chunk, N - first), ws, total, out)
        return out

    out = run(capacity)
    M = int(total.item())  # the one read of the frame
    if M > capacity:
        return run(M)
    return out[:M] if 4 * M >= capacity else out[:M].clone()


@torch.no_grad()
def carve_visual_hull(fmasks, Ps, bounds, voxel_size=0.02, batch_size=1e6, min_views=None, device="cuda") -> torch.Tensor:
    """Carve the visual hull of one frame (carve_visual_hull.py:76-151).

    fmasks: [B, H, W] torch.bool; Ps: [B, 3, 4]; bounds: (xmin, xmax, ymin, ymax, zmin, zmax); min_views: keep a voxel seen on
    foreground by at least that many views (None: by every view).  Returns the kept voxel centres, float32 [M, 3] on `device`, in
    ascending voxel index (z fastest) -- the order in which the reference concatenates its batches; an empty hull is [0, 3].

    Differences from the reference, all in what is NOT computed differently:
      * the projection is always fp64.  The reference computes in Ps' dtype, but its own command line only ever builds fp64
        matrices; a float32 Ps is widened first, any other dtype raises ValueError;
      * the result is float32: the reference returns Ps' dtype and its main() calls .float() on it;
      * batch_size is an upper bound on the voxels per launch series, rounded down to whole blocks of 256 (at least one); the
        result does not depend on it;
      * `device` must be a HIP device: anything else raises Dm4dError, there is no CPU path."""
    P = _check_args(fmasks, Ps, voxel_size, min_views)
    axes = build_voxel_grid_linspaces(bounds, voxel_size)
    for a, name in zip(axes, "xyz"):
        if a.numel() == 0:
            raise ValueError(f"bounds: the {name} axis is empty ({name}min >= {name}max for voxel_size {voxel_size})")
    dev = _l.hip_device(device, "carve_visual_hull")
    with torch.cuda.device(dev):
        bits = ops.vhull_pack_masks(fmasks.contiguous().to(dev))  # a pageable copy on the carving stream: not overlapped
        axes = tuple(a.to(torch.float32).to(dev) for a in axes)
        return _carve(bits, tuple(fmasks.shape[1:]), P.contiguous().to(dev), axes, batch_size, min_views)


def _frame_bits(paths: Sequence[str], datas: Sequence[bytes], frm: str, dev) -> Tuple[torch.Tensor, Tuple[int, int]]:
    """The packed masks of one frame from its files' bytes, decoded on the device (host/pngdec.py): every supported mode-L file goes
    into its plane of one [B, H, W] uint8 buffer in one call, and ``dm4d_vhull_pack_masks_u8`` turns value >= 128 (load_binary_mask's
    rule) into the bits.  A file the decoder does not take (mode ``1`` files among them) or flags is decoded by load_binary_mask and its
    plane uploaded; a supported file of another mode raises load_binary_mask's ValueError from the header."""
    from . import pngdec
    plans = [pngdec.probe(d) for d in datas]
    host: Dict[int, torch.Tensor] = {}
    shapes = []
    for k, (path, plan) in enumerate(zip(paths, plans)):
        if plan is None:
            host[k] = load_binary_mask(path)
            shapes.append(tuple(host[k].shape))
        elif plan.mode != "L":
            raise ValueError(f"{path}: image mode {plan.mode!r}, expected 'L' or '1'")
        else:
            shapes.append((plan.h, plan.w))
    if len(set(shapes)) != 1:
        raise ValueError(f"fmasks_dir: the masks of frame {frm} differ in size: {sorted(set(shapes))}")
    H, W = shapes[0]
    with torch.cuda.device(dev):
        planes = torch.empty((len(paths), H, W), dtype=torch.uint8, device=dev)
        ours = [k for k, p in enumerate(plans) if p is not None]
        if ours:  # a stream the decoder refuses: load_binary_mask's pixels (or its exception)
            decode_or_fallback(pngdec, [(plans[k], datas[k], k * H * W, 1) for k in ours], planes.view(-1),
                               lambda j: (load_binary_mask(paths[ours[j]]).to(torch.uint8) * 255).numpy())
        for k, m in host.items():
            planes[k].copy_(m.to(torch.uint8) * 255)
        return ops.vhull_pack_masks_u8(planes, 128), (H, W)


def _list_labels(fmasks_dir: str, camera_range, frame_range) -> Tuple[List[str], List[str]]:
    cam_labels = sorted(os.listdir(fmasks_dir))
    if not cam_labels:
        raise ValueError(f"fmasks_dir: {fmasks_dir} holds no camera directory")
    frm_labels = [os.path.splitext(f)[0] for f in sorted(os.listdir(os.path.join(fmasks_dir, cam_labels[0])))]
    cam_labels = cam_labels[slice(*camera_range)]
    frm_labels = frm_labels[slice(*frame_range)]
    if not cam_labels or not frm_labels:
        raise ValueError(f"camera_range / frame_range: nothing selected ({len(cam_labels)} cameras, {len(frm_labels)} frames)")
    return cam_labels, frm_labels


def carve_scene(fmasks_dir: str, cameras_path: str, out_vhull_dir: str, camera_range=(0, None, 1), frame_range=(0, None, 1),
                bounds=(-3.0, 3.0, -3.0, 3.0, -3.0, 3.0), voxel_size: float = 0.025, batch_size=1e6, min_views: Optional[int] = None,
                device="cuda", sparse_pcd_path: Optional[str] = None, host_threads: int = 8, device_decode: bool = False) -> Dict:
    """Carve every selected frame of a scene (the reference's main, carve_visual_hull.py:154-231): writes
    ``out_vhull_dir/{frame}.ply`` and ``{out_vhull_dir}_bounds.json`` ([min, max] over all frames) and, with `sparse_pcd_path`, the
    first frame's cloud there as well (the ``cp`` of preprocess.sh:47).  Camera and frame labels come from the sorted listings of
    `fmasks_dir` and of its first camera; views are matched to `cameras_path` as read_projections describes.

    Frames are streamed: the masks of frame t + 1 decode in a pool of `host_threads` threads (at most 16) while frame t carves, so
    the host holds two frames of masks, not the scene's.  A frame whose hull is empty raises ValueError (the reference fails there
    inside ndarray.min).  Returns {"frames": {label: number of points}, "bounds": [min, max]}.

    device_decode: the pool prefetches the next frame's file BYTES instead of decoded masks; a frame's 8-bit PNG files are decoded on
    the device in one call and packed to bits there (_frame_bits), so no bool tensor exists and no decoded plane crosses PCIe.  The
    same files are written."""
    cam_labels, frm_labels = _list_labels(fmasks_dir, camera_range, frame_range)
    P = read_projections(cameras_path, cam_labels)
    dev = _l.hip_device(device, "carve_visual_hull")
    threads = max(1, min(int(host_threads), MAX_HOST_THREADS))

    def paths(frm: str) -> List[str]:
        return [os.path.join(fmasks_dir, cam, f"{frm}.png") for cam in cam_labels]

    fetch = read_file if device_decode else load_binary_mask

    def carve_bits(frm: str, datas) -> torch.Tensor:
        """carve_visual_hull from the frame's file bytes: the same checks, grid and launches, the bits made on the device"""
        Pd = _check_args(torch.zeros((P.shape[0], 1, 1), dtype=torch.bool), P, voxel_size, min_views)
        axes = build_voxel_grid_linspaces(bounds, voxel_size)
        for a, name in zip(axes, "xyz"):
            if a.numel() == 0:
                raise ValueError(f"bounds: the {name} axis is empty ({name}min >= {name}max for voxel_size {voxel_size})")
        bits, hw = _frame_bits(paths(frm), datas, frm, dev)
        with torch.cuda.device(dev):
            axes = tuple(a.to(torch.float32).to(dev) for a in axes)
            return _carve(bits, hw, Pd.contiguous().to(dev), axes, batch_size, min_views)

    lows, highs = [], []  # per frame: the corners of its cloud's box
    counts: Dict[str, int] = {}
    with ThreadPoolExecutor(max_workers=threads, thread_name_prefix="dm4d-vhull") as pool:
        pending = [pool.submit(fetch, p) for p in paths(frm_labels[0])]
        for i, frm in enumerate(frm_labels):
            masks = [f.result() for f in pending]
            if i + 1 < len(frm_labels):
                pending = [pool.submit(fetch, p) for p in paths(frm_labels[i + 1])]
            if device_decode:
                pts = carve_bits(frm, masks).cpu().numpy()
            else:
                shapes = {tuple(m.shape) for m in masks}
                if len(shapes) != 1:
                    raise ValueError(f"fmasks_dir: the masks of frame {frm} differ in size: {sorted(shapes)}")
                pts = carve_visual_hull(torch.stack(masks), P, bounds, voxel_size=voxel_size, batch_size=batch_size, min_views=min_views,
                                        device=dev).cpu().numpy()
            if len(pts) == 0:
                raise ValueError(f"frame {frm}: the visual hull is empty; enlarge bounds or lower min_views")
            save_pcd_ply(os.path.join(out_vhull_dir, f"{frm}.ply"), pts)
            if i == 0 and sparse_pcd_path:
                save_pcd_ply(sparse_pcd_path, pts)
            counts[frm] = len(pts)
            lows.append(pts.min(axis=0))
            highs.append(pts.max(axis=0))
    result = [np.min(lows, axis=0).astype(np.float64).tolist(), np.max(highs, axis=0).astype(np.float64).tolist()]
    with open(f"{out_vhull_dir}_bounds.json", "w") as f:
        json.dump(result, f)
    return {"frames": counts, "bounds": result}
