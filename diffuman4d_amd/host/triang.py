"""Skeleton triangulation: 3-D keypoints from a scene's per-view 2-D keypoints and cameras (``poses_3d/{frame}.json``) and their
re-projection with depths into every camera (``poses_2d/{cam}/{frame}.json``, what skeleton drawing consumes).

The reference's ``scripts/preprocess/triangulate_skeleton.py`` and ``scripts/preprocess/utils/triang_utils.py`` (the
``triangulate_skeleton`` action of ``preprocess.sh``) with the same function names and arguments, built from their behaviour.  The
reference solves one keypoint at a time -- an SVD and a ``scipy.optimize.least_squares(method="trf", loss="huber")`` each, in a Python
loop; here every (frame, keypoint) of a scene is one wave of one launch (``dm4d_triangulate_points_f64``), and the projection into
the cameras is a second launch (``dm4d_project_points_f64``).  The host reads and writes the JSON files in a thread pool, builds the
cameras in the reference's float32 arithmetic and computes the per-keypoint score threshold with numpy's own ``np.percentile``.
There is no CPU path: a ``device`` that is not a HIP device is an error.
"""
from __future__ import annotations

import json
import os
import time
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import lib as _l
from . import ops
from .capture import read_cameras
from .staging import MAX_HOST_THREADS  # noqa: F401  (importable from here as before)
from .vhull import save_pcd_ply

INVALID = -1e6
MAX_VIEWS = 24            # triangulate_one_point's max_views default, which triangulate_points never overrides
LAUNCH_BYTES = 1 << 28    # the frame axis is cut so that one launch's kp2d + score stay below this


_hip_device = _l.hip_device


# -- the two operations ---------------------------------------------------------------------------------------------------------------
def score_thresholds(kp2d_score: np.ndarray, score_thr: float = 0.6, max_views: int = MAX_VIEWS) -> np.ndarray:
    """kp2d_score [..., n, k] -> [..., k]: the threshold a view's score must reach for each keypoint, ``max(score_thr, percentile)``
    with the percentile that keeps about `max_views` of the n views (triang_utils.py:63-71), by numpy's own np.percentile over the
    view axis, so that its interpolation is the reference's and is not re-derived."""
    n = kp2d_score.shape[-2]
    max_views = min(max_views, n)
    return np.maximum(score_thr, np.percentile(kp2d_score, 100 * (1 - max_views / n), axis=-2))


def triangulate_points(Ks, Ts, kp2d, kp2d_score=None, min_views=3, score_thr=0.6, device="cuda"):
    """Triangulate every keypoint from its views (triang_utils.py:129-175).

    Ks (n, 3, 3), Ts (n, 4, 4) world -> camera, kp2d (n, k, 2), kp2d_score (n, k) or None (all ones) -> kp3d (k, 3), reproj (k,),
    n_views (k,), numpy like the reference's.  A keypoint that fewer than `min_views` views see with a score of at least
    max(score_thr, the percentile that keeps 24 views) is -1e6 in kp3d and reproj.  kp2d (F, n, k, 2) with kp2d_score (F, n, k) does F
    frames in the same launch and returns (F, k, 3), (F, k), (F, k); a frame's result does not depend on the others.

    Differences from the reference: n_views is int32 (the reference returns the counts in a float array); the minimiser of the Huber
    cost is iterated to fp64 convergence where the reference stops at scipy's 1e-8 tolerances, so the points agree to the reference's
    own distance from that minimiser (about 1e-8 m); `device` must be a HIP device (Dm4dError otherwise)."""
    Ks, Ts, kp2d = np.asarray(Ks), np.asarray(Ts), np.asarray(kp2d)
    batched = kp2d.ndim == 4
    if kp2d_score is None:
        kp2d_score = np.ones(kp2d.shape[:-1], dtype=np.float64)
    kp2d_score = np.asarray(kp2d_score)
    n, k, _ = kp2d.shape[1:] if batched else kp2d.shape
    lead = kp2d.shape[:1] if batched else ()
    if min_views < 3:
        raise ValueError(f"min_views should be at least 3, got {min_views}.")
    if kp2d.shape != lead + (n, k, 2):
        raise ValueError(f"kp2d must have shape (n, k, 2), got {kp2d.shape}")
    if kp2d_score.shape != lead + (n, k):
        raise ValueError(f"kp2d_score must have shape (n, k), got {kp2d_score.shape}")
    if Ks.shape != (n, 3, 3):
        raise ValueError(f"Ks must have shape (n, 3, 3), got {Ks.shape}")
    if Ts.shape != (n, 4, 4):
        raise ValueError(f"Ts must have shape (n, 4, 4), got {Ts.shape}")
    if score_thr is None:
        raise ValueError("score_thr must be a number (the reference's triangulate_points fails without one)")
    if n > ops.TRIANG_MAX_VIEWS or k < 1 or (batched and lead[0] < 1):
        raise ValueError(f"kp2d: between 1 and {ops.TRIANG_MAX_VIEWS} views and at least one keypoint and frame, got {kp2d.shape}")
    dev = _hip_device(device, "triangulate_points")
    kp2d = np.ascontiguousarray(kp2d, dtype=np.float64).reshape(-1, n, k, 2)
    score = np.ascontiguousarray(kp2d_score, dtype=np.float64).reshape(-1, n, k)
    thr = score_thresholds(score, score_thr)
    F = kp2d.shape[0]
    step = max(1, LAUNCH_BYTES // (n * k * 24))
    outs = []
    with torch.cuda.device(dev):
        K_d = torch.from_numpy(np.ascontiguousarray(Ks, dtype=np.float64)).to(dev)
        T_d = torch.from_numpy(np.ascontiguousarray(Ts, dtype=np.float64)).to(dev)
        for f0 in range(0, F, step):
            sl = slice(f0, min(F, f0 + step))
            outs.append(ops.triangulate_points(K_d, T_d, torch.from_numpy(kp2d[sl]).to(dev), torch.from_numpy(score[sl]).to(dev),
                                               torch.from_numpy(np.ascontiguousarray(thr[sl])).to(dev), int(min_views)))
        kp3d, reproj, n_views = (torch.cat([o[i] for o in outs]).cpu().numpy() for i in range(3))
    return (kp3d, reproj, n_views) if batched else (kp3d[0], reproj[0], n_views[0])


def _face_normal(kp3d: np.ndarray) -> np.ndarray:
    nose, left_eye, right_eye = kp3d[:3]
    eye_mid = (left_eye + right_eye) / 2
    normal = np.cross(right_eye - left_eye, nose - eye_mid)
    normal /= np.linalg.norm(normal)
    return normal


def project_points(kp3d, Ks, Ts, kp3d_score=None, device="cuda"):
    """Project the 3-D keypoints into every camera (triang_utils.py:20-50).

    kp3d (k, 3), Ks (m, 3, 3), Ts (m, 4, 4) -> kp2d (m, k, 2), depth (m, k) (the third homogeneous coordinate) and kp2d_score (m, k)
    or None; a point with a coordinate equal to -1e6 gives -1e6 in kp2d and depth for every camera.  With kp3d_score (k,) the scores
    are repeated per camera and those of the face (keypoints 0-2 and 23-90) are scaled by how far the face, by the normal of nose and
    eyes, turns towards the camera -- on the host, as the reference does.  kp3d (F, k, 3) (with kp3d_score (F, k) or (k,)) does F
    frames in one launch and returns (F, m, k, 2), (F, m, k), (F, m, k)."""
    kp3d, Ks, Ts = np.asarray(kp3d, dtype=np.float64), np.asarray(Ks), np.asarray(Ts)
    batched = kp3d.ndim == 3
    if kp3d.ndim not in (2, 3) or kp3d.shape[-1] != 3 or kp3d.size == 0:
        raise ValueError(f"kp3d must have shape (k, 3), got {kp3d.shape}")
    m = Ks.shape[0]
    if Ks.shape != (m, 3, 3) or m < 1:
        raise ValueError(f"Ks must have shape (n, 3, 3), got {Ks.shape}")
    if Ts.shape != (m, 4, 4):
        raise ValueError(f"Ts must have shape (n, 4, 4), got {Ts.shape}")
    dev = _hip_device(device, "project_points")
    pts = np.ascontiguousarray(kp3d).reshape(-1, kp3d.shape[-2], 3)
    F, k, _ = pts.shape
    with torch.cuda.device(dev):
        uv, depth = ops.project_points(torch.from_numpy(pts).to(dev), torch.from_numpy(np.ascontiguousarray(Ks, dtype=np.float64)).to(dev),
                                       torch.from_numpy(np.ascontiguousarray(Ts, dtype=np.float64)).to(dev))
        uv, depth = uv.cpu().numpy(), depth.cpu().numpy()
    score = None
    if kp3d_score is not None:
        kp3d_score = np.broadcast_to(np.asarray(kp3d_score), (F, k))
        score = np.repeat(kp3d_score[:, None, :], m, axis=1)
        for f in range(F):
            face_cam_score = -np.dot(Ts[:, 2, :3], _face_normal(pts[f])) * 0.5 + 0.5
            score[f, :, :3] *= face_cam_score[:, None]
            score[f, :, 23:91] *= face_cam_score[:, None]
    if batched:
        return uv, depth, score
    return uv[0], depth[0], None if score is None else score[0]


# -- files ----------------------------------------------------------------------------------------------------------------------------
def read_kp2d(path, dtype=np.float64):
    """A keypoint file -> (keypoints (k, 2), keypoint_depths (k,) or None, keypoint_scores (k,)) of ``instance_info[0]``, the finger
    scores scaled by the square of their hand root's score as the reference does (triangulate_skeleton.py:15-30; 91 and 112 are the
    hand roots of the 133-keypoint layout).  A file without ``keypoint_scores`` raises ValueError (the reference fails there with a
    TypeError)."""
    with open(path, "r") as f:
        pose = json.load(f)
    instance = pose["instance_info"][0]
    kp = np.array(instance["keypoints"], dtype=dtype)
    kp_depth = np.array(instance["keypoint_depths"], dtype=dtype) if "keypoint_depths" in instance else None
    if "keypoint_scores" not in instance:
        raise ValueError(f"{path}: no keypoint_scores")
    kp_score = np.array(instance["keypoint_scores"], dtype=dtype)
    kp_score[92:112] *= kp_score[91] ** 2
    kp_score[113:133] *= kp_score[112] ** 2
    return kp, kp_depth, kp_score


def _write_instance(path, instance: Dict) -> None:
    parent = os.path.dirname(path)
    if parent:
        os.makedirs(parent, exist_ok=True)
    with open(path, "w") as f:
        json.dump({"instance_info": [instance]}, f, indent=4)


def write_kp2d(path, kp, kp_depth=None, kp_score=None) -> None:
    """``{"instance_info": [{"keypoints", "keypoint_depths"?, "keypoint_scores"?}]}`` with indent=4 (triangulate_skeleton.py:33-42)."""
    instance = {"keypoints": kp.tolist()}
    if kp_depth is not None:
        instance["keypoint_depths"] = kp_depth.tolist()
    if kp_score is not None:
        instance["keypoint_scores"] = kp_score.tolist()
    _write_instance(path, instance)


def write_kp3d(path, kp3d, kp3d_reproj) -> None:
    """``{"instance_info": [{"keypoints", "keypoint_reproj"}]}`` with indent=4 (triangulate_skeleton.py:45-53)."""
    _write_instance(path, {"keypoints": kp3d.tolist(), "keypoint_reproj": kp3d_reproj.tolist()})


# -- a scene --------------------------------------------------------------------------------------------------------------------------
def _labels(labels, label_range, name: str, range_name: str, width: int, listing) -> List[str]:
    if labels is not None:
        if label_range is not None:
            raise ValueError(f"{name} and {range_name} cannot be specified together")
        return [f"{int(i):0{width}d}" for i in labels]
    if label_range is not None:
        b, e, s = label_range
        return [f"{int(i):0{width}d}" for i in range(b, e, s)]
    return listing()


def scene_cameras(camera_path: str, labels: Sequence[str], intri_scale: Optional[float] = None) -> Tuple[np.ndarray, np.ndarray]:
    """-> fp64 Ks [n, 3, 3], Ts [n, 4, 4] of the labelled cameras exactly as the reference builds them (triangulate_skeleton.py:116-127):
    parse_cameras(coord_system="opencv", normalize_scene=False) gives float32 K and camera-to-world pose; the pose is inverted in
    float32 and both are widened; intri_scale multiplies K and resets K[2, 2] = 1."""
    cams = read_cameras(camera_path, normalize_scene=False)
    missing = [c for c in labels if c not in cams]
    if missing:
        raise ValueError(f"camera_path: {camera_path} has no camera_label {missing} (it lists {sorted(cams)})")
    Ks = np.array([cams[c]["K"].numpy() for c in labels], dtype=np.float64)
    Ts = np.array([np.linalg.inv(cams[c]["pose"].numpy()) for c in labels], dtype=np.float64)
    if intri_scale is not None:
        Ks = Ks * intri_scale
        Ks[:, -1, -1] = 1.0
    return Ks, Ts


def triangulate_skeleton(camera_path: str, kp2d_dir: str, out_kp3d_dir: str, out_pcd_dir: Optional[str] = None,
                         out_kp2d_proj_dir: Optional[str] = None, spa_label_range=None, spa_label_proj_range=None, tem_label_range=None,
                         spa_labels=None, spa_labels_proj=None, tem_labels=None, kp2d_padding=None, intri_scale: Optional[float] = None,
                         skip_exists: bool = False, num_workers: int = 8, device="cuda") -> Dict:
    """Triangulate every selected frame of a scene (triangulate_skeleton.py:65-178): reads ``kp2d_dir/{cam}/{frame}.json`` of the
    cameras `spa_labels`, writes ``out_kp3d_dir/{frame}.json`` and, when the directories are given, ``out_pcd_dir/{frame}.ply`` and
    ``out_kp2d_proj_dir/{cam}/{frame}.json`` for the cameras `spa_labels_proj`.  Labels are given as lists of integers, as
    (begin, end, step) ranges, or default to the sorted listings of `kp2d_dir` and of its first camera, as in the reference.

    The files are read in a pool of `num_workers` threads (at most 16), all frames are triangulated in one launch and projected in a
    second one (the frame axis is cut only where a launch's inputs would pass 256 MiB), and the files are then written from the
    same pool.  With `skip_exists` a frame whose ``out_kp3d_dir`` file exists and parses is left alone with all its outputs.
    fp64 throughout (the reference's `dtype` argument is not taken).  ``out_pcd_dir`` receives the k points of a frame, invalid ones
    included as the reference does, through vhull.save_pcd_ply: float32 x, y, z and white colours -- NOT the byte layout of
    Open3D's writer, which the reference uses (Open3D is not a dependency here, and nothing downstream reads these files).
    Returns counts: frames, skipped, cameras, cameras_proj, keypoints, valid (triangulated keypoints), files, and the wall-clock
    seconds of the three phases (read; launch = uploads, the two launches and the downloads; write)."""
    spa_labels = _labels(spa_labels, spa_label_range, "spa_labels", "spa_label_range", 2, lambda: sorted(os.listdir(kp2d_dir)))
    spa_labels_proj = _labels(spa_labels_proj, spa_label_proj_range, "spa_labels_proj", "spa_label_proj_range", 2,
                              lambda: sorted(os.listdir(kp2d_dir)))
    tem_labels = _labels(tem_labels, tem_label_range, "tem_labels", "tem_label_range", 6,
                         lambda: [label.split(".")[0] for label in sorted(os.listdir(f"{kp2d_dir}/{spa_labels[0]}"))])
    Ks, Ts = scene_cameras(camera_path, spa_labels, intri_scale)
    Ks_proj, Ts_proj = scene_cameras(camera_path, spa_labels_proj, intri_scale)
    dev = _hip_device(device, "triangulate_skeleton")

    todo, skipped = [], 0
    for tem in tem_labels:
        path = f"{out_kp3d_dir}/{tem}.json"
        if skip_exists and os.path.exists(path):
            try:
                with open(path, "r") as f:
                    json.load(f)
                skipped += 1
                continue
            except Exception as e:
                print(f"Error loading {path}: {e}, skipping...")
        todo.append(tem)
    counts = {"frames": len(todo), "skipped": skipped, "cameras": len(spa_labels), "cameras_proj": len(spa_labels_proj) if out_kp2d_proj_dir else 0,
              "keypoints": 0, "valid": 0, "files": 0}
    if not todo:
        return counts

    with ThreadPoolExecutor(max_workers=max(1, min(int(num_workers), MAX_HOST_THREADS)), thread_name_prefix="dm4d-triang") as pool:
        t0 = time.perf_counter()
        paths = [f"{kp2d_dir}/{spa}/{tem}.json" for tem in todo for spa in spa_labels]
        read = list(pool.map(read_kp2d, paths))
        shapes = {(kp.shape, sc.shape) for kp, _, sc in read}
        if len(shapes) != 1:
            raise ValueError(f"kp2d_dir: the keypoint files differ in shape: {sorted(shapes)}")
        F, n = len(todo), len(spa_labels)
        kp2d = np.stack([kp for kp, _, _ in read]).reshape(F, n, -1, 2)
        score = np.stack([sc for _, _, sc in read]).reshape(F, n, -1)
        del read
        if kp2d_padding is not None:
            kp2d += np.array(kp2d_padding, dtype=np.float64)[None]
        t1 = time.perf_counter()
        kp3d, reproj, n_views = triangulate_points(Ks, Ts, kp2d, score, device=dev)
        uv = depth = None
        if out_kp2d_proj_dir is not None:
            uv, depth, _ = project_points(kp3d, Ks_proj, Ts_proj, device=dev)
        t2 = time.perf_counter()
        jobs = [(write_kp3d, (f"{out_kp3d_dir}/{tem}.json", kp3d[f], reproj[f])) for f, tem in enumerate(todo)]
        if out_pcd_dir is not None:
            jobs += [(save_pcd_ply, (f"{out_pcd_dir}/{tem}.ply", kp3d[f])) for f, tem in enumerate(todo)]
        if out_kp2d_proj_dir is not None:
            jobs += [(write_kp2d, (f"{out_kp2d_proj_dir}/{spa}/{tem}.json", uv[f, c], depth[f, c]))
                     for f, tem in enumerate(todo) for c, spa in enumerate(spa_labels_proj)]
        list(pool.map(lambda job: job[0](*job[1]), jobs))
        t3 = time.perf_counter()
    counts.update(keypoints=int(kp3d.shape[1]), valid=int((n_views >= 3).sum()), files=len(jobs),
                  seconds={"read": round(t1 - t0, 4), "launch": round(t2 - t1, 4), "write": round(t3 - t2, 4)})
    return counts
