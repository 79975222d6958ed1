"""Constructed inputs for the plan kernel (tests/test_skel_plan_cpu.py, tests/test_skel_plan_gpu.py) and the file-route oracle they are
held against: project -> triang.write_kp2d -> skeleton._read_instance -> plan_draw_calls -> pack_calls.

A case is one map: a 133-keypoint pose and one camera, built so that the projection lands on chosen fp32 values.  The camera is
K = diag(f, f, 1), T = identity: u = f X / (Z + 1e-9), depth = Z exactly, so a pose with X = u (Z + 1e-9) / f projects within an ulp
of fp64 of u, and rounds to u exactly in fp32 when u is an fp32 number (every builder asserts that on the model's projection).
"""
import copy
import json
from pathlib import Path
from typing import NamedTuple, Optional

import numpy as np

import triang_model
from diffuman4d_amd.host import skeleton, triang

PALETTE_PATH = Path(__file__).resolve().parent / "golden" / "skel_palette.json"
PALETTE_DATA = json.loads(PALETTE_PATH.read_text())
PALETTE = skeleton.make_palette(PALETTE_DATA)
K_PTS = len(PALETTE.keypoint_colors)
SQUARE = ((1024, 1024), (256, 256))       # scale_ratio 2, offset 0: a coordinate of x.25 lands on .5
WIDE = ((1024, 1024), (320, 256))         # canvas 2048 x 1638, scale_ratio 1638 / 1024
FOCAL = 1.0
K_FLAT = np.diag([FOCAL, FOCAL, 1.0])
T_FLAT = np.eye(4)
LINKS = skeleton.plan_links(PALETTE)


class Case(NamedTuple):
    name: str
    kp3d: np.ndarray                  # fp64 [k, 3]
    scores: Optional[np.ndarray]      # fp32 [k] or None
    shapes: tuple
    palette: skeleton.Palette
    error: Optional[str]              # the ValueError text plan_draw_calls raises, or None


def pose(uv, z) -> np.ndarray:
    """The pose that the flat camera projects onto uv (fp32 numbers) at depth z, checked on the model's projection."""
    uv, z = np.asarray(uv, np.float32).astype(np.float64), np.broadcast_to(np.asarray(z, np.float64), (len(uv),))
    kp3d = np.concatenate([uv * (z[:, None] + 1e-9) / FOCAL, z[:, None]], axis=1)
    got_uv, got_z = project(kp3d)
    assert np.array_equal(got_uv.astype(np.float32), uv.astype(np.float32)) and np.array_equal(got_z, z)
    return kp3d


def project(kp3d):
    with np.errstate(all="ignore"):
        uv, depth = triang_model.project(kp3d[None], K_FLAT[None], T_FLAT[None])
    return uv[0, 0], depth[0, 0]


def base_uv(rng) -> np.ndarray:
    return rng.uniform(100, 900, (K_PTS, 2)).astype(np.float32)


def with_colourless(index: int) -> skeleton.Palette:
    data = copy.deepcopy(PALETTE_DATA)
    data["keypoint_colors"][index] = None
    return skeleton.make_palette(data)


def cases():
    rng = np.random.default_rng(2024)
    out = []
    for seed in range(3):  # random poses, a tenth of the keypoints not triangulated
        kp3d = pose(base_uv(rng), rng.uniform(2, 4, K_PTS))
        kp3d[rng.random(K_PTS) < 0.1] = -1e6
        out.append(Case(f"random{seed}", kp3d, None, SQUARE if seed != 1 else WIDE, PALETTE, None))
    out.append(Case("score_override", pose(base_uv(rng), rng.uniform(2, 4, K_PTS)), rng.uniform(0, 1, K_PTS).astype(np.float32), SQUARE, PALETTE, None))
    # equal link depths: three depth values only, so that many links tie and stability decides
    out.append(Case("equal_depths", pose(base_uv(rng), rng.choice([2.0, 2.5, 3.0], K_PTS)), None, SQUARE, PALETTE, None))
    out.append(Case("one_depth", pose(base_uv(rng), 3.0), None, WIDE, PALETTE, None))
    # all depths zero: list order with scores of 1, ascending line score (with ties) otherwise
    out.append(Case("zero_depths", pose(base_uv(rng), 0.0), None, SQUARE, PALETTE, None))
    out.append(Case("zero_depths_scores", pose(base_uv(rng), 0.0), rng.choice([0.6, 0.75, 1.0], K_PTS).astype(np.float32), SQUARE, PALETTE, None))
    # scaled coordinates exactly on .5: half to even, both parities
    uv = base_uv(rng)
    uv[:, 0] = np.floor(uv[:, 0]) + rng.choice([0.25, 0.75], K_PTS)
    uv[:, 1] = np.floor(uv[:, 1]) + rng.choice([0.25, 0.75, 0.0], K_PTS)
    out.append(Case("half_landings", pose(uv, rng.uniform(2, 4, K_PTS)), None, SQUARE, PALETTE, None))
    # scores exactly at the thresholds (as fp32), just below and just above
    at = np.array([0.5, 0.9, np.nextafter(np.float32(0.5), np.float32(0)), np.nextafter(np.float32(0.9), np.float32(1)), 1.0, 0.7], np.float32)
    out.append(Case("threshold_scores", pose(base_uv(rng), rng.uniform(2, 4, K_PTS)), rng.choice(at, K_PTS), SQUARE, PALETTE, None))
    # a point behind the camera: negative depth; where u or v turns negative the score is 0
    z = rng.uniform(2, 4, K_PTS)
    z[[5, 7, 9, 100]] = -2.0
    kp3d = pose(base_uv(rng), np.abs(z))
    kp3d[:, 2] = z
    out.append(Case("behind_camera", kp3d, None, SQUARE, PALETTE, None))
    # ... and where both stay positive (the point is mirrored through the centre) the link is drawn, with its negative depth as sort key
    out.append(Case("behind_camera_positive_uv", pose(base_uv(rng), np.where(np.isin(np.arange(K_PTS), [5, 7, 9, 100]), -2.0, 3.0)), None, SQUARE, PALETTE, None))
    # an endpoint outside [-8192, 8191] on the canvas: dropped and counted
    uv = base_uv(rng)
    uv[[6, 11, 95]] = (5000.0, 300.0)
    uv[12] = (300.0, 4096.0)       # 8192: one past the range
    uv[13] = (4095.5, 300.0)       # 8191: the last one inside
    out.append(Case("outside", pose(uv, rng.uniform(2, 4, K_PTS)), None, SQUARE, PALETTE, None))
    # a NaN keypoint on a kept link raises; on a link dropped by its score it does not
    kp3d = pose(base_uv(rng), rng.uniform(2, 4, K_PTS))
    kp3d[9, 0] = np.nan
    out.append(Case("nan_kept", kp3d, None, SQUARE, PALETTE, "a keypoint of a drawn link is not finite"))
    scores = np.ones(K_PTS, np.float32)
    scores[9] = 0.0
    out.append(Case("nan_dropped", kp3d, scores, SQUARE, PALETTE, None))
    # a keypoint without a colour: the first kept link that joins it is named; none is when its links are dropped
    i1, i2 = LINKS[3]["link"]
    first = next(l for l in LINKS if i1 in l["link"])
    text = f"palette: link {first['id']} joins keypoints {first['link'][0]} and {first['link'][1]}, one of which has no colour"
    kp3d = pose(base_uv(rng), rng.uniform(2, 4, K_PTS))
    out.append(Case("colourless", kp3d, None, SQUARE, with_colourless(i1), text))
    scores = np.ones(K_PTS, np.float32)
    scores[i1] = 0.25
    out.append(Case("colourless_dropped", kp3d, scores, SQUARE, with_colourless(i1), None))
    return out


def file_route(case: Case, tmp: Path, projected=None):
    """-> (records int32 [n, 8], dropped links) of the file route, or the ValueError it raises.  `projected`: (uv, depth) from the
    device's projection; by default the model's."""
    uv, depth = project(case.kp3d) if projected is None else projected
    triang.write_kp2d(tmp / "kp.json", uv, depth)
    score = None
    if case.scores is not None:
        triang.write_kp2d(tmp / "score.json", uv, None, case.scores)
        score = skeleton._read_instance(tmp / "score.json")
    try:
        plan = skeleton.plan_draw_calls(skeleton._read_instance(tmp / "kp.json"), score, case.shapes, case.palette)
    except ValueError as e:
        return e
    return skeleton.pack_calls(plan.calls), plan.dropped_links
