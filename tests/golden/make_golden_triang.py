#!/usr/bin/env python
"""The skeleton-triangulation fixture of tests/test_triang_cpu.py and tests/test_triang_gpu.py.

  python tests/golden/make_golden_triang.py --scene   writes tests/golden/triang_scene/{ring8,ring30}/: a transforms.json (cameras on
                                                      a ring with distinct intrinsics, camera_label) and
                                                      poses_sapiens/{cam}/{frame}.json with 133 keypoints each: projections of a
                                                      synthetic body with Gaussian pixel noise, a few gross outliers and varied
                                                      scores.  ring8: 8 cameras x 2 frames; ring30: 30 cameras x 1 frame
  python tests/golden/make_golden_triang.py           runs the REFERENCE's scripts/preprocess/triangulate_skeleton.py and
                                                      scripts/preprocess/utils/triang_utils.py, imported unmodified, on the CPU and
                                                      records triang_reference.pt: triangulate_skeleton(...) on both scenes (the
                                                      parsed JSON values and the Ks, Ts it built), triangulate_points(...) per case of
                                                      CASES and project_points(...) of recorded points

Stand-ins go into sys.modules for what the reference imports and this machine lacks: fire and easyvolcap (tqdm and
parallel_execution become a plain loop).  open3d is only imported by the reference's point-cloud writer, which is not called.

Accuracy.  The reference stops at scipy's 1e-8 tolerances after at most 50 evaluations, so it is only near the minimiser of its
own cost.  For every valid keypoint this script therefore also solves the same Huber problem with scipy at ftol = xtol = gtol =
1e-15 (analytic Jacobian, a large max_nfev), once from the reference's result and once from the linear start.  scipy accepts a step
only if the cost, a sum of magnitude F, is seen to fall, so it stalls where the fall drops below F's rounding (steps of about
1e-10 m, gradients of 1e-5 left): each solve is therefore polished by Newton steps on the gradient of the same cost, which is
accurate far below that, and asserted to move by less than 1e-8 m.  Stored per case:
  d_ref  = max |reference - converged|      (3-D point: the Euclidean distance in metres; reproj: pixels)
  d_conv = max |converged_a - converged_b|
It asserts that the two converged solves agree (d_conv <= 1e-3 d_ref, or below 1e-12 m) and that d_ref <= 1e-6 m.  The tests
hold the numpy model and the kernels to |x - converged| <= d_ref + d_conv.  If a scene constant breaks an assertion, change the
constant, not the assertion.
"""
from __future__ import annotations

import importlib.util
import json
import math
import sys
import tempfile
import time
import types
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
OUT = Path(__file__).resolve().parent
SCENE_DIR = OUT / "triang_scene"
K_POINTS = 133
IMG = 1024
SCENES = {"ring8": (8, 2), "ring30": (30, 1)}  # name -> (cameras, frames)


# -- synthetic scene --------------------------------------------------------------------------------------------------------------
def body(k: int, seed: int, t: int = 0) -> np.ndarray:
    """k points in a standing body's box (x +-0.4, y -0.9 .. 0.8, z +-0.25), moved a little with the frame t."""
    rng = np.random.default_rng(seed)
    p = rng.uniform([-0.4, -0.9, -0.25], [0.4, 0.8, 0.25], size=(k, 3))
    return p + t * np.array([0.05, 0.01, -0.03])


def ring(n: int, span: float = 2 * math.pi, phase: float = 0.3):
    """-> list of (label, fl_x, fl_y, cx, cy, camera-to-world 4 x 4 in OpenGL axes, rounded to 6 decimals as the file stores it)."""
    out = []
    for c in range(n):
        a = span * c / n + phase
        o = np.array([2.8 * math.cos(a), 0.1 + 0.25 * math.sin(2 * a), 2.8 * math.sin(a)])
        back = o / np.linalg.norm(o)  # OpenGL: the camera looks down -z
        right = np.cross([0.0, 1.0, 0.0], back)
        right /= np.linalg.norm(right)
        up = np.cross(back, right)
        m = np.eye(4)
        m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = right, up, back, o
        m = np.array([[round(float(v), 6) for v in row] for row in m])
        out.append((f"{c:02d}", 1100.0 + 7.5 * (c % 11), 1104.25 + 6.5 * (c % 7), 509.3 + 1.45 * (c % 5), 515.6 - 1.35 * (c % 9), m))
    return out


def camera_matrices(cams):
    """fp64 K [n, 3, 3] and world -> camera T [n, 4, 4] (OpenCV axes) of a ring() list."""
    Ks, Ts = [], []
    for _, fx, fy, cx, cy, m in cams:
        Ks.append(np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]]))
        c2w = m.copy()
        c2w[:3, 1:3] *= -1
        Ts.append(np.linalg.inv(c2w))
    return np.stack(Ks), np.stack(Ts)


def observe(Ks, Ts, pts, rng, sigma: float, n_outliers: int = 0):
    """pts [k, 3] -> kp2d [n, k, 2]: the projections + Gaussian noise; n_outliers keypoints get 20 - 60 px in one or two views."""
    n, k = len(Ks), len(pts)
    P = Ks @ Ts[:, :3]
    h = np.einsum("nrc,kc->nkr", P[:, :, :3], pts) + P[:, None, :, 3]
    uv = h[..., :2] / h[..., 2:3]
    uv = uv + sigma * rng.standard_normal(uv.shape)
    for i in rng.choice(k, size=n_outliers, replace=False):
        for j in rng.choice(n, size=int(rng.integers(1, 3)), replace=False):
            ang = rng.uniform(0, 2 * math.pi)
            uv[j, i] += rng.uniform(20, 60) * np.array([math.cos(ang), math.sin(ang)])
    return uv


def write_scene() -> None:
    for name, (n, frames) in SCENES.items():
        cams = ring(n)
        Ks, Ts = camera_matrices(cams)
        rng = np.random.default_rng(100 + n)
        tf = [{"camera_label": lab, "file_path": f"images/{lab}/000000.webp", "h": IMG, "w": IMG, "fl_x": fx, "fl_y": fy, "cx": cx, "cy": cy,
               "transform_matrix": m.tolist()} for lab, fx, fy, cx, cy, m in cams]
        d = SCENE_DIR / name
        d.mkdir(parents=True, exist_ok=True)
        (d / "transforms.json").write_text(json.dumps({"w": IMG, "h": IMG, "frames": tf}, indent=1))
        for t in range(frames):
            uv = observe(Ks, Ts, body(K_POINTS, 7, t), rng, sigma=1.0, n_outliers=12)
            score = rng.uniform(0.45, 1.0, size=(n, K_POINTS))
            score[:, 91] = rng.uniform(0.93, 1.0, size=n)    # left hand root: its fingers keep most of their score
            score[:, 112] = rng.uniform(0.45, 0.6, size=n)   # right hand root: its fingers fall below the threshold -> INVALID
            for j, (lab, *_rest) in enumerate(cams):
                inst = {"keypoints": [[round(float(u), 2), round(float(v), 2)] for u, v in uv[j]],
                        "keypoint_scores": [round(float(s), 3) for s in score[j]]}
                p = d / "poses_sapiens" / lab / f"{t:06d}.json"
                p.parent.mkdir(parents=True, exist_ok=True)
                p.write_text(json.dumps({"instance_info": [inst]}, separators=(",", ":")))


# -- in-memory cases --------------------------------------------------------------------------------------------------------------
def build_cases():
    """-> list of {"name", "Ks", "Ts", "kp2d" [n, k, 2], "score" [n, k]}."""
    cases = []

    def add(name, Ks, Ts, kp2d, score):
        cases.append({"name": name, "Ks": Ks, "Ts": Ts, "kp2d": np.ascontiguousarray(kp2d), "score": np.ascontiguousarray(score)})

    K8, T8 = camera_matrices(ring(8))
    pts = body(K_POINTS, 11)

    rng = np.random.default_rng(1)  # exactly min_views views, every score >= 0.6: the threshold is the smallest score
    K3, T3 = camera_matrices(ring(3, span=2.2))
    add("n3_min_views", K3, T3, observe(K3, T3, pts, rng, 0.7), rng.uniform(0.6, 1.0, size=(3, K_POINTS)))

    rng = np.random.default_rng(2)  # Huber's linear branch
    add("n8_outliers", K8, T8, observe(K8, T8, pts, rng, 1.0, n_outliers=40), rng.uniform(0.62, 1.0, size=(8, K_POINTS)))

    rng = np.random.default_rng(3)  # quadratic branch only, reproj ~ 0
    add("n8_clean", K8, T8, observe(K8, T8, pts, rng, 0.0), rng.uniform(0.62, 1.0, size=(8, K_POINTS)))

    rng = np.random.default_rng(4)  # keypoint i keeps 2, 3 or 8 views (i % 3): INVALID and n_views
    score = rng.uniform(0.62, 1.0, size=(8, K_POINTS))
    for i in range(K_POINTS):
        keep = (2, 3, 8)[i % 3]
        drop = rng.permutation(8)[keep:]
        score[drop, i] = rng.uniform(0.1, 0.55, size=len(drop))
    add("n8_views_2_3_8", K8, T8, observe(K8, T8, pts, rng, 0.8), score)

    rng = np.random.default_rng(5)  # camera 2's principal point lies far left: points on its left project to u < 0 with a high score
    Kn = K8.copy()
    Kn[2, 0, 2] = 60.0
    uv = observe(Kn, T8, pts, rng, 0.8)
    score = rng.uniform(0.62, 1.0, size=(8, K_POINTS))
    score[2] = rng.uniform(0.9, 1.0, size=K_POINTS)
    assert 10 <= (uv[2, :, 0] < 0).sum() <= K_POINTS - 10
    add("n8_negative_u", Kn, T8, uv, score)

    K30, T30 = camera_matrices(ring(30))
    rng = np.random.default_rng(6)  # more than max_views = 24 views: the percentile threshold lies above 0.6
    add("n30_percentile", K30, T30, observe(K30, T30, pts, rng, 1.0, n_outliers=20), rng.uniform(0.62, 1.0, size=(30, K_POINTS)))

    rng = np.random.default_rng(7)  # tied scores at the threshold: more than 24 views are selected
    score = np.full((30, K_POINTS), 0.9)
    for i in range(K_POINTS):
        low = rng.permutation(30)[: int(rng.integers(8, 27))]
        score[low, i] = 0.7
    add("n30_ties", K30, T30, observe(K30, T30, pts, rng, 1.0), score)

    K70, T70 = camera_matrices(ring(70))
    rng = np.random.default_rng(8)  # more views than a wave has lanes, k = 4
    score = rng.uniform(0.5, 1.0, size=(70, 4))
    score[:, 1] = 0.8                                  # every view tied: 70 selected
    score[64:, 2] = rng.uniform(0.95, 1.0, size=6)    # the views past lane 63 are all selected
    score[:, 3] = rng.uniform(0.1, 0.55, size=70)
    score[[5, 66], 3] = 0.9                            # 2 views: INVALID
    add("n70_k4", K70, T70, observe(K70, T70, body(4, 12), rng, 1.0), score)

    for t in range(3):  # the frames of the F = 3 batch, each recorded singly
        rng = np.random.default_rng(20 + t)
        score = rng.uniform(0.5, 1.0, size=(8, K_POINTS))
        add(f"batch3_f{t}", K8, T8, observe(K8, T8, body(K_POINTS, 11, t), rng, 1.0, n_outliers=15), score)
    return cases


# -- the reference ----------------------------------------------------------------------------------------------------------------
def install_standins() -> None:
    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__path__ = []
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m

    module("fire", Fire=lambda fn: None)
    module("easyvolcap")
    module("easyvolcap.utils")
    module("easyvolcap.utils.console_utils", tqdm=lambda it, **kw: it)
    module("easyvolcap.utils.parallel_utils", parallel_execution=lambda items, action, **kw: [action(i) for i in items])


def load_reference():
    from oracle import refshim
    install_standins()
    spec = importlib.util.spec_from_file_location("ref_triangulate_skeleton",
                                                  Path(refshim.REFERENCE_ROOT) / "scripts" / "preprocess" / "triangulate_skeleton.py")
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)  # appends the reference root to sys.path itself and imports triang_utils from there
    return ref, sys.modules["scripts.preprocess.utils.triang_utils"]


def converged(tu, Ks, Ts, kp2d, score, kp3d_ref, n_views_ref, min_views=3, score_thr=0.6):
    """Per valid keypoint: the Huber problem of triangulate_one_point on the views it selects, solved by scipy at 1e-15 from the
    reference's result (a) and from the linear start (b) -> kp3d_a, reproj_a, kp3d_b, reproj_b (INVALID rows where the reference's)."""
    from scipy.optimize import least_squares
    import triang_model
    n, k, _ = kp2d.shape
    out = [np.full((k, 3), tu.INVALID), np.full(k, tu.INVALID), np.full((k, 3), tu.INVALID), np.full(k, tu.INVALID)]
    max_views = min(24, n)
    for i in range(k):
        s = score[:, i]
        thr = max(score_thr, np.percentile(s, 100 * (1 - max_views / n)))
        sel = s >= thr
        assert sel.sum() == n_views_ref[i]
        if sel.sum() < min_views:
            continue
        K, T, uv, s = Ks[sel], Ts[sel], kp2d[sel, i], s[sel]
        P = K @ T[:, :3]
        w = np.repeat(np.sqrt(s), 2)

        def residual(X):
            pred, _ = tu.project_one_point(X, K, T)
            return (pred.reshape(-1) - uv.reshape(-1)) * w

        def jac(X):
            h = P[:, :, :3] @ X + P[:, :, 3]
            den = h[:, 2] + 1e-9
            J = np.empty((len(K), 2, 3))
            J[:, 0] = (P[:, 0, :3] - (h[:, 0] / den)[:, None] * P[:, 2, :3]) / den[:, None]
            J[:, 1] = (P[:, 1, :3] - (h[:, 1] / den)[:, None] * P[:, 2, :3]) / den[:, None]
            return J.reshape(-1, 3) * w[:, None]

        def reproj(X):
            pred, _ = tu.project_one_point(X, K, T)
            return (np.linalg.norm(pred - uv, axis=1) * s).sum() / (s.sum() + 1e-9)

        for slot, start in ((0, kp3d_ref[i]), (2, triang_model.linear_start(P, uv, s))):
            x = least_squares(residual, start, jac=jac, method="trf", loss="huber", f_scale=1.0, ftol=1e-15, xtol=1e-15, gtol=1e-15,
                              max_nfev=5000).x
            x_scipy = x
            for _ in range(30):  # polish: Newton steps on the gradient of the same cost (see the module docstring)
                r, J = residual(x), jac(x)
                quad = np.abs(r) <= 1.0
                step = -np.linalg.solve(J[quad].T @ J[quad], J.T @ np.where(quad, r, np.sign(r)))
                x = x + step
                if np.abs(step).max() <= 1e-16:
                    break
            assert np.abs(x - x_scipy).max() <= 1e-8, (i, x, x_scipy)  # the polish stays where scipy ended
            out[slot][i], out[slot + 1][i] = x, reproj(x)
    return out


def distances(kp3d, reproj, conv):
    """-> d_ref and d_conv for the point (m) and for reproj (px), maxima over the valid keypoints, and the asserted properties."""
    ca, ra, cb, rb = conv
    valid = ~(kp3d == -1e6).any(axis=-1)
    assert valid.any()
    d = {"d_ref_m": float(np.linalg.norm(kp3d[valid] - ca[valid], axis=-1).max()),
         "d_conv_m": float(np.linalg.norm(ca[valid] - cb[valid], axis=-1).max()),
         "d_ref_px": float(np.abs(reproj[valid] - ra[valid]).max()), "d_conv_px": float(np.abs(ra[valid] - rb[valid]).max())}
    assert d["d_conv_m"] <= 1e-3 * d["d_ref_m"] or d["d_conv_m"] < 1e-12, d
    assert d["d_ref_m"] <= 1e-6, d
    return d


def record() -> None:
    ref, tu = load_reference()

    # file route: triangulate_skeleton on both scenes; Ks, Ts and the 2-D input as the reference hands them to triangulate_points
    scenes = {}
    for name, (n, frames) in SCENES.items():
        seen = []
        inner = ref.triangulate_points

        def recording(Ks, Ts, kp2d, kp2d_score=None, **kw):
            seen.append((Ks.copy(), Ts.copy(), kp2d.copy(), kp2d_score.copy()))
            return inner(Ks, Ts, kp2d, kp2d_score, **kw)
        ref.triangulate_points = recording
        with tempfile.TemporaryDirectory() as tmp:
            t0 = time.perf_counter()
            ref.triangulate_skeleton(camera_path=str(SCENE_DIR / name / "transforms.json"), kp2d_dir=str(SCENE_DIR / name / "poses_sapiens"),
                                     out_kp3d_dir=f"{tmp}/poses_3d", out_kp2d_proj_dir=f"{tmp}/poses_2d")
            seconds = (time.perf_counter() - t0) / frames
            files = {}  # relative path -> {key: array of the parsed values} of instance_info[0]
            for p in sorted(Path(tmp).rglob("*.json")):
                parsed = json.loads(p.read_text())
                assert list(parsed) == ["instance_info"] and len(parsed["instance_info"]) == 1
                files[str(p.relative_to(tmp))] = {k: np.array(v, dtype=np.float64) for k, v in parsed["instance_info"][0].items()}
        ref.triangulate_points = inner
        assert len(seen) == frames and len(files) == frames * (1 + n)
        Ks, Ts = seen[0][0], seen[0][1]
        assert Ks.dtype == np.float64 and Ts.dtype == np.float64 and Ks.shape == (n, 3, 3) and Ts.shape == (n, 4, 4)
        per_frame = []
        for t, (_, _, kp2d, score) in enumerate(seen):
            inst = files[f"poses_3d/{t:06d}.json"]
            kp3d, reproj = inst["keypoints"], inst["keypoint_reproj"]
            _, _, n_views = tu.triangulate_points(Ks, Ts, kp2d, score)
            conv = converged(tu, Ks, Ts, kp2d, score, kp3d, n_views)
            d = distances(kp3d, reproj, conv)
            per_frame.append({"label": f"{t:06d}", "kp3d_converged": conv[0], "reproj_converged": conv[1], "n_views": n_views.astype(np.int32), **d})
            print(f"{name} frame {t}: {int((n_views >= 3).sum())} valid, " + ", ".join(f"{k} {v:.2e}" for k, v in d.items()))
        scenes[name] = {"labels": [f"{c:02d}" for c in range(n)], "Ks": Ks, "Ts": Ts, "files": files, "frames": per_frame,
                        "ref_cpu_seconds_per_frame": seconds}
        print(f"{name}: {len(files)} files, reference {seconds:.3f} s per frame on the CPU")

    cases = []
    for c in build_cases():
        kp3d, reproj, n_views = tu.triangulate_points(c["Ks"], c["Ts"], c["kp2d"], c["score"])
        conv = converged(tu, c["Ks"], c["Ts"], c["kp2d"], c["score"], kp3d, n_views)
        d = distances(kp3d, reproj, conv)
        cases.append({**c, "kp3d": kp3d, "reproj": reproj, "n_views": n_views.astype(np.int32), "kp3d_converged": conv[0],
                      "reproj_converged": conv[1], **d})
        print(f"{c['name']}: n_views {sorted(set(n_views.astype(int).tolist()))}, {int((n_views >= 3).sum())} valid, "
              + ", ".join(f"{k} {v:.2e}" for k, v in d.items()))
    by = {c["name"]: c for c in cases}
    assert set(by["n3_min_views"]["n_views"].tolist()) == {3}
    assert set(by["n8_views_2_3_8"]["n_views"].tolist()) == {2, 3, 8}
    assert by["n30_percentile"]["n_views"].max() <= 24 and by["n30_ties"]["n_views"].max() > 24
    assert by["n70_k4"]["n_views"].tolist()[1] == 70 and by["n70_k4"]["n_views"].tolist()[3] == 2
    assert by["n8_clean"]["reproj"].max() < 1e-6

    # projection: recorded points with INVALID rows, into the 8 cameras; once with scores (the face-normal update)
    src = by["n8_views_2_3_8"]
    rng = np.random.default_rng(9)
    kp3d_score = rng.uniform(0.3, 1.0, size=K_POINTS)
    uv, depth, _ = tu.project_points(src["kp3d"], src["Ks"], src["Ts"])
    _, _, score_out = tu.project_points(by["n8_outliers"]["kp3d"], src["Ks"], src["Ts"], kp3d_score=kp3d_score.copy())
    projections = [{"name": "invalid_rows", "kp3d": src["kp3d"], "Ks": src["Ks"], "Ts": src["Ts"], "kp2d": uv, "depth": depth},
                   {"name": "face_scores", "kp3d": by["n8_outliers"]["kp3d"], "Ks": src["Ks"], "Ts": src["Ts"], "kp3d_score": kp3d_score,
                    "kp2d_score": score_out}]
    assert (uv == -1e6).any() and (depth == -1e6).any()
    torch.save({"scenes": scenes, "cases": cases, "projections": projections}, OUT / "triang_reference.pt", pickle_protocol=4)
    print("wrote", OUT / "triang_reference.pt", (OUT / "triang_reference.pt").stat().st_size, "bytes")


if __name__ == "__main__":
    if "--scene" in sys.argv:
        write_scene()
    else:
        record()
