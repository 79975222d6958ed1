"""The algorithm of csrc/triang.hip (dm4d_triangulate_points_f64, dm4d_project_points_f64) restated in plain numpy fp64.

Same selection, linear start, damped Gauss-Newton iteration on scipy's Huber cost (with the residuals' numerators in double-double),
stopping rule, `reproj` and projection as the kernels; the order of the sums over views differs (numpy's, not the wave's) and the 3 x 3
system is solved by LAPACK instead of cofactors, so the model agrees with the device to rounding
and is held to the same bound against the converged minimiser (tests/test_triang_cpu.py).  Used by tests/test_triang_cpu.py and by
tests/golden/make_golden_triang.py (the linear start of its converged solves).
"""
from __future__ import annotations

import numpy as np

INVALID = -1e6
MAX_EVALS = 64        # csrc/triang.hip kMaxEvals
LAMBDA0, LAMBDA_MIN, LAMBDA_MAX = 1e-3, 1e-15, 1e15
STEP_TOL = 1e-15      # stop once max|step| <= STEP_TOL * (max|X| + 1e-3)
COST_SLACK_REL, COST_SLACK_ABS = 1e-12, 1e-24   # a step may raise the cost by the rounding noise of the residuals only


_SPLIT = 134217729.0  # 2^27 + 1: Dekker's split of a double into two 26-bit halves


def two_sum(a, b):
    """-> (s, e) with s = fl(a + b) and s + e = a + b exactly."""
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def two_prod(a, b):
    """-> (p, e) with p = fl(a b) and p + e = a b exactly (the kernel takes e from one fma)."""
    p = a * b
    t = _SPLIT * a
    ah = t - (t - a)
    al = a - ah
    t = _SPLIT * b
    bh = t - (t - b)
    bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma(a, b, c):
    """fl(a b + c) from the exact product (a double rounding can differ from a hardware fma in the last bit, rarely)."""
    p, e = two_prod(a, b)
    s, t = two_sum(p, c)
    return s + (t + e)


def projections(Ks, Ts):
    """K [n, 3, 3], T [n, 4, 4] -> P = K @ T[:3], [n, 3, 4], each entry fma(K2, T2, fma(K1, T1, K0 T0)) as the kernel forms it."""
    Ks, Ts = np.asarray(Ks, np.float64), np.asarray(Ts, np.float64)
    k = [np.broadcast_to(Ks[:, :, c, None], (len(Ks), 3, 4)) for c in range(3)]
    t = [np.broadcast_to(Ts[:, None, c, :], (len(Ks), 3, 4)) for c in range(3)]
    return fma(k[2], t[2], fma(k[1], t[1], k[0] * t[0]))


def project_rows(P, X):
    """h [n, 3] = P (X, 1), each row accumulated in index order with fused multiply-adds."""
    return fma(P[:, :, 2], X[2], fma(P[:, :, 1], X[1], P[:, :, 0] * X[0])) + P[:, :, 3]


def residual_numerator(pr, p2, obs, X):
    """pr . (X, 1) - obs (p2 . (X, 1) + 1e-9) per view in double-double, rounded once at the end (csrc/triang.hip): pr, p2 [n, 4]."""
    acc_hi, acc_lo = np.zeros(len(obs)), np.zeros(len(obs))
    for c in range(5):
        if c < 4:
            ph, pl = two_prod(obs, p2[:, c])
            a_hi, sl = two_sum(pr[:, c], -ph)
            a_lo = sl - pl
        else:
            a_hi, a_lo = two_prod(-obs, np.full(len(obs), 1e-9))
        x = X[c] if c < 3 else 1.0
        th, tl = two_prod(a_hi, np.full(len(obs), x))
        tl = tl + a_lo * x
        acc_hi, e = two_sum(acc_hi, th)
        acc_lo = acc_lo + (e + tl)
    return acc_hi + acc_lo


def jacobi_smallest(M):
    """Eigenvector of the smallest eigenvalue of the symmetric 4 x 4 M by cyclic Jacobi sweeps (as the kernel: at most 16 sweeps,
    ended early once every off-diagonal entry is zero)."""
    A = np.array(M, dtype=np.float64)
    V = np.eye(4)
    for _ in range(16):
        off = sum(abs(A[p, q]) for p in range(4) for q in range(p + 1, 4))
        if off == 0.0:
            break
        for p in range(3):
            for q in range(p + 1, 4):
                if A[p, q] == 0.0:
                    continue
                with np.errstate(over="ignore"):
                    theta = (A[q, q] - A[p, p]) / (2.0 * A[p, q])
                if abs(theta) > 1e100:  # theta * theta would overflow
                    t = 0.5 / theta
                else:
                    t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                J = np.eye(4)
                J[p, p] = J[q, q] = c
                J[p, q], J[q, p] = s, -s
                A = J.T @ A @ J
                A[p, q] = A[q, p] = 0.0
                V = V @ J
    return V[:, int(np.argmin(np.diag(A)))]


def linear_start(P, uv, s):
    """The reference's DLT start on the selected views (triang_utils.py:81-95) through the 4 x 4 normal matrix."""
    use = (s > 0) & (uv[:, 0] >= 0) & (uv[:, 1] >= 0)
    a = uv[:, 0, None] * P[:, 2] - P[:, 0]
    b = uv[:, 1, None] * P[:, 2] - P[:, 1]
    w = np.where(use, s, 0.0)
    M = np.einsum("j,ja,jb->ab", w, a, a) + np.einsum("j,ja,jb->ab", w, b, b)
    x = jacobi_smallest(M)
    return x[:3] / (x[3] + 1e-9)


def _evaluate(P, uv, s, X):
    """-> (cost, gradient [3], Gauss-Newton matrix of the quadratic-branch rows [3, 3], diagonal of the IRLS matrix [3])."""
    den = project_rows(P, X)[:, 2] + 1e-9
    w = np.sqrt(s)
    cost, g, H, d = 0.0, np.zeros(3), np.zeros((3, 3)), np.zeros(3)
    for row in (0, 1):
        obs = uv[:, row]
        diff = residual_numerator(P[:, row], P[:, 2], obs, X) / den  # proj - obs
        p = obs + diff
        r = diff * w
        J = (P[:, row, :3] - p[:, None] * P[:, 2, :3]) * (w / den)[:, None]
        a = np.abs(r)
        quad = a <= 1.0
        cost += np.where(quad, 0.5 * (r * r), a - 0.5).sum()
        psi = np.where(quad, r, np.sign(r))            # rho'(r^2) r
        irls = np.where(quad, 1.0, 1.0 / np.where(quad, 1.0, a))
        g += (J * psi[:, None]).sum(axis=0)
        H += np.einsum("j,ja,jb->ab", quad.astype(np.float64), J, J)
        d += (irls[:, None] * J * J).sum(axis=0)
    return cost, g, H, d


def refine(P, uv, s, X):
    """Damped Gauss-Newton on 0.5 sum rho(r^2), rho = scipy's huber with f_scale = 1, r per scalar component."""
    cost, g, H, d = _evaluate(P, uv, s, X)
    lam = LAMBDA0
    for _ in range(MAX_EVALS):
        A = H + lam * np.diag(d)
        det = np.linalg.det(A)
        ok = np.isfinite(det) and det > 0.0
        if ok:
            step = -np.linalg.solve(A, g)
            ok = bool(np.isfinite(step).all())
        if ok:
            Xn = X + step
            cn, gn, Hn, dn = _evaluate(P, uv, s, Xn)
            ok = np.isfinite(cn) and cn <= cost * (1.0 + COST_SLACK_REL) + COST_SLACK_ABS
        if ok:
            small = np.abs(step).max() <= STEP_TOL * (np.abs(X).max() + 1e-3)
            X, cost, g, H, d = Xn, cn, gn, Hn, dn
            lam = max(lam * 0.1, LAMBDA_MIN)
            if small:
                break
        else:
            lam *= 10.0
            if lam > LAMBDA_MAX:
                break
    return X


def reprojection_error(P, uv, s, X):
    h = project_rows(P, X)
    den = h[:, 2] + 1e-9
    du, dv = h[:, 0] / den - uv[:, 0], h[:, 1] / den - uv[:, 1]
    return (np.sqrt(du * du + dv * dv) * s).sum() / (s.sum() + 1e-9)


def triangulate(Ks, Ts, kp2d, score, thr, min_views=3):
    """Ks [n, 3, 3], Ts [n, 4, 4], kp2d [F, n, k, 2], score [F, n, k], thr [F, k] -> kp3d [F, k, 3], reproj [F, k], n_views int32
    [F, k]: what dm4d_triangulate_points_f64 writes."""
    P = projections(Ks, Ts)
    F, n, k, _ = kp2d.shape
    kp3d = np.full((F, k, 3), INVALID)
    reproj = np.full((F, k), INVALID)
    n_views = np.zeros((F, k), np.int32)
    for f in range(F):
        for i in range(k):
            sel = score[f, :, i] >= thr[f, i]
            n_views[f, i] = sel.sum()
            if n_views[f, i] < min_views:
                continue
            Ps, uv, s = P[sel], kp2d[f, sel, i], score[f, sel, i]
            X = refine(Ps, uv, s, linear_start(Ps, uv, s))
            kp3d[f, i], reproj[f, i] = X, reprojection_error(Ps, uv, s, X)
    return kp3d, reproj, n_views


def project(kp3d, Ks, Ts):
    """kp3d [F, k, 3], Ks [m, 3, 3], Ts [m, 4, 4] -> kp2d [F, m, k, 2], depth [F, m, k]: what dm4d_project_points_f64 writes."""
    P = projections(Ks, Ts)
    kp3d = np.asarray(kp3d, np.float64)
    X = [kp3d[:, None, :, c] for c in range(3)]
    h = np.stack([fma(P[None, :, None, r, 2], X[2], fma(P[None, :, None, r, 1], X[1], P[None, :, None, r, 0] * X[0])) + P[None, :, None, r, 3]
                  for r in range(3)], axis=-1)
    depth = h[..., 2]
    uv = h[..., :2] / (depth[..., None] + 1e-9)
    bad = (kp3d == INVALID).any(axis=-1)[:, None, :]
    return np.where(bad[..., None], INVALID, uv), np.where(bad, INVALID, depth)
