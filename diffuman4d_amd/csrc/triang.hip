// Skeleton triangulation (scripts/preprocess/utils/triang_utils.py): 3-D keypoints from per-view 2-D keypoints and scores, and their
// projection with depths into a set of cameras.  All arithmetic is fp64.
//
// dm4d_triangulate_points_f64: one wave per (frame, keypoint) problem, lanes over views (view j = lane, lane + 64, ...: any n).  Every
// sum over views is a per-lane sum in ascending j followed by a 6-stage xor butterfly, whose two partners add the same two numbers, so
// all 64 lanes hold the same bits and every branch below is wave-uniform.  A problem reads only its own column of the inputs: the
// result does not depend on the batch it is launched in, and repeats bit for bit.  No atomics, no shared memory, no barrier; no block
// waits on another.
//
//   selection   view j is selected iff score >= thr; n_views = their number; fewer than min_views -> kp3d = reproj = -1e6
//   start       M = sum s (a a^T + b b^T), a = u P[2] - P[0], b = v P[2] - P[1] (selected views with s > 0, u >= 0, v >= 0);
//               eigenvector of M's smallest eigenvalue by cyclic Jacobi sweeps; X = x[:3] / (x[3] + 1e-9)
//   iteration   damped Gauss-Newton on scipy's Huber cost 0.5 sum rho(r^2), r = (proj - obs) sqrt(s) per scalar component,
//               rho(z) = z (z <= 1), 2 sqrt(z) - 1 (z > 1).  g = J^T psi(r) with psi = r or sign(r); H = J^T J over the rows on the
//               quadratic branch (the linear branch has no curvature in r); the damping is lambda diag(D), D = sum rho'(r^2) J^T J
//               over all rows, which stays positive when few rows are quadratic.  Solve (H + lambda diag D) step = -g.  The step is
//               taken when the cost does not rise by more than the rounding of its own sum (kCostSlack*), then lambda /= 10;
//               otherwise lambda *= 10.  Stop when a taken step has max |step| <= 1e-15 (max |X| + 1e-3), when lambda > 1e15, or after
//               kMaxEvals evaluations; the last iterate is written in every case.
//   residuals   proj - obs = (h0 - u (h2 + 1e-9)) / (h2 + 1e-9): the numerator cancels from ~1e3 to the size of the residual, so it
//               is summed in double-double (two_sum / two_prod with fma).  Plain fp64 leaves ~1e-13 px of noise per residual,
//               about 4e-16 m on the point: more than the distance of the reference from its own minimiser on noise-free input.
//   reproj      sum(err_px s) / (sum s + 1e-9) over the selected views, err_px the unweighted pixel norm
//
// P = K @ T[:3] is formed per view as fma(K2, T2, fma(K1, T1, K0 T0)): the order in which a BLAS kernel accumulates the reference's
// matmul, so P is the reference's to the bit where its BLAS does so.  Compiled with -ffp-contract=off (build.py EXTRA_FLAGS): every
// fused multiply-add below is written as fma(), and the error-free transformations rely on nothing else being fused.
#include <stdint.h>

#include "common.h"
#include "dm4d.h"
#include "errors.h"
#include "project_common.h"

namespace {

constexpr int kThreads = 256;  // 4 waves = 4 problems per block
constexpr int kWaves = kThreads / 64;
constexpr int kMaxEvals = 64;
constexpr int kJacobiSweeps = 16;
constexpr double kInvalid = -1e6;
constexpr double kLambda0 = 1e-3, kLambdaMin = 1e-15, kLambdaMax = 1e15;
constexpr double kStepTol = 1e-15;
constexpr double kCostSlackRel = 1e-12, kCostSlackAbs = 1e-24;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

__device__ __forceinline__ void two_sum(double a, double b, double& s, double& e) {
  s = a + b;
  const double bb = s - a;
  e = (a - (s - bb)) + (b - bb);
}

__device__ __forceinline__ void two_prod(double a, double b, double& p, double& e) {
  p = a * b;
  e = fma(a, b, -p);
}

struct View {
  double P[12];  // row-major 3 x 4
  double u, v, s;
};

// projection(), project_row() and project_point(): project_common.h, shared with the skeleton plan kernel

// pr . (X, 1) - obs (p2 . (X, 1) + 1e-9) in double-double, rounded once at the end
__device__ __forceinline__ double residual_numerator(const double* pr, const double* p2, double obs, const double* X) {
  double acc_hi = 0.0, acc_lo = 0.0;
#pragma unroll
  for (int c = 0; c < 5; ++c) {
    double a_hi, a_lo;
    if (c < 4) {  // a = pr[c] - obs p2[c]
      double ph, pl, sl;
      two_prod(obs, p2[c], ph, pl);
      two_sum(pr[c], -ph, a_hi, sl);
      a_lo = sl - pl;
    } else {  // the 1e-9 of the denominator
      two_prod(-obs, 1e-9, a_hi, a_lo);
    }
    const double x = c < 3 ? X[c] : 1.0;
    double th, tl, s, e;
    two_prod(a_hi, x, th, tl);
    tl = fma(a_lo, x, tl);
    two_sum(acc_hi, th, s, e);
    acc_hi = s;
    acc_lo += e + tl;
  }
  return acc_hi + acc_lo;
}

struct Problem {
  const double* K;
  const double* T;
  const double* kp2d;   // this problem's first view: element j at [j * stride * 2]
  const double* score;  // element j at [j * stride]
  int64_t stride;       // k
  double thr;
  int n, lane;
};

__device__ __forceinline__ bool load_view(const Problem& q, int j, View& w) {
  if (j >= q.n) return false;
  const double s = q.score[(int64_t)j * q.stride];
  if (!(s >= q.thr)) return false;
  projection(q.K + (int64_t)j * 9, q.T + (int64_t)j * 16, w.P);
  w.u = q.kp2d[(int64_t)j * q.stride * 2];
  w.v = q.kp2d[(int64_t)j * q.stride * 2 + 1];
  w.s = s;
  return true;
}

struct Eval {
  double cost, g[3], H[6], D[3];  // H: 00 01 02 11 12 22
};

__device__ void evaluate(const Problem& q, const double* X, Eval& out) {
  double acc[13];
#pragma unroll
  for (int i = 0; i < 13; ++i) acc[i] = 0.0;
  for (int base = 0; base < q.n; base += 64) {
    View w;
    if (load_view(q, base + q.lane, w)) {
      const double den = project_row(w.P + 8, X) + 1e-9;
      const double sw = sqrt(w.s);
      const double scale = sw / den;
#pragma unroll
      for (int row = 0; row < 2; ++row) {
        const double obs = row == 0 ? w.u : w.v;
        const double d = residual_numerator(w.P + row * 4, w.P + 8, obs, X) / den;  // proj - obs
        const double p = obs + d;
        const double r = d * sw;
        const double a = fabs(r);
        const bool quad = a <= 1.0;
        double J[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) J[c] = (w.P[row * 4 + c] - p * w.P[8 + c]) * scale;
        acc[0] += quad ? 0.5 * (r * r) : a - 0.5;
        const double psi = quad ? r : (r > 0.0 ? 1.0 : -1.0);
        const double wq = quad ? 1.0 : 0.0;
        const double wi = quad ? 1.0 : 1.0 / a;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          acc[1 + c] += J[c] * psi;
          acc[10 + c] += wi * (J[c] * J[c]);
        }
        acc[4] += wq * (J[0] * J[0]);
        acc[5] += wq * (J[0] * J[1]);
        acc[6] += wq * (J[0] * J[2]);
        acc[7] += wq * (J[1] * J[1]);
        acc[8] += wq * (J[1] * J[2]);
        acc[9] += wq * (J[2] * J[2]);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 13; ++i) acc[i] = wave_sum(acc[i]);
  out.cost = acc[0];
#pragma unroll
  for (int c = 0; c < 3; ++c) out.g[c] = acc[1 + c], out.D[c] = acc[10 + c];
#pragma unroll
  for (int c = 0; c < 6; ++c) out.H[c] = acc[4 + c];
}

// (H + lambda diag D) step = -g by cofactors; false when the matrix is not positive or something is not finite
__device__ bool solve_step(const Eval& e, double lambda, double* step) {
  const double a00 = e.H[0] + lambda * e.D[0], a01 = e.H[1], a02 = e.H[2];
  const double a11 = e.H[3] + lambda * e.D[1], a12 = e.H[4], a22 = e.H[5] + lambda * e.D[2];
  const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
  const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
  const double det = a00 * c00 + a01 * c01 + a02 * c02;
  if (!(det > 0.0) || !isfinite(det)) return false;
  step[0] = -(c00 * e.g[0] + c01 * e.g[1] + c02 * e.g[2]) / det;
  step[1] = -(c01 * e.g[0] + c11 * e.g[1] + c12 * e.g[2]) / det;
  step[2] = -(c02 * e.g[0] + c12 * e.g[1] + c22 * e.g[2]) / det;
  return isfinite(step[0]) && isfinite(step[1]) && isfinite(step[2]);
}

// eigenvector of the smallest eigenvalue of the symmetric 4 x 4 A (destroyed), cyclic Jacobi
__device__ void jacobi_smallest(double A[4][4], double* x) {
  double V[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
    const double off = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[0][3]) + fabs(A[1][2]) + fabs(A[1][3]) + fabs(A[2][3]);
    if (off == 0.0) break;
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int q = p + 1; q < 4; ++q) {
        const double apq = A[p][q];
        if (apq != 0.0) {
          const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
          const double t = fabs(theta) > 1e100 ? 0.5 / theta : copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
          const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
          for (int k = 0; k < 4; ++k) {  // A J
            const double akp = A[k][p], akq = A[k][q];
            A[k][p] = c * akp - s * akq;
            A[k][q] = s * akp + c * akq;
          }
#pragma unroll
          for (int k = 0; k < 4; ++k) {  // J^T (A J)
            const double apk = A[p][k], aqk = A[q][k];
            A[p][k] = c * apk - s * aqk;
            A[q][k] = s * apk + c * aqk;
          }
          A[p][q] = A[q][p] = 0.0;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const double vkp = V[k][p], vkq = V[k][q];
            V[k][p] = c * vkp - s * vkq;
            V[k][q] = s * vkp + c * vkq;
          }
        }
      }
  }
  double best = A[0][0];
#pragma unroll
  for (int k = 0; k < 4; ++k) x[k] = V[k][0];
#pragma unroll
  for (int j = 1; j < 4; ++j)
    if (A[j][j] < best) {
      best = A[j][j];
#pragma unroll
      for (int k = 0; k < 4; ++k) x[k] = V[k][j];
    }
}

__device__ void linear_start(const Problem& q, double* X) {
  double m[10];  // upper triangle of M: 00 01 02 03 11 12 13 22 23 33
#pragma unroll
  for (int i = 0; i < 10; ++i) m[i] = 0.0;
  for (int base = 0; base < q.n; base += 64) {
    View w;
    if (load_view(q, base + q.lane, w) && w.s > 0.0 && w.u >= 0.0 && w.v >= 0.0) {
#pragma unroll
      for (int row = 0; row < 2; ++row) {
        const double obs = row == 0 ? w.u : w.v;
        double a[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) a[c] = obs * w.P[8 + c] - w.P[row * 4 + c];
        int i = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int c = r; c < 4; ++c) m[i++] += w.s * (a[r] * a[c]);
      }
    }
  }
  double A[4][4];
  int i = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = r; c < 4; ++c) {
      const double v = wave_sum(m[i++]);
      A[r][c] = v;
      A[c][r] = v;
    }
  double x[4];
  jacobi_smallest(A, x);
  const double d = x[3] + 1e-9;
  X[0] = x[0] / d, X[1] = x[1] / d, X[2] = x[2] / d;
}

__global__ void __launch_bounds__(kThreads) triangulate_kernel(const double* __restrict__ K, const double* __restrict__ T,
                                                               const double* __restrict__ kp2d, const double* __restrict__ score,
                                                               const double* __restrict__ thr, int64_t problems, int n, int k, int min_views,
                                                               double* __restrict__ kp3d, double* __restrict__ reproj, int32_t* __restrict__ n_views) {
  const int64_t prob = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (prob >= problems) return;  // the whole wave
  const int64_t f = prob / k, i = prob - f * k;
  Problem q;
  q.K = K, q.T = T;
  q.kp2d = kp2d + (f * n * k + i) * 2;
  q.score = score + f * n * k + i;
  q.stride = k;
  q.thr = thr[prob];
  q.n = n, q.lane = threadIdx.x & 63;

  int count = 0;
  for (int base = 0; base < n; base += 64) {
    const int j = base + q.lane;
    count += __popcll(__ballot(j < n && q.score[(int64_t)j * k] >= q.thr));
  }
  double X[3] = {kInvalid, kInvalid, kInvalid}, rp = kInvalid;
  if (count >= min_views) {
    linear_start(q, X);
    Eval cur, next;
    evaluate(q, X, cur);
    double lambda = kLambda0;
    for (int it = 0; it < kMaxEvals; ++it) {
      double step[3], Xn[3];
      bool ok = solve_step(cur, lambda, step);
      if (ok) {
#pragma unroll
        for (int c = 0; c < 3; ++c) Xn[c] = X[c] + step[c];
        evaluate(q, Xn, next);
        ok = isfinite(next.cost) && next.cost <= cur.cost * (1.0 + kCostSlackRel) + kCostSlackAbs;
      }
      if (ok) {
        const double big = fmax(fabs(step[0]), fmax(fabs(step[1]), fabs(step[2])));
        const double size = fmax(fabs(X[0]), fmax(fabs(X[1]), fabs(X[2])));
#pragma unroll
        for (int c = 0; c < 3; ++c) X[c] = Xn[c];
        cur = next;
        lambda = fmax(lambda * 0.1, kLambdaMin);
        if (big <= kStepTol * (size + 1e-3)) break;
      } else {
        lambda *= 10.0;
        if (lambda > kLambdaMax) break;
      }
    }
    double num = 0.0, den = 0.0;
    for (int base = 0; base < n; base += 64) {
      View w;
      if (load_view(q, base + q.lane, w)) {
        const double z = project_row(w.P + 8, X) + 1e-9;
        const double du = project_row(w.P, X) / z - w.u, dv = project_row(w.P + 4, X) / z - w.v;
        num += sqrt(du * du + dv * dv) * w.s;
        den += w.s;
      }
    }
    rp = wave_sum(num) / (wave_sum(den) + 1e-9);
  }
  if (q.lane == 0) {
    kp3d[prob * 3] = X[0], kp3d[prob * 3 + 1] = X[1], kp3d[prob * 3 + 2] = X[2];
    reproj[prob] = rp;
    n_views[prob] = count;
  }
}

// one lane per (frame, camera, keypoint)
__global__ void __launch_bounds__(kThreads) project_kernel(const double* __restrict__ kp3d, const double* __restrict__ K, const double* __restrict__ T,
                                                           int64_t total, int m, int k, double* __restrict__ kp2d, double* __restrict__ depth) {
  const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= total) return;
  const int64_t fm = idx / k, i = idx - fm * k;
  const int64_t f = fm / m, cam = fm - f * m;
  const double* Xp = kp3d + (f * k + i) * 3;
  const double X[3] = {Xp[0], Xp[1], Xp[2]};
  double u, v, z;
  project_point(K + cam * 9, T + cam * 16, X, u, v, z);
  kp2d[idx * 2] = u, kp2d[idx * 2 + 1] = v;
  depth[idx] = z;
}

bool misaligned8(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr, const void* e = nullptr) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d | (uintptr_t)e) & 7) != 0;
}

}  // namespace

extern "C" int dm4d_triangulate_points_f64(void* stream, const double* K, const double* T, const double* kp2d, const double* score,
                                           const double* thr, int F, int n, int k, int min_views, double* kp3d, double* reproj,
                                           int32_t* n_views) {
  if (!K || !T || !kp2d || !score || !thr || !kp3d || !reproj || !n_views)
    return dm4d_set_error(DM4D_ERR_ARG, "triangulate_points: null pointer");
  if (F <= 0 || n <= 0 || k <= 0 || n > DM4D_TRIANG_MAX_VIEWS) return dm4d_set_error(DM4D_ERR_ARG, "triangulate_points: empty shape or too many views");
  if (min_views < 1) return dm4d_set_error(DM4D_ERR_ARG, "triangulate_points: min_views must be positive");
  if (misaligned8(K, T, kp2d, score, thr) || misaligned8(kp3d, reproj) || ((uintptr_t)n_views & 3))
    return dm4d_set_error(DM4D_ERR_ARG, "triangulate_points: misaligned pointer");
  const int64_t problems = (int64_t)F * k;
  const int64_t grid = (problems + kWaves - 1) / kWaves;
  if (grid > 0x7fffffffll) return dm4d_set_error(DM4D_ERR_ARG, "triangulate_points: too many problems for one launch");
  hipLaunchKernelGGL(triangulate_kernel, dim3((unsigned)grid), dim3(kThreads), 0, (hipStream_t)stream, K, T, kp2d, score, thr, problems, n, k,
                     min_views, kp3d, reproj, n_views);
  return dm4d_check_launch("triangulate_kernel");
}

extern "C" int dm4d_project_points_f64(void* stream, const double* kp3d, const double* K, const double* T, int F, int m, int k, double* kp2d,
                                       double* depth) {
  if (!kp3d || !K || !T || !kp2d || !depth) return dm4d_set_error(DM4D_ERR_ARG, "project_points: null pointer");
  if (F <= 0 || m <= 0 || k <= 0) return dm4d_set_error(DM4D_ERR_ARG, "project_points: empty shape");
  if (misaligned8(kp3d, K, T, kp2d, depth)) return dm4d_set_error(DM4D_ERR_ARG, "project_points: misaligned pointer");
  const int64_t total = (int64_t)F * m * k;
  const int64_t grid = (total + kThreads - 1) / kThreads;
  if (grid > 0x7fffffffll) return dm4d_set_error(DM4D_ERR_ARG, "project_points: too many points for one launch");
  hipLaunchKernelGGL(project_kernel, dim3((unsigned)grid), dim3(kThreads), 0, (hipStream_t)stream, kp3d, K, T, total, m, k, kp2d, depth);
  return dm4d_check_launch("project_kernel");
}
