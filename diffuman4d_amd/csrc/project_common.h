// The projection of a 3-D keypoint into a camera (triang_utils.py project_one_point), fp64: the one definition that
// dm4d_project_points_f64 (triang.hip) and dm4d_skeleton_plan_kp3d (skeleton.hip) both evaluate, so that a map planned from poses_3d
// sees the bits that triangulate_skeleton writes into poses_2d.  Every fused multiply-add is written as fma(); the sources that
// include this header are compiled with -ffp-contract=off (build.py EXTRA_FLAGS), so nothing else is fused.
#pragma once

constexpr double kProjectInvalid = -1e6;

// P = K @ T[:3], each entry as fma(K2, T2, fma(K1, T1, K0 T0)): the order in which a BLAS kernel accumulates the reference's matmul
__device__ __forceinline__ void projection(const double* __restrict__ K, const double* __restrict__ T, double* P) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) P[r * 4 + c] = fma(K[r * 3 + 2], T[8 + c], fma(K[r * 3 + 1], T[4 + c], K[r * 3] * T[c]));
}

// h_r = P[r] . (X, 1), accumulated in index order
__device__ __forceinline__ double project_row(const double* p, const double* X) {
  return fma(p[2], X[2], fma(p[1], X[1], p[0] * X[0])) + p[3];
}

// (u, v) = xy / (depth + 1e-9), z = the third homogeneous coordinate; a point with a coordinate equal to -1e6 gives -1e6 in all three
__device__ __forceinline__ void project_point(const double* __restrict__ K, const double* __restrict__ T, const double* X, double& u, double& v,
                                              double& z) {
  u = v = z = kProjectInvalid;
  if (X[0] != kProjectInvalid && X[1] != kProjectInvalid && X[2] != kProjectInvalid) {
    double P[12];
    projection(K, T, P);
    z = project_row(P + 8, X);
    u = project_row(P, X) / (z + 1e-9);
    v = project_row(P + 4, X) / (z + 1e-9);
  }
}
