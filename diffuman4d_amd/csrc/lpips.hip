// LPIPS-VGG (the reference's third metric: torchmetrics' LearnedPerceptualImagePatchSimilarity(net_type="vgg", normalize=True),
// data/utils/metric_utils.py:14-19,134-137): the kernels around the thirteen VGG-16 convolutions, which themselves run on the MFMA
// convolution of gemm.hip (dm4d_conv3x3_nhwc_bf16_flags, fp32 out) -- host/lpips.py strings them together.
//
// Arithmetic.  VGG's weights are fp32 and its activations are not normalised, so every product is the three-term bf16 product of the
// parity precision: activations leave these kernels as pattern-1 operands [hi | lo | hi] (hi = bf16(x), lo = bf16(x - hi)) against
// weights packed per tap as [w_hi | w_hi | w_lo] at load time:  hi w_hi + lo w_hi + hi w_lo, fp32 accumulation.
//
//   lpips_input_kernel     the cropped composites of one pair (fp32 planes in [0, 1]) -> LPIPS' input scaling -> the operand of the first
//                          convolution, a batch of two images (0 = ground truth, 1 = prediction); the 3 x 3 planes are padded to one
//                          64-column K slab;
//   lpips_relu_pool_kernel ReLU (+ the 2 x 2 stride-2 floor max-pool) of a convolution's fp32 output -> the operand of the next one
//                          (ReLU and max commute: the convolution kernels need no epilogue of their own);
//   lpips_dist_kernel      one tap: ReLU on read, channel normalisation of both images, the linear layer's weighted squared difference,
//                          summed over channels and pixels in fp64 in a fixed order -> one partial per 256 pixels;
//   lpips_reduce_kernel    the partials of a tap in order -> its spatial mean (the host adds the five means in tap order).
// No floating-point atomics and a launch geometry that depends on the image size alone: a pair's value is the same bits on every run,
// and swapping the two images swaps only the sign inside a square.  This translation unit is compiled with -ffp-contract=off (as
// metrics.hip), so every fp32 / fp64 operation below is rounded on its own.
// Every index that scales with the pixel count is 64 bits wide.  The largest pair the path takes is set by the convolution entry, which
// refuses tensors of 2^31 elements: 2 h w 192 operand values of the 64-channel stage, i.e. h w < 5 592 405 (an edge of about 2364;
// host/lpips.py raises above it).  At that size the operand is 4 GiB, so byte offsets do pass 2^31.
#include <math.h>
#include <stdint.h>

#include "common.h"
#include "dm4d.h"
#include "errors.h"

namespace {

constexpr int kThreads = 256;
constexpr int kInCols = DM4D_LPIPS_IN_COLS;  // columns of the first operand: [hi(3) | lo(3) | hi(3) | zeros]
constexpr int kDistPixels = DM4D_LPIPS_DIST_PIXELS;

// torchmetrics' _LPIPS ScalingLayer (functional/image/lpips.py): (x - shift) / scale per channel, x in [-1, 1]
__constant__ float kShift[3] = {-0.030f, -0.088f, -0.188f};
__constant__ float kScale[3] = {0.458f, 0.448f, 0.450f};
// torchmetrics' _normalize_tensor(in_feat, eps=1e-8): in_feat / sqrt(eps + sum_c in_feat^2) -- the epsilon is INSIDE the square root
constexpr double kNormEps = 1e-8;

// ---- (a) composites -> scaled first-layer operand ------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) lpips_input_kernel(const float* __restrict__ gt, const float* __restrict__ pred,
                                                               int64_t cs, int64_t rs, int h, int w, u16* __restrict__ Y) {
  const int64_t hw = (int64_t)h * w;
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= 2 * hw) return;
  const int img = i >= hw ? 1 : 0;
  const int64_t pix = i - img * hw;
  const int y = (int)(pix / w), x = (int)(pix - (int64_t)y * w);
  const float* src = (img ? pred : gt) + (int64_t)y * rs + x;
  float v[8], z[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = z[e] = 0.0f;
  u16 hi[3], lo[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float s = 2.0f * src[c * cs] - 1.0f;  // normalize=True: [0, 1] -> [-1, 1]
    split2((s - kShift[c]) / kScale[c], hi[c], lo[c]);
  }
  // [hi0 hi1 hi2 lo0 lo1 lo2 hi0 hi1 | hi2 0 ...]: the values are already bf16, so pack8's rounding is exact
  v[0] = bf2f(hi[0]), v[1] = bf2f(hi[1]), v[2] = bf2f(hi[2]), v[3] = bf2f(lo[0]), v[4] = bf2f(lo[1]), v[5] = bf2f(lo[2]);
  v[6] = bf2f(hi[0]), v[7] = bf2f(hi[1]);
  z[0] = bf2f(hi[2]);
  u16* o = Y + i * kInCols;
  stg16(o, pack8(v));
  stg16(o + 8, pack8(z));
  z[0] = 0.0f;
#pragma unroll
  for (int k = 16; k < kInCols; k += 8) stg16(o + k, pack8(z));
}

// ---- (b) ReLU (+ 2 x 2 max-pool) of fp32 NHWC -> pattern-1 operand [hi(C) | lo(C) | hi(C)], 8 channels per lane ------------------------
__global__ void __launch_bounds__(kThreads) lpips_relu_pool_kernel(const float* __restrict__ X, u16* __restrict__ Y, int B, int H, int W,
                                                                   int C, int pool) {
  const int Ho = pool ? H / 2 : H, Wo = pool ? W / 2 : W, CV = C >> 3;
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (int64_t)B * Ho * Wo * CV) return;
  const int64_t m = i / CV;  // output pixel (b, yo, xo)
  const int c = (int)(i - m * CV) << 3;
  const int xo = (int)(m % Wo);
  const int64_t t = m / Wo;
  const int yo = (int)(t % Ho), b = (int)(t / Ho);
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = 0.0f;  // ReLU: the maximum starts at zero
  const int n = pool ? 2 : 1;
  for (int dy = 0; dy < n; ++dy)
    for (int dx = 0; dx < n; ++dx) {
      const float* src = X + (((int64_t)b * H + (yo * n + dy)) * W + (xo * n + dx)) * C + c;
      const f32x4_t a = *reinterpret_cast<const f32x4_t*>(src), d = *reinterpret_cast<const f32x4_t*>(src + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], a[e]), v[4 + e] = fmaxf(v[4 + e], d[e]);
    }
  float hi[8], lo[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    u16 h16, l16;
    split2(v[e], h16, l16);
    hi[e] = bf2f(h16), lo[e] = bf2f(l16);
  }
  u16* o = Y + m * (3 * (int64_t)C) + c;
  const U4 ph = pack8(hi);
  stg16(o, ph);
  stg16(o + C, pack8(lo));
  stg16(o + 2 * C, ph);
}

// ---- (c) tap distance ----------------------------------------------------------------------------------------------------------------
// F [2, HW, C] fp32 (before ReLU).  L = min(C / 4, 64) lanes share a pixel, each with NV float4 of either image; a workgroup owns
// kDistPixels consecutive pixels and leaves one partial sum.
template <int NV>
__global__ void __launch_bounds__(kThreads) lpips_dist_kernel(const float* __restrict__ F, const float* __restrict__ lin, int64_t HW, int C,
                                                              int L, double* __restrict__ partials) {
  __shared__ double red[kThreads];
  const int groups = kThreads / L, g = threadIdx.x / L, l = threadIdx.x % L;
  f32x4_t wl[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) wl[v] = *reinterpret_cast<const f32x4_t*>(lin + 4 * (l + L * v));
  double acc = 0.0;
  for (int j = g; j < kDistPixels; j += groups) {
    const int64_t p = (int64_t)blockIdx.x * kDistPixels + j;
    const bool on = p < HW;  // uniform over the L lanes of a pixel
    f32x4_t a[NV], b[NV];
    double sa = 0.0, sb = 0.0;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      if (on) {
        a[v] = *reinterpret_cast<const f32x4_t*>(F + p * C + 4 * (l + L * v));
        b[v] = *reinterpret_cast<const f32x4_t*>(F + (HW + p) * C + 4 * (l + L * v));
      } else {
        a[v] = b[v] = f32x4_t{0.0f, 0.0f, 0.0f, 0.0f};
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        a[v][e] = fmaxf(a[v][e], 0.0f), b[v][e] = fmaxf(b[v][e], 0.0f);
        sa += (double)a[v][e] * (double)a[v][e];
        sb += (double)b[v][e] * (double)b[v][e];
      }
    }
    for (int off = L >> 1; off > 0; off >>= 1) sa += __shfl_xor(sa, off, 64), sb += __shfl_xor(sb, off, 64);
    const double ia = 1.0 / sqrt(kNormEps + sa), ib = 1.0 / sqrt(kNormEps + sb);
    double d = 0.0;
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double diff = (double)a[v][e] * ia - (double)b[v][e] * ib;
        d += (double)wl[v][e] * (diff * diff);
      }
    for (int off = L >> 1; off > 0; off >>= 1) d += __shfl_xor(d, off, 64);
    if (on) acc += d;
  }
  red[threadIdx.x] = l == 0 ? acc : 0.0;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) partials[blockIdx.x] = red[0];
}

// out[tap] = mean over the pixels
__global__ void __launch_bounds__(kThreads) lpips_reduce_kernel(const double* __restrict__ partials, int64_t n, int64_t HW, int tap,
                                                                double* __restrict__ out) {
  __shared__ double red[kThreads];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += kThreads) s += partials[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int k = kThreads / 2; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[tap] = red[0] / (double)HW;
  }
}

}  // namespace

extern "C" int dm4d_lpips_input_split(void* stream, const float* gt, const float* pred, int64_t chan_stride, int64_t row_stride, int h,
                                      int w, void* Y) {
  if (!gt || !pred || !Y) return dm4d_set_error(DM4D_ERR_ARG, "lpips_input: null pointer");
  if (h <= 0 || w <= 0 || h > (1 << 15) || w > (1 << 15)) return dm4d_set_error(DM4D_ERR_ARG, "lpips_input: bad image size");
  if (row_stride < w || chan_stride < (int64_t)(h - 1) * row_stride + w)
    return dm4d_set_error(DM4D_ERR_ARG, "lpips_input: planes overlap (row_stride >= w and chan_stride >= (h - 1) row_stride + w)");
  if ((uintptr_t)Y & 15) return dm4d_set_error(DM4D_ERR_ARG, "lpips_input: Y must be 16-byte aligned");
  hipLaunchKernelGGL(lpips_input_kernel, grid1d((int64_t)2 * h * w, kThreads), dim3(kThreads), 0, (hipStream_t)stream, gt, pred, chan_stride,
                     row_stride, h, w, (u16*)Y);
  return dm4d_check_launch("lpips_input_kernel");
}

extern "C" int dm4d_lpips_relu_pool_split(void* stream, const float* X, void* Y, int B, int H, int W, int C, int pool) {
  if (!X || !Y) return dm4d_set_error(DM4D_ERR_ARG, "lpips_relu_pool: null pointer");
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 != 0) return dm4d_set_error(DM4D_ERR_ARG, "lpips_relu_pool: empty shape or C not a multiple of 8");
  if (pool && (H < 2 || W < 2)) return dm4d_set_error(DM4D_ERR_ARG, "lpips_relu_pool: nothing is left of an edge below 2 after the pooling");
  if (((uintptr_t)X | (uintptr_t)Y) & 15) return dm4d_set_error(DM4D_ERR_ARG, "lpips_relu_pool: X and Y must be 16-byte aligned");
  const int Ho = pool ? H / 2 : H, Wo = pool ? W / 2 : W;
  if ((int64_t)B * Ho * Wo * (C / 8) >= ((int64_t)1 << 31) * kThreads) return dm4d_set_error(DM4D_ERR_ARG, "lpips_relu_pool: tensor too large");
  hipLaunchKernelGGL(lpips_relu_pool_kernel, grid1d((int64_t)B * Ho * Wo * (C / 8), kThreads), dim3(kThreads), 0, (hipStream_t)stream, X,
                     (u16*)Y, B, H, W, C, pool ? 1 : 0);
  return dm4d_check_launch("lpips_relu_pool_kernel");
}

extern "C" size_t dm4d_lpips_ws_bytes(int H, int W) {
  if (H <= 0 || W <= 0) return 0;
  return (size_t)(((int64_t)H * W + kDistPixels - 1) / kDistPixels) * sizeof(double);
}

extern "C" int dm4d_lpips_tap_distance_f64(void* stream, const float* F, const float* lin, int H, int W, int C, int tap, void* workspace,
                                           int64_t workspace_bytes, double* out) {
  if (!F || !lin || !workspace || !out) return dm4d_set_error(DM4D_ERR_ARG, "lpips_tap_distance: null pointer");
  if (H <= 0 || W <= 0 || H > (1 << 15) || W > (1 << 15)) return dm4d_set_error(DM4D_ERR_ARG, "lpips_tap_distance: bad tap size");
  if (C != 64 && C != 128 && C != 256 && C != 512) return dm4d_set_error(DM4D_ERR_ARG, "lpips_tap_distance: C must be a VGG-16 width (64, 128, 256, 512)");
  if (tap < 0 || tap >= DM4D_LPIPS_TAPS) return dm4d_set_error(DM4D_ERR_ARG, "lpips_tap_distance: tap outside [0, DM4D_LPIPS_TAPS)");
  if (((uintptr_t)F | (uintptr_t)lin | (uintptr_t)workspace | (uintptr_t)out) & 15)
    return dm4d_set_error(DM4D_ERR_ARG, "lpips_tap_distance: F, lin, workspace and out must be 16-byte aligned");
  if ((size_t)workspace_bytes < dm4d_lpips_ws_bytes(H, W)) return dm4d_set_error(DM4D_ERR_ARG, "lpips_tap_distance: workspace too small (dm4d_lpips_ws_bytes)");
  const int64_t HW = (int64_t)H * W, n = (HW + kDistPixels - 1) / kDistPixels;
  const int L = C / 4 < 64 ? C / 4 : 64;
  hipStream_t st = (hipStream_t)stream;
  if (C == 512)
    hipLaunchKernelGGL(lpips_dist_kernel<2>, dim3((unsigned)n), dim3(kThreads), 0, st, F, lin, HW, C, L, (double*)workspace);
  else
    hipLaunchKernelGGL(lpips_dist_kernel<1>, dim3((unsigned)n), dim3(kThreads), 0, st, F, lin, HW, C, L, (double*)workspace);
  int rc = dm4d_check_launch("lpips_dist_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(lpips_reduce_kernel, dim3(1), dim3(kThreads), 0, st, (const double*)workspace, n, HW, tap, out);
  return dm4d_check_launch("lpips_reduce_kernel");
}
