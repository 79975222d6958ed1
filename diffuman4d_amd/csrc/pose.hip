// 2-D keypoint prediction around a caller-named pose network (diffuman4d_amd/host/pose.py; the reference's predict_keypoints stage:
// scripts/preprocess/sapiens/lite/demo/vis_pose.py preprocess_pose / img_save_and_vis with pose_utils.py top_down_affine_transform and
// udp_decode).  The network is the caller's; the three entries here are the arithmetic on either side of it.
//
//   dm4d_pose_input_u8_f32     composite over black through the mask, bilinear warp of the person box, normalisation, in one launch
//   dm4d_pose_mask_box_u8      bounding box of a mask's pixels >= 128 (the box source a user has without a detector)
//   dm4d_pose_udp_decode_f32   arg-max, 11 x 11 Gaussian modulation, DARK/UDP sub-pixel step, one workgroup per heatmap
//
// The warp and the composite are integer-only from the host's tables on; the normalisation and the decode round every fp32 / fp64
// operation on its own (this file is compiled with -ffp-contract=off; the blur's multiply-adds are written as fmaf()).  No atomics, no
// workgroup waits on another, and a row's / map's result does not depend on the batch around it.
#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "common.h"
#include "dm4d.h"
#include "errors.h"
#include "image_common.h"
#include "pose_rows.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------- network input
constexpr int kInThreads = 256;

struct PoseNorm {
  float mean[3], stdv[3];
};

// grid (ceil(H W / kInThreads), rows): one output pixel per thread, its three channels
__global__ void __launch_bounds__(kInThreads) pose_input_kernel(const uint8_t* __restrict__ staging, const int64_t* __restrict__ desc,
                                                                const int32_t* __restrict__ tab, float* __restrict__ out, int H, int W,
                                                                PoseNorm norm) {
  const int idx = blockIdx.x * kInThreads + threadIdx.x;
  if (idx >= H * W) return;
  const int row = blockIdx.y, y = idx / W, x = idx - y * W;
  const int64_t* d = desc + (int64_t)row * DM4D_POSE_FIELDS;
  const uint8_t* img = staging + d[0];
  const uint8_t* mask = d[1] >= 0 ? staging + d[1] : nullptr;
  const int h = (int)d[2], w = (int)d[3];
  const int32_t* t = tab + d[4];  // {adelta[W] | bdelta[W] | X0[H] | Y0[H]}: 10 fractional bits, the rounding offset inside X0 / Y0
  const int X = (t[2 * W + y] + t[x]) >> 5, Y = (t[2 * W + H + y] + t[W + x]) >> 5;  // 1/32 pixel
  const int sx = X >> 5, sy = Y >> 5, fx = X & 31, fy = Y & 31;
  // the 32 x 32 table of four weights in closed form: 32 (32 - fx)(32 - fy), ...; every entry sums to 32768
  const int wgt[4] = {32 * (32 - fx) * (32 - fy), 32 * fx * (32 - fy), 32 * (32 - fx) * fy, 32 * fx * fy};
  int acc[3] = {0, 0, 0};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int px = sx + (k & 1), py = sy + (k >> 1);
    if (px < 0 || px >= w || py < 0 || py >= h || wgt[k] == 0) continue;  // zero outside the image
    const int64_t at = (int64_t)py * w + px;
    const uint8_t* p = img + at * 3;
    uint32_t c0 = p[0], c1 = p[1], c2 = p[2];
    if (mask) {
      const uint32_t m = mask[at];
      c0 = muldiv255(c0, m), c1 = muldiv255(c1, m), c2 = muldiv255(c2, m);
    }
    acc[0] += wgt[k] * (int)c0, acc[1] += wgt[k] * (int)c1, acc[2] += wgt[k] * (int)c2;
  }
  float* o = out + (int64_t)row * 3 * H * W + idx;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int v = (acc[c] + (1 << 14)) >> 15;
    o[(int64_t)c * H * W] = __fdiv_rn(__fsub_rn((float)v, norm.mean[c]), norm.stdv[c]);
  }
}

// ------------------------------------------------------------------------------------------------------------------------ mask box
constexpr int kBoxThreads = 1024;

// one workgroup per mask: 16-byte loads between a scalar head and tail, shuffles reduce a wave, LDS the workgroup
__global__ void __launch_bounds__(kBoxThreads) pose_mask_box_kernel(const uint8_t* __restrict__ staging, const int64_t* __restrict__ desc,
                                                                    int32_t* __restrict__ boxes) {
  const int tid = threadIdx.x, f = blockIdx.x;
  const int64_t* d = desc + (int64_t)f * DM4D_POSE_FIELDS;
  const int h = (int)d[2], w = (int)d[3];
  Box b{w, h, -1, -1};
  box_scan_plane<1, 0x80808080u>(staging + d[1], (int64_t)h * w, w, tid, kBoxThreads, true, b);
  box_block_reduce<kBoxThreads>(b);
  if (tid == 0) {
    int32_t* dst = boxes + (int64_t)f * 4;
    if (b.lc < 0) {
      dst[0] = 0, dst[1] = 0, dst[2] = w, dst[3] = h;  // an empty mask: the whole image
    } else {
      dst[0] = b.fc, dst[1] = b.fr, dst[2] = b.lc + 1, dst[3] = b.lr + 1;
    }
  }
}

// -------------------------------------------------------------------------------------------------------------------------- decode
constexpr int kDecThreads = 512;
constexpr int kDecWaves = kDecThreads / 64;
constexpr int kTaps = 11, kHalo = 5;   // blur_kernel_size = 11 -> sigma = 0.3 ((11 - 1) / 2 - 1) + 0.8 = 2
constexpr int kBandRows = 32;          // output rows per band at most; the LDS holds them and 2 kHalo rows of horizontal sums
constexpr int kDecStatic = 128;        // bytes set aside for the kernel's static LDS (s_val, s_idx, s_cap)
constexpr int kLdsFloats = (64 * 1024 - kDecStatic) / 4;  // dynamic + static stay within the 64 KiB a launch gets without asking for
                                                          // more, and several workgroups share a CU's 160 KiB
static_assert(kDecWaves * (sizeof(float) + sizeof(int)) + 9 * sizeof(float) <= kDecStatic, "kDecStatic: the static LDS outgrew it");
constexpr int kSeg = 8;                // consecutive outputs per thread and pass: 18 loads feed 8 x 11 multiply-adds

struct PoseTaps {
  float t[kTaps];
};

// the widest map still gets a band of at least one row between its halos
static_assert(kLdsFloats / DM4D_POSE_MAX_HEATMAP_W - 2 * kHalo >= 1, "DM4D_POSE_MAX_HEATMAP_W: a band with its halos must fit kLdsFloats");

__host__ __device__ inline int dec_band_rows(int Wh) {
  const int fit = kLdsFloats / Wh - 2 * kHalo;
  return fit < kBandRows ? fit : kBandRows;
}

__global__ void __launch_bounds__(kDecThreads) pose_udp_decode_kernel(const float* __restrict__ heat, int Hh, int Wh, PoseTaps taps,
                                                                      float* __restrict__ scores, float* __restrict__ locs) {
  extern __shared__ float s_rows[];  // [band + 2 kHalo][Wh]: horizontally blurred rows
  __shared__ float s_val[kDecWaves];
  __shared__ int s_idx[kDecWaves];
  __shared__ float s_cap[9];
  const int tid = threadIdx.x, map = blockIdx.x, HW = Hh * Wh;
  const float* src = heat + (int64_t)map * HW;

  // pass 1: the maximum and its first position in row-major order (np.argmax)
  float best = -INFINITY;
  int bi = INT_MAX;
  for (int i = tid; i < HW; i += kDecThreads) {
    const float v = src[i];
    if (v > best) best = v, bi = i;  // ascending i: the first of equal values stays
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(best, off);
    const int oi = __shfl_xor(bi, off);
    if (ov > best || (ov == best && oi < bi)) best = ov, bi = oi;
  }
  if ((tid & 63) == 0) s_val[tid >> 6] = best, s_idx[tid >> 6] = bi;
  __syncthreads();
  best = s_val[0], bi = s_idx[0];
#pragma unroll
  for (int k = 1; k < kDecWaves; ++k) {
    const float ov = s_val[k];
    const int oi = s_idx[k];
    if (ov > best || (ov == best && oi < bi)) best = ov, bi = oi;
  }
  if (bi == INT_MAX) best = src[0], bi = 0;  // nothing above -inf (non-finite maps are unspecified; the index stays inside the map)
  __syncthreads();                           // s_val is used again below
  if (!(best > 0.f)) {                       // the one deviation from the reference: not refined, the location stays (-1, -1)
    if (tid == 0) scores[map] = best, locs[2 * (int64_t)map] = -1.f, locs[2 * (int64_t)map + 1] = -1.f;
    return;
  }
  const int ay = bi / Wh, ax = bi - ay * Wh;

  // pass 2: zero-padded separable 11-tap blur in row bands; the maximum of the blurred map and its values around the arg-max
  const int band = dec_band_rows(Wh);
  const int nseg = (Wh + kSeg - 1) / kSeg;
  float bmax = -INFINITY;
  for (int r0 = 0; r0 < Hh; r0 += band) {
    const int lo = max(r0 - kHalo, 0), hi = min(r0 + band + kHalo, Hh), r1 = min(r0 + band, Hh);
    for (int it = tid; it < (hi - lo) * nseg; it += kDecThreads) {  // horizontal pass, global -> LDS
      const int rr = it / nseg, x0 = (it - rr * nseg) * kSeg;
      const float* line = src + (int64_t)(lo + rr) * Wh;
      float v[kSeg + kTaps - 1];
#pragma unroll
      for (int j = 0; j < kSeg + kTaps - 1; ++j) {
        const int x = x0 - kHalo + j;
        v[j] = (x >= 0 && x < Wh) ? line[x] : 0.f;
      }
#pragma unroll
      for (int o = 0; o < kSeg; ++o) {
        if (x0 + o >= Wh) break;
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < kTaps; ++k) a = fmaf(taps.t[k], v[o + k], a);
        s_rows[rr * Wh + x0 + o] = a;
      }
    }
    __syncthreads();
    const int nvs = (r1 - r0 + kSeg - 1) / kSeg;
    for (int it = tid; it < nvs * Wh; it += kDecThreads) {  // vertical pass out of the LDS: consecutive threads, consecutive columns
      const int sg = it / Wh, x = it - sg * Wh, y0 = r0 + sg * kSeg;
      float v[kSeg + kTaps - 1];
#pragma unroll
      for (int j = 0; j < kSeg + kTaps - 1; ++j) {
        const int y = y0 - kHalo + j;
        v[j] = (y >= lo && y < hi) ? s_rows[(y - lo) * Wh + x] : 0.f;  // lo / hi cut at the map's rim only: rows outside it are zero
      }
#pragma unroll
      for (int o = 0; o < kSeg; ++o) {
        const int y = y0 + o;
        if (y >= r1) break;
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < kTaps; ++k) a = fmaf(taps.t[k], v[o + k], a);
        bmax = fmaxf(bmax, a);
        if (abs(x - ax) <= 1 && abs(y - ay) <= 1) s_cap[(y - ay + 1) * 3 + (x - ax + 1)] = a;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) bmax = fmaxf(bmax, __shfl_xor(bmax, off));
  if ((tid & 63) == 0) s_val[tid >> 6] = bmax;
  __syncthreads();
  if (tid != 0) return;
  for (int k = 1; k < kDecWaves; ++k) bmax = fmaxf(bmax, s_val[k]);

  // the blurred map times maximum / blurred maximum, clipped, log: the centre c and its neighbours l, r (x -+ 1), u, d (y -+ 1),
  // ul (x - 1, y - 1), dr (x + 1, y + 1), replicated at the map's edge
  const float ratio = __fdiv_rn(best, bmax);
  auto lg = [&](int ox, int oy) -> float {
    const int cx = min(max(ax + ox, 0), Wh - 1) - ax + 1, cy = min(max(ay + oy, 0), Hh - 1) - ay + 1;
    return logf(fminf(fmaxf(s_cap[cy * 3 + cx] * ratio, 1e-3f), 50.f));
  };
  const float c = lg(0, 0), l = lg(-1, 0), r = lg(1, 0), u = lg(0, -1), d = lg(0, 1), ul = lg(-1, -1), dr = lg(1, 1);
  // central differences, every fp32 operation in the order DESIGN.md states ("Keypoint prediction", the DARK step)
  const float gx = (r - l) * 0.5f, gy = (d - u) * 0.5f;
  const float hxx = (r - c * 2.f) + l, hyy = (d - c * 2.f) + u;
  const float terms[7] = {-r, -d, c, c, -l, -u, ul};  // added to dr one by one, in this order
  float cross = dr;
#pragma unroll
  for (int k = 0; k < 7; ++k) cross += terms[k];
  const float hxy = cross * 0.5f;
  // (H + FLT_EPSILON I)^-1 g in fp64 by adjugate / determinant
  const double p = (double)hxx + (double)FLT_EPSILON, q = (double)hyy + (double)FLT_EPSILON, o = (double)hxy;
  const double det = p * q - o * o;
  const double ox = (q * (double)gx - o * (double)gy) / det, oy = (p * (double)gy - o * (double)gx) / det;
  scores[map] = best;
  locs[2 * (int64_t)map] = (float)((double)ax - ox);
  locs[2 * (int64_t)map + 1] = (float)((double)ay - oy);
}

}  // namespace

extern "C" int dm4d_pose_input_u8_f32(void* stream, const void* staging, int64_t staging_bytes, const int64_t* desc_host,
                                      const int64_t* desc_dev, int rows, const int32_t* tab_host, const int32_t* tab_dev, int64_t tab_len,
                                      const float* norm_host, float* out, int H, int W) {
  if (!staging || !desc_host || !desc_dev || !tab_host || !tab_dev || !norm_host || !out)
    return dm4d_set_error(DM4D_ERR_ARG, "pose_input: null pointer");
  if (rows < 1 || rows > 65535) return dm4d_set_error(DM4D_ERR_ARG, "pose_input: rows outside 1..65535");
  if (H < 1 || W < 1 || H > 4096 || W > 4096) return dm4d_set_error(DM4D_ERR_ARG, "pose_input: network input size outside 1..4096");
  if (staging_bytes < 1 || tab_len < 1) return dm4d_set_error(DM4D_ERR_ARG, "pose_input: empty staging buffer or table");
  if (((uintptr_t)out & 3) || ((uintptr_t)tab_dev & 3) || ((uintptr_t)desc_dev & 7))
    return dm4d_set_error(DM4D_ERR_ARG, "pose_input: out, tab_dev (4 bytes) and desc_dev (8 bytes) must be aligned");
  PoseNorm norm;
  for (int c = 0; c < 3; ++c) {
    norm.mean[c] = norm_host[c], norm.stdv[c] = norm_host[3 + c];
    if (!isfinite(norm.mean[c]) || !isfinite(norm.stdv[c]) || norm.stdv[c] == 0.f)
      return dm4d_set_error(DM4D_ERR_ARG, "pose_input: mean must be finite and std finite and non-zero");
  }
  int rc = pose_check_rows("pose_input", staging_bytes, desc_host, rows, true, false, false);
  if (rc) return rc;
  const int64_t per_row = 2 * ((int64_t)W + H);
  for (int r = 0; r < rows; ++r) {
    const int64_t off = desc_host[(int64_t)r * DM4D_POSE_FIELDS + 4];
    if (off < 0 || off > tab_len || per_row > tab_len - off) return dm4d_set_error(DM4D_ERR_ARG, "pose_input: a row's warp table lies outside tab");
    const int32_t* t = tab_host + off;
    for (int64_t k = 0; k < per_row; ++k)
      if (t[k] > DM4D_POSE_TAB_LIMIT || t[k] < -DM4D_POSE_TAB_LIMIT)
        return dm4d_set_error(DM4D_ERR_ARG, "pose_input: a warp table entry is outside +-2^29 (a degenerate or far-away box)");
  }
  hipLaunchKernelGGL(pose_input_kernel, dim3((H * W + kInThreads - 1) / kInThreads, rows), dim3(kInThreads), 0, (hipStream_t)stream,
                     (const uint8_t*)staging, desc_dev, tab_dev, out, H, W, norm);
  return dm4d_check_launch("pose_input_kernel");
}

extern "C" int dm4d_pose_mask_box_u8(void* stream, const void* staging, int64_t staging_bytes, const int64_t* desc_host,
                                     const int64_t* desc_dev, int n, int32_t* boxes) {
  if (!staging || !desc_host || !desc_dev || !boxes) return dm4d_set_error(DM4D_ERR_ARG, "pose_mask_box: null pointer");
  if (n < 1 || n > 65535) return dm4d_set_error(DM4D_ERR_ARG, "pose_mask_box: n outside 1..65535");
  if (staging_bytes < 1) return dm4d_set_error(DM4D_ERR_ARG, "pose_mask_box: empty staging buffer");
  if (((uintptr_t)boxes & 3) || ((uintptr_t)desc_dev & 7))
    return dm4d_set_error(DM4D_ERR_ARG, "pose_mask_box: boxes (4 bytes) and desc_dev (8 bytes) must be aligned");
  const int rc = pose_check_rows("pose_mask_box", staging_bytes, desc_host, n, false, true, false);
  if (rc) return rc;
  hipLaunchKernelGGL(pose_mask_box_kernel, dim3(n), dim3(kBoxThreads), 0, (hipStream_t)stream, (const uint8_t*)staging, desc_dev, boxes);
  return dm4d_check_launch("pose_mask_box_kernel");
}

extern "C" int dm4d_pose_udp_decode_f32(void* stream, const float* heatmaps, int n, int K, int Hh, int Wh, float* scores, float* locs) {
  if (!heatmaps || !scores || !locs) return dm4d_set_error(DM4D_ERR_ARG, "pose_udp_decode: null pointer");
  if (n < 1 || K < 1 || (int64_t)n * K > (1 << 24)) return dm4d_set_error(DM4D_ERR_ARG, "pose_udp_decode: n * K outside 1..2^24");
  if (Hh < 2 || Wh < 2 || Hh > DM4D_POSE_MAX_HEATMAP_H || Wh > DM4D_POSE_MAX_HEATMAP_W)
    return dm4d_set_error(DM4D_ERR_ARG, "pose_udp_decode: heatmap size outside 2..4096 rows x 2..1024 columns");
  if (((uintptr_t)heatmaps & 3) || ((uintptr_t)scores & 3) || ((uintptr_t)locs & 3))
    return dm4d_set_error(DM4D_ERR_ARG, "pose_udp_decode: pointers must be 4-byte aligned");
  // getGaussianKernel(11, sigma = 2): exp(-x^2 / (2 sigma^2)) / sum in fp64, rounded to fp32 once
  PoseTaps taps;
  double g[kTaps], sum = 0.0;
  for (int i = 0; i < kTaps; ++i) {
    const double x = i - kHalo;
    g[i] = exp(-(x * x) / 8.0);
    sum += g[i];
  }
  for (int i = 0; i < kTaps; ++i) taps.t[i] = (float)(g[i] / sum);
  const int band = dec_band_rows(Wh);
  const size_t lds = (size_t)(band + 2 * kHalo) * Wh * sizeof(float);
  hipLaunchKernelGGL(pose_udp_decode_kernel, dim3(n * K), dim3(kDecThreads), lds, (hipStream_t)stream, heatmaps, Hh, Wh, taps, scores, locs);
  return dm4d_check_launch("pose_udp_decode_kernel");
}
