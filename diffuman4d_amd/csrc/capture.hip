// Crop + bicubic resize of captured frames (the input half of the dataset): Pillow's
//   Image.crop((l, t, l + cw, t + ch)).resize((W, H), Image.BICUBIC)
// byte for byte, on the image (RGB), foreground mask (L) and skeleton (RGB) of every frame of a task, followed by the reference's
// fp32 epilogue (TF.to_tensor -> x * 2 - 1, then apply_fmask(white, vae_normalized) on the image).
//
// Pillow's separable filter (libImaging/Resample.c): int32 coefficients with 22 fractional bits, a horizontal pass whose result is
// rounded to uint8, then a vertical pass over it; every output value is clip8((2^21 + sum u * k) >> 22).  Crop pixels outside the
// image are zeros that take part in the sums (Pillow's crop padding).  The coefficient tables are computed on the host
// (diffuman4d_amd/host/resample.py) in float64 exactly as Pillow computes them; this file only applies them, with clip8 and the
// constants of image_common.h (the 7-channel, 4-columns-per-lane register layout of its two loops is its own).
//
// This translation unit is compiled with -ffp-contract=off (build.py EXTRA_FLAGS): the epilogue rounds every fp32 operation on its
// own, as PyTorch's CPU kernels do, and a contracted multiply-add would change the last bit.
#include <stdint.h>

#include "common.h"
#include "dm4d.h"
#include "errors.h"
#include "image_common.h"

namespace {

constexpr int kThreads = 64;

// descriptor fields (int64 each, DM4D_CAPTURE_FIELDS per frame), see dm4d.h
enum {
  F_IMG = 0, F_MASK, F_SKEL, F_SRC_H, F_SRC_W, F_TOP, F_LEFT, F_CROP_H, F_CROP_W, F_HTAB, F_HK, F_VTAB, F_VK, F_SCRATCH, F_YFIRST, F_NROWS
};

// Horizontal pass: one lane = 4 consecutive output columns of one scratch row, all 7 channels (image RGB, mask, skeleton RGB);
// scratch pixel = 8 bytes {i0 i1 i2 m s0 s1 s2 0}, a lane stores 32 contiguous bytes.
__global__ void __launch_bounds__(kThreads) capture_hpass_kernel(const uint8_t* __restrict__ stage, const int64_t* __restrict__ desc,
                                                                 const int32_t* __restrict__ tab, uint8_t* __restrict__ scratch, int W) {
  const int64_t* d = desc + (int64_t)blockIdx.z * DM4D_CAPTURE_FIELDS;
  const int r = blockIdx.y;
  const int x0 = (blockIdx.x * kThreads + threadIdx.x) * 4;
  if (r >= (int)d[F_NROWS] || x0 >= W) return;
  const int src_h = (int)d[F_SRC_H], src_w = (int)d[F_SRC_W];
  const int sy = (int)d[F_TOP] + (int)d[F_YFIRST] + r;
  const bool row_ok = sy >= 0 && sy < src_h;
  const int left = (int)d[F_LEFT];
  const int ksize = (int)d[F_HK];
  const int32_t* bounds = tab + d[F_HTAB];
  const int32_t* coefs = bounds + 2 * W;
  const uint8_t* img = stage + d[F_IMG] + (int64_t)sy * src_w * 3;
  const uint8_t* msk = stage + d[F_MASK] + (int64_t)sy * src_w;
  const uint8_t* skl = stage + d[F_SKEL] + (int64_t)sy * src_w * 3;
  uint32_t out[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ox = x0 + j;
    int32_t acc[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) acc[c] = kPillowHalf;
    if (row_ok) {
      const int xmin = bounds[2 * ox], cnt = bounds[2 * ox + 1];
      const int32_t* k = coefs + (int64_t)ox * ksize;
      for (int t = 0; t < cnt; ++t) {
        const int sx = left + xmin + t;
        if (sx < 0 || sx >= src_w) continue;  // zero padding: adds nothing
        const int32_t w = k[t];
        acc[0] += (int32_t)img[3 * sx] * w;
        acc[1] += (int32_t)img[3 * sx + 1] * w;
        acc[2] += (int32_t)img[3 * sx + 2] * w;
        acc[3] += (int32_t)msk[sx] * w;
        acc[4] += (int32_t)skl[3 * sx] * w;
        acc[5] += (int32_t)skl[3 * sx + 1] * w;
        acc[6] += (int32_t)skl[3 * sx + 2] * w;
      }
    }
    out[2 * j] = clip8(acc[0]) | (clip8(acc[1]) << 8) | (clip8(acc[2]) << 16) | (clip8(acc[3]) << 24);
    out[2 * j + 1] = clip8(acc[4]) | (clip8(acc[5]) << 8) | (clip8(acc[6]) << 16);
  }
  U4* dst = reinterpret_cast<U4*>(scratch + d[F_SCRATCH] + ((int64_t)r * W + x0) * 8);
  dst[0] = U4{out[0], out[1], out[2], out[3]};
  dst[1] = U4{out[4], out[5], out[6], out[7]};
}

// TF.to_tensor(u8) * 2 - 1: a true division, then two separately rounded operations
__device__ __forceinline__ float unit(uint32_t u) { return __fdiv_rn((float)u, 255.0f) * 2.0f - 1.0f; }

// Vertical pass + epilogue: one lane = 4 consecutive output columns of one output row; reads 32 bytes of each scratch row of its
// window, writes 16 bytes to each of the 3 pixel_values and 3 skeleton planes.
__global__ void __launch_bounds__(kThreads) capture_vpass_kernel(const int64_t* __restrict__ desc, const int32_t* __restrict__ tab,
                                                                 const uint8_t* __restrict__ scratch, float* __restrict__ pix,
                                                                 float* __restrict__ skel, int H, int W) {
  const int f = blockIdx.z;
  const int64_t* d = desc + (int64_t)f * DM4D_CAPTURE_FIELDS;
  const int oy = blockIdx.y;
  const int x0 = (blockIdx.x * kThreads + threadIdx.x) * 4;
  if (x0 >= W) return;
  const int ksize = (int)d[F_VK];
  const int32_t* bounds = tab + d[F_VTAB];
  const int32_t* k = bounds + 2 * H + (int64_t)oy * ksize;
  const int ymin = bounds[2 * oy] - (int)d[F_YFIRST], cnt = bounds[2 * oy + 1];
  const uint8_t* col = scratch + d[F_SCRATCH] + (int64_t)x0 * 8;
  int32_t acc[4][7];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int c = 0; c < 7; ++c) acc[j][c] = kPillowHalf;
  for (int t = 0; t < cnt; ++t) {
    const U4* row = reinterpret_cast<const U4*>(col + (int64_t)(ymin + t) * W * 8);
    const U4 a = row[0], b = row[1];
    const uint32_t v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    const int32_t w = k[t];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int c = 0; c < 7; ++c) acc[j][c] += (int32_t)((v[2 * j + (c >> 2)] >> (8 * (c & 3))) & 0xffu) * w;
  }
  float pv[3][4], sk[3][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    // apply_fmask(image, fmask, "white", vae_normalized=True): both operands * 0.5 + 0.5, image * m + (1 - m) * 1, then * 2 - 1
    const float m = unit(clip8(acc[j][3])) * 0.5f + 0.5f;
    const float bg = 1.0f - m;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float i = unit(clip8(acc[j][c])) * 0.5f + 0.5f;
      pv[c][j] = (i * m + bg) * 2.0f - 1.0f;
      sk[c][j] = unit(clip8(acc[j][4 + c]));
    }
  }
  const int64_t plane = (int64_t)H * W;
  const int64_t o = (int64_t)f * 3 * plane + (int64_t)oy * W + x0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    *reinterpret_cast<f32x4_t*>(pix + o + c * plane) = f32x4_t{pv[c][0], pv[c][1], pv[c][2], pv[c][3]};
    *reinterpret_cast<f32x4_t*>(skel + o + c * plane) = f32x4_t{sk[c][0], sk[c][1], sk[c][2], sk[c][3]};
  }
}

}  // namespace

extern "C" int dm4d_capture_crop_resize_f32(void* stream, const void* staging, int64_t staging_bytes, const int64_t* desc_host,
                                            const int64_t* desc_dev, int n_frames, const int32_t* tab_host, const int32_t* tab_dev,
                                            int64_t tab_len, void* scratch, int64_t scratch_bytes, float* pixel_values, float* skeletons,
                                            int H, int W) {
  if (!staging || !desc_host || !desc_dev || !tab_host || !tab_dev || !scratch || !pixel_values || !skeletons)
    return dm4d_set_error(DM4D_ERR_ARG, "capture_crop_resize: null pointer");
  if (n_frames <= 0 || n_frames > 65535 || H <= 0 || W <= 0 || H > 65535 || W > (1 << 20) || staging_bytes <= 0 || tab_len <= 0 ||
      scratch_bytes <= 0)
    return dm4d_set_error(DM4D_ERR_ARG, "capture_crop_resize: empty or oversized shape");
  if (W % 4 != 0) return dm4d_set_error(DM4D_ERR_ARG, "capture_crop_resize: W must be a multiple of 4");
  if (((uintptr_t)scratch | (uintptr_t)pixel_values | (uintptr_t)skeletons) & 15)
    return dm4d_set_error(DM4D_ERR_ARG, "capture_crop_resize: scratch and outputs must be 16-byte aligned");
  int max_rows = 0;
  for (int f = 0; f < n_frames; ++f) {
    const int64_t* d = desc_host + (int64_t)f * DM4D_CAPTURE_FIELDS;
    const int64_t sh = d[F_SRC_H], sw = d[F_SRC_W], ch = d[F_CROP_H], cw = d[F_CROP_W];
    if (sh <= 0 || sw <= 0 || sh > (1 << 16) || sw > (1 << 16) || ch <= 0 || cw <= 0 || ch > (1 << 20) || cw > (1 << 20) ||
        d[F_TOP] < -(1 << 20) || d[F_TOP] > (1 << 20) || d[F_LEFT] < -(1 << 20) || d[F_LEFT] > (1 << 20))
      return dm4d_set_error(DM4D_ERR_ARG, "capture_crop_resize: bad frame or crop size in a descriptor");
    if (d[F_IMG] < 0 || d[F_IMG] + sh * sw * 3 > staging_bytes || d[F_MASK] < 0 || d[F_MASK] + sh * sw > staging_bytes ||
        d[F_SKEL] < 0 || d[F_SKEL] + sh * sw * 3 > staging_bytes)
      return dm4d_set_error(DM4D_ERR_ARG, "capture_crop_resize: a source plane lies outside the staging buffer");
    if (!pillow_table_ok(tab_host, tab_len, d[F_HTAB], d[F_HK], 1 << 16, W, cw, false) ||
        !pillow_table_ok(tab_host, tab_len, d[F_VTAB], d[F_VK], 1 << 16, H, ch, false))
      return dm4d_set_error(DM4D_ERR_ARG, "capture_crop_resize: a coefficient table is out of range or its windows leave the crop");
    const int64_t y_first = d[F_YFIRST], n_rows = d[F_NROWS];
    if (y_first < 0 || n_rows < 1 || n_rows > 65535 || y_first + n_rows > ch)
      return dm4d_set_error(DM4D_ERR_ARG, "capture_crop_resize: bad scratch row range");
    for (int i = 0; i < H; ++i) {  // every vertical window inside the rows the horizontal pass produces
      const int64_t y0 = tab_host[d[F_VTAB] + 2 * i], cnt = tab_host[d[F_VTAB] + 2 * i + 1];
      if (y0 < y_first || y0 + cnt > y_first + n_rows)
        return dm4d_set_error(DM4D_ERR_ARG, "capture_crop_resize: a vertical window leaves the scratch rows");
    }
    if (d[F_SCRATCH] < 0 || (d[F_SCRATCH] & 15) || d[F_SCRATCH] + n_rows * W * 8 > scratch_bytes)
      return dm4d_set_error(DM4D_ERR_ARG, "capture_crop_resize: scratch region out of range or not 16-byte aligned");
    if (n_rows > max_rows) max_rows = (int)n_rows;
  }
  const dim3 block(kThreads);
  const unsigned gx = (unsigned)((W / 4 + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(capture_hpass_kernel, dim3(gx, max_rows, n_frames), block, 0, (hipStream_t)stream, (const uint8_t*)staging,
                     desc_dev, tab_dev, (uint8_t*)scratch, W);
  int rc = dm4d_check_launch("capture_hpass_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(capture_vpass_kernel, dim3(gx, H, n_frames), block, 0, (hipStream_t)stream, desc_dev, tab_dev,
                     (const uint8_t*)scratch, pixel_values, skeletons, H, W);
  return dm4d_check_launch("capture_vpass_kernel");
}
