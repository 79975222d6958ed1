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
// The device cell cache (host/capture_cache.py) splits the same arithmetic at the epilogue: dm4d_capture_crop_resize_packed_u8 is the two
// passes with the vertical one storing its clip8 values as 8-byte pixels into caller-named cells, dm4d_capture_unpack_cells_f32 applies
// the epilogue to cells.  The epilogue is one function, capture_epilogue, for both.
//
// This translation unit is compiled with -ffp-contract=off (build.py EXTRA_FLAGS): the epilogue rounds every fp32 operation on its
// own, as PyTorch's CPU kernels do, and a contracted multiply-add would change the last bit.
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

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

// The dataset's fp32 epilogue of one resized pixel {i0 i1 i2 m s0 s1 s2}: the one copy, for the fused vertical pass and for the cells.
// apply_fmask(image, fmask, "white", vae_normalized=True): both operands * 0.5 + 0.5, image * m + (1 - m) * 1, then * 2 - 1
__device__ __forceinline__ void capture_epilogue(uint32_t i0, uint32_t i1, uint32_t i2, uint32_t mask, uint32_t s0, uint32_t s1, uint32_t s2,
                                                 float (&pv)[3], float (&sk)[3]) {
  const float m = unit(mask) * 0.5f + 0.5f;
  const float bg = 1.0f - m;
  const uint32_t img[3] = {i0, i1, i2}, skl[3] = {s0, s1, s2};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float i = unit(img[c]) * 0.5f + 0.5f;
    pv[c] = (i * m + bg) * 2.0f - 1.0f;
    sk[c] = unit(skl[c]);
  }
}

// 4 columns of one row of 3 + 3 fp32 planes: px[j] = the 7 bytes of column x0 + j; o = the offset of (row, x0) in plane 0
__device__ __forceinline__ void capture_store_planes(const uint32_t (&px)[4][7], float* __restrict__ pix, float* __restrict__ skel, int64_t o,
                                                     int64_t plane) {
  float pv[3][4], sk[3][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float p[3], s[3];
    capture_epilogue(px[j][0], px[j][1], px[j][2], px[j][3], px[j][4], px[j][5], px[j][6], p, s);
#pragma unroll
    for (int c = 0; c < 3; ++c) pv[c][j] = p[c], sk[c][j] = s[c];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    *reinterpret_cast<f32x4_t*>(pix + o + c * plane) = f32x4_t{pv[c][0], pv[c][1], pv[c][2], pv[c][3]};
    *reinterpret_cast<f32x4_t*>(skel + o + c * plane) = f32x4_t{sk[c][0], sk[c][1], sk[c][2], sk[c][3]};
  }
}

// cell descriptor fields (int64 each, DM4D_CAPTURE_CELL_FIELDS per row), see dm4d.h
enum { C_SLAB = 0, C_BYTES, C_OFF, C_ROW };

__device__ __forceinline__ uint8_t* cell_base(const int64_t* __restrict__ c) {
  return reinterpret_cast<uint8_t*>((uintptr_t)c[C_SLAB]) + c[C_OFF];
}

// Vertical pass: one lane = 4 consecutive output columns of one output row; reads 32 bytes of each scratch row of its window.
// kPacked = false: + epilogue, 16 bytes to each of the 3 pixel_values and 3 skeleton planes of frame f.
// kPacked = true:  the clip8 values themselves, 32 bytes {i0 i1 i2 m s0 s1 s2 0} x 4 into cell f (the scratch row format).
template <bool kPacked>
__global__ void __launch_bounds__(kThreads) capture_vpass_kernel(const int64_t* __restrict__ desc, const int32_t* __restrict__ tab,
                                                                 const uint8_t* __restrict__ scratch, float* __restrict__ pix,
                                                                 float* __restrict__ skel, const int64_t* __restrict__ cells, int H, int W) {
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
  uint32_t px[4][7];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int c = 0; c < 7; ++c) px[j][c] = clip8(acc[j][c]);
  if constexpr (kPacked) {
    uint32_t out[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      out[2 * j] = px[j][0] | (px[j][1] << 8) | (px[j][2] << 16) | (px[j][3] << 24);
      out[2 * j + 1] = px[j][4] | (px[j][5] << 8) | (px[j][6] << 16);
    }
    U4* dst = reinterpret_cast<U4*>(cell_base(cells + (int64_t)f * DM4D_CAPTURE_CELL_FIELDS) + ((int64_t)oy * W + x0) * 8);
    dst[0] = U4{out[0], out[1], out[2], out[3]};
    dst[1] = U4{out[4], out[5], out[6], out[7]};
  } else {
    const int64_t plane = (int64_t)H * W;
    capture_store_planes(px, pix, skel, (int64_t)f * 3 * plane + (int64_t)oy * W + x0, plane);
  }
}

// Cells -> samples: one lane = 4 consecutive columns of one row of one cell; one 32-byte load, the epilogue, six 16-byte stores into
// row cells[r][C_ROW] of pixel_values / skeletons.  Rows no descriptor names are not touched.
__global__ void __launch_bounds__(kThreads) capture_unpack_kernel(const int64_t* __restrict__ cells, float* __restrict__ pix,
                                                                  float* __restrict__ skel, int H, int W) {
  const int64_t* c = cells + (int64_t)blockIdx.z * DM4D_CAPTURE_CELL_FIELDS;
  const int oy = blockIdx.y;
  const int x0 = (blockIdx.x * kThreads + threadIdx.x) * 4;
  if (x0 >= W) return;
  const U4* src = reinterpret_cast<const U4*>(cell_base(c) + ((int64_t)oy * W + x0) * 8);
  const U4 a = src[0], b = src[1];
  const uint32_t v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  uint32_t px[4][7];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int ch = 0; ch < 7; ++ch) px[j][ch] = (v[2 * j + (ch >> 2)] >> (8 * (ch & 3))) & 0xffu;
  const int64_t plane = (int64_t)H * W;
  capture_store_planes(px, pix, skel, c[C_ROW] * 3 * plane + (int64_t)oy * W + x0, plane);
}

// What dm4d_capture_crop_resize_f32 and dm4d_capture_crop_resize_packed_u8 check alike, in the order the first always had: `other_null`
// and `other_bits` stand for the pointers that are the entry's own (any of them null; the OR of those that must be 16-byte aligned).
int capture_check_resize(const void* staging, int64_t staging_bytes, const int64_t* desc_host, const int64_t* desc_dev, int n_frames,
                         const int32_t* tab_host, const int32_t* tab_dev, int64_t tab_len, const void* scratch, int64_t scratch_bytes,
                         bool other_null, uintptr_t other_bits, int H, int W, int* max_rows_out) {
  if (!staging || !desc_host || !desc_dev || !tab_host || !tab_dev || !scratch || other_null)
    return dm4d_set_error(DM4D_ERR_ARG, "capture_crop_resize: null pointer");
  if (n_frames <= 0 || n_frames > 65535 || H <= 0 || W <= 0 || H > 65535 || W > (1 << 20) || staging_bytes <= 0 || tab_len <= 0 ||
      scratch_bytes <= 0)
    return dm4d_set_error(DM4D_ERR_ARG, "capture_crop_resize: empty or oversized shape");
  if (W % 4 != 0) return dm4d_set_error(DM4D_ERR_ARG, "capture_crop_resize: W must be a multiple of 4");
  if (((uintptr_t)scratch | other_bits) & 15)
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
  *max_rows_out = max_rows;
  return 0;
}

// Every cell of `n` descriptors a whole H x W x 8-byte region of its slab, on a 16-byte address
int capture_check_cells(const int64_t* cell_host, int n, int H, int W) {
  const int64_t cell_bytes = (int64_t)H * W * 8;
  for (int r = 0; r < n; ++r) {
    const int64_t* c = cell_host + (int64_t)r * DM4D_CAPTURE_CELL_FIELDS;
    if (c[C_SLAB] == 0 || (c[C_SLAB] & 15)) return dm4d_set_error(DM4D_ERR_ARG, "capture_cells: a slab address is zero or not 16-byte aligned");
    if (c[C_OFF] < 0 || (c[C_OFF] & 15) || c[C_BYTES] < cell_bytes || c[C_OFF] > c[C_BYTES] - cell_bytes)
      return dm4d_set_error(DM4D_ERR_ARG, "capture_cells: a cell's offset is negative, not 16-byte aligned or the cell leaves its slab");
  }
  return 0;
}

void capture_launch_hpass(hipStream_t stream, const void* staging, const int64_t* desc_dev, const int32_t* tab_dev, void* scratch,
                          int max_rows, int n_frames, int W) {
  const unsigned gx = (unsigned)((W / 4 + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(capture_hpass_kernel, dim3(gx, max_rows, n_frames), dim3(kThreads), 0, stream, (const uint8_t*)staging, desc_dev,
                     tab_dev, (uint8_t*)scratch, W);
}

}  // namespace

extern "C" int dm4d_capture_crop_resize_f32(void* stream, const void* staging, int64_t staging_bytes, const int64_t* desc_host,
                                            const int64_t* desc_dev, int n_frames, const int32_t* tab_host, const int32_t* tab_dev,
                                            int64_t tab_len, void* scratch, int64_t scratch_bytes, float* pixel_values, float* skeletons,
                                            int H, int W) {
  int max_rows = 0;
  int rc = capture_check_resize(staging, staging_bytes, desc_host, desc_dev, n_frames, tab_host, tab_dev, tab_len, scratch, scratch_bytes,
                                !pixel_values || !skeletons, (uintptr_t)pixel_values | (uintptr_t)skeletons, H, W, &max_rows);
  if (rc) return rc;
  capture_launch_hpass((hipStream_t)stream, staging, desc_dev, tab_dev, scratch, max_rows, n_frames, W);
  rc = dm4d_check_launch("capture_hpass_kernel");
  if (rc) return rc;
  const unsigned gx = (unsigned)((W / 4 + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(capture_vpass_kernel<false>, dim3(gx, H, n_frames), dim3(kThreads), 0, (hipStream_t)stream, desc_dev, tab_dev,
                     (const uint8_t*)scratch, pixel_values, skeletons, (const int64_t*)nullptr, H, W);
  return dm4d_check_launch("capture_vpass_kernel");
}

extern "C" int dm4d_capture_crop_resize_packed_u8(void* stream, const void* staging, int64_t staging_bytes, const int64_t* desc_host,
                                                  const int64_t* desc_dev, int n_frames, const int32_t* tab_host, const int32_t* tab_dev,
                                                  int64_t tab_len, void* scratch, int64_t scratch_bytes, const int64_t* cell_host,
                                                  const int64_t* cell_dev, int H, int W) {
  int max_rows = 0;
  int rc = capture_check_resize(staging, staging_bytes, desc_host, desc_dev, n_frames, tab_host, tab_dev, tab_len, scratch, scratch_bytes,
                                !cell_host || !cell_dev, 0, H, W, &max_rows);
  if (rc) return rc;
  if ((uintptr_t)cell_dev & 7) return dm4d_set_error(DM4D_ERR_ARG, "capture_crop_resize_packed: cell_dev must be 8-byte aligned");
  rc = capture_check_cells(cell_host, n_frames, H, W);
  if (rc) return rc;
  std::vector<std::pair<int64_t, int64_t>> at(n_frames);  // (slab, offset) of every frame: no two alike
  for (int f = 0; f < n_frames; ++f) at[f] = {cell_host[(int64_t)f * DM4D_CAPTURE_CELL_FIELDS + C_SLAB], cell_host[(int64_t)f * DM4D_CAPTURE_CELL_FIELDS + C_OFF]};
  std::sort(at.begin(), at.end());
  if (std::adjacent_find(at.begin(), at.end()) != at.end())
    return dm4d_set_error(DM4D_ERR_ARG, "capture_crop_resize_packed: two frames name the same cell");
  capture_launch_hpass((hipStream_t)stream, staging, desc_dev, tab_dev, scratch, max_rows, n_frames, W);
  rc = dm4d_check_launch("capture_hpass_kernel");
  if (rc) return rc;
  const unsigned gx = (unsigned)((W / 4 + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(capture_vpass_kernel<true>, dim3(gx, H, n_frames), dim3(kThreads), 0, (hipStream_t)stream, desc_dev, tab_dev,
                     (const uint8_t*)scratch, (float*)nullptr, (float*)nullptr, cell_dev, H, W);
  return dm4d_check_launch("capture_vpass_kernel<packed>");
}

extern "C" int dm4d_capture_unpack_cells_f32(void* stream, const int64_t* cell_host, const int64_t* cell_dev, int n_rows, float* pixel_values,
                                             float* skeletons, int n_out_rows, int H, int W) {
  if (!cell_host || !cell_dev || !pixel_values || !skeletons) return dm4d_set_error(DM4D_ERR_ARG, "capture_unpack_cells: null pointer");
  if (n_rows <= 0 || n_rows > 65535 || n_out_rows <= 0 || n_out_rows > 65535 || H <= 0 || W <= 0 || H > 65535 || W > (1 << 20))
    return dm4d_set_error(DM4D_ERR_ARG, "capture_unpack_cells: empty or oversized shape");
  if (W % 4 != 0) return dm4d_set_error(DM4D_ERR_ARG, "capture_unpack_cells: W must be a multiple of 4");
  if ((((uintptr_t)pixel_values | (uintptr_t)skeletons) & 15) || ((uintptr_t)cell_dev & 7))
    return dm4d_set_error(DM4D_ERR_ARG, "capture_unpack_cells: outputs (16 bytes) and cell_dev (8 bytes) must be aligned");
  int rc = capture_check_cells(cell_host, n_rows, H, W);
  if (rc) return rc;
  std::vector<char> named(n_out_rows, 0);
  for (int r = 0; r < n_rows; ++r) {
    const int64_t row = cell_host[(int64_t)r * DM4D_CAPTURE_CELL_FIELDS + C_ROW];
    if (row < 0 || row >= n_out_rows) return dm4d_set_error(DM4D_ERR_ARG, "capture_unpack_cells: an output row is outside [0, n_out_rows)");
    if (named[row]) return dm4d_set_error(DM4D_ERR_ARG, "capture_unpack_cells: two rows name the same output row");
    named[row] = 1;
  }
  const unsigned gx = (unsigned)((W / 4 + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(capture_unpack_kernel, dim3(gx, H, n_rows), dim3(kThreads), 0, (hipStream_t)stream, cell_dev, pixel_values, skeletons, H,
                     W);
  return dm4d_check_launch("capture_unpack_kernel");
}

// Box and byte sum of decoded planes, and masks that are filled rectangles: what SpaTemDataset(device_decode=True) needs of planes that
// were decoded on the device and never visit the host (the crop box, the empty and 2 % checks, the has_gt_target=False box mask).
//
//   partial  grid (blocks, planes): a block walks its share of its plane's 16-byte vectors (planes start on 16-byte addresses; the tail
//            of up to 15 bytes goes to block 0).  An all-zero vector costs one load and one test; any other adds its bytes (four
//            sums of absolute differences against 0) and is walked by box_scan_word.  Shuffles reduce a wave, LDS the block, and
//            thread 0 stores {first column, first row, last column, last row, sum} in the workspace.  Planes differ in size: a
//            plane uses the first stats_blocks(its bytes) blocks of its grid row, the others leave at once.
//   fold     one wave per plane folds its partials (a fixed assignment to lanes, then the shuffle tree) into out[plane].
//   fill     grid (blocks, planes): rect_fill_plane of every descriptor's rectangle.
//
// min, max and sums of integers: no atomics, no block waits on another, and a plane's row does not depend on the batch it is in.
namespace {

constexpr int kStatsThreads = 256;
constexpr int kStatsMaxBlocks = 256;    // per plane
constexpr int kStatsVecsPerThread = 8;  // 32 KiB of a plane per block before the grid stride sets in
constexpr int kStatsMaxSide = 1 << 15;  // h * w * 3 stays below 2^32

enum { S_OFF = 0, S_H, S_W, S_CH };                       // DM4D_CAPTURE_PLANE_FIELDS
enum { R_OFF = 0, R_H, R_W, R_C0, R_R0, R_C1, R_R1 };     // DM4D_CAPTURE_RECT_FIELDS

__host__ __device__ inline int stats_blocks(int64_t plane_bytes) {
  const int64_t per_block = (int64_t)kStatsThreads * kStatsVecsPerThread * 16;
  const int64_t n = (plane_bytes + per_block - 1) / per_block;
  return (int)(n < 1 ? 1 : n > kStatsMaxBlocks ? kStatsMaxBlocks : n);
}

__device__ __forceinline__ uint32_t byte_sum(uint32_t word, uint32_t acc) { return __builtin_amdgcn_sad_u8(word, 0u, acc); }

template <int BPP>
__device__ __forceinline__ void stats_scan_plane(const uint8_t* __restrict__ src, int64_t total_bytes, int row_bytes, int64_t first_vec,
                                                 int64_t vec_stride, bool do_tail, Box& b, int64_t& sum) {
  const int64_t nvec = total_bytes / 16;
  for (int64_t v = first_vec; v < nvec; v += vec_stride) {
    const int64_t at = v * 16;
    const U4 q = ldg16(src + at);
    if ((q.x | q.y | q.z | q.w) == 0) continue;
    sum += byte_sum(q.x, byte_sum(q.y, byte_sum(q.z, byte_sum(q.w, 0u))));
    box_scan_word<BPP, 0xffffffffu>(b, q.x, 4, at, row_bytes);
    box_scan_word<BPP, 0xffffffffu>(b, q.y, 4, at + 4, row_bytes);
    box_scan_word<BPP, 0xffffffffu>(b, q.z, 4, at + 8, row_bytes);
    box_scan_word<BPP, 0xffffffffu>(b, q.w, 4, at + 12, row_bytes);
  }
  if (do_tail) {
    const int64_t t = nvec * 16 + threadIdx.x;
    if (t < total_bytes) {
      const uint32_t v = src[t];
      sum += v;
      box_scan_word<BPP, 0xffffffffu>(b, v, 1, t, row_bytes);
    }
  }
}

__device__ __forceinline__ int64_t sum_wave_reduce(int64_t s) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  return s;
}

__global__ void __launch_bounds__(kStatsThreads) capture_stats_partial_kernel(const uint8_t* __restrict__ blob, const int64_t* __restrict__ desc,
                                                                              int64_t* __restrict__ partials) {
  __shared__ int64_t s_sum[kStatsThreads / 64];
  const int tid = threadIdx.x, p = blockIdx.y;
  const int64_t* d = desc + (int64_t)p * DM4D_CAPTURE_PLANE_FIELDS;
  const int h = (int)d[S_H], w = (int)d[S_W], ch = (int)d[S_CH];
  const int64_t plane_bytes = (int64_t)h * w * ch;
  const int nblocks = stats_blocks(plane_bytes);
  if ((int)blockIdx.x >= nblocks) return;  // the same for every thread of the block
  Box b{w, h, -1, -1};
  int64_t sum = 0;
  const uint8_t* src = blob + d[S_OFF];
  const int64_t first = (int64_t)blockIdx.x * kStatsThreads + tid, stride = (int64_t)nblocks * kStatsThreads;
  if (ch == 3)
    stats_scan_plane<3>(src, plane_bytes, w * 3, first, stride, blockIdx.x == 0, b, sum);
  else
    stats_scan_plane<1>(src, plane_bytes, w, first, stride, blockIdx.x == 0, b, sum);
  sum = sum_wave_reduce(sum);
  if ((tid & 63) == 0) s_sum[tid >> 6] = sum;
  box_block_reduce<kStatsThreads>(b);  // its barrier also publishes s_sum
  if (tid == 0) {
    for (int k = 1; k < kStatsThreads / 64; ++k) sum += s_sum[k];
    int64_t* dst = partials + ((int64_t)p * gridDim.x + blockIdx.x) * 5;
    dst[0] = b.fc, dst[1] = b.fr, dst[2] = b.lc, dst[3] = b.lr, dst[4] = sum;
  }
}

__global__ void __launch_bounds__(64) capture_stats_fold_kernel(const int64_t* __restrict__ desc, const int64_t* __restrict__ partials,
                                                                int row_blocks, int64_t* __restrict__ out) {
  const int p = blockIdx.x, lane = threadIdx.x;  // one wave per plane
  const int64_t* d = desc + (int64_t)p * DM4D_CAPTURE_PLANE_FIELDS;
  const int h = (int)d[S_H], w = (int)d[S_W];
  const int nblocks = stats_blocks((int64_t)h * w * d[S_CH]);
  Box b{w, h, -1, -1};
  int64_t sum = 0;
  const int64_t* src = partials + (int64_t)p * row_blocks * 5;
  for (int k = lane; k < nblocks; k += 64) {
    box_merge(b, Box{(int)src[5 * k], (int)src[5 * k + 1], (int)src[5 * k + 2], (int)src[5 * k + 3]});
    sum += src[5 * k + 4];
  }
  box_wave_reduce(b);
  sum = sum_wave_reduce(sum);
  if (lane == 0) {
    int64_t* dst = out + (int64_t)p * 5;
    dst[0] = b.fc, dst[1] = b.fr, dst[2] = b.lc, dst[3] = b.lr, dst[4] = sum;
  }
}

__global__ void __launch_bounds__(kStatsThreads) capture_fill_rects_kernel(uint8_t* __restrict__ blob, const int64_t* __restrict__ desc) {
  const int64_t* d = desc + (int64_t)blockIdx.y * DM4D_CAPTURE_RECT_FIELDS;
  rect_fill_plane(blob + d[R_OFF], (int)d[R_H], (int)d[R_W], (int)d[R_C0], (int)d[R_R0], (int)d[R_C1], (int)d[R_R1],
                  (int64_t)blockIdx.x * kStatsThreads + threadIdx.x, (int64_t)gridDim.x * kStatsThreads, blockIdx.x == 0);
}

}  // namespace

extern "C" size_t dm4d_capture_plane_stats_ws_bytes(int n, int64_t max_plane_bytes) {
  if (n <= 0 || n > 65535 || max_plane_bytes <= 0 || max_plane_bytes > (int64_t)kStatsMaxSide * kStatsMaxSide * 3) return 0;
  return (size_t)n * stats_blocks(max_plane_bytes) * 5 * sizeof(int64_t);
}

extern "C" int dm4d_capture_plane_stats_u8(void* stream, const void* blob, int64_t blob_bytes, const int64_t* desc_host, const int64_t* desc_dev,
                                           int n, int64_t* out, void* ws, int64_t ws_bytes) {
  if (!blob || !desc_host || !desc_dev || !out || !ws) return dm4d_set_error(DM4D_ERR_ARG, "capture_plane_stats: null pointer");
  if (n < 1 || n > 65535) return dm4d_set_error(DM4D_ERR_ARG, "capture_plane_stats: n outside 1..65535");
  if (blob_bytes < 1) return dm4d_set_error(DM4D_ERR_ARG, "capture_plane_stats: empty blob");
  if (((uintptr_t)blob & 15) || ((uintptr_t)desc_dev & 7) || ((uintptr_t)out & 7) || ((uintptr_t)ws & 7))
    return dm4d_set_error(DM4D_ERR_ARG, "capture_plane_stats: blob (16 bytes), desc_dev, out and workspace (8 bytes) must be aligned");
  int64_t max_bytes = 0;
  for (int p = 0; p < n; ++p) {
    const int64_t* d = desc_host + (int64_t)p * DM4D_CAPTURE_PLANE_FIELDS;
    const int64_t off = d[S_OFF], h = d[S_H], w = d[S_W], ch = d[S_CH];
    if (h < 1 || w < 1 || h > kStatsMaxSide || w > kStatsMaxSide) return dm4d_set_error(DM4D_ERR_ARG, "capture_plane_stats: a plane's size is outside 1..32768");
    if (ch != 1 && ch != 3) return dm4d_set_error(DM4D_ERR_ARG, "capture_plane_stats: channels must be 1 or 3");
    if (off & 15) return dm4d_set_error(DM4D_ERR_ARG, "capture_plane_stats: a plane's offset is not 16-byte aligned");
    if (off < 0 || off > blob_bytes || h * w * ch > blob_bytes - off) return dm4d_set_error(DM4D_ERR_ARG, "capture_plane_stats: a plane lies outside the blob");
    if (h * w * ch > max_bytes) max_bytes = h * w * ch;
  }
  if (ws_bytes < 0 || (size_t)ws_bytes < dm4d_capture_plane_stats_ws_bytes(n, max_bytes))
    return dm4d_set_error(DM4D_ERR_ARG, "capture_plane_stats: the workspace is smaller than dm4d_capture_plane_stats_ws_bytes");
  const hipStream_t s = (hipStream_t)stream;
  const int nb = stats_blocks(max_bytes);
  hipLaunchKernelGGL(capture_stats_partial_kernel, dim3(nb, n), dim3(kStatsThreads), 0, s, (const uint8_t*)blob, desc_dev, (int64_t*)ws);
  const int rc = dm4d_check_launch("capture_stats_partial_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(capture_stats_fold_kernel, dim3(n), dim3(64), 0, s, desc_dev, (const int64_t*)ws, nb, out);
  return dm4d_check_launch("capture_stats_fold_kernel");
}

extern "C" int dm4d_capture_fill_rects_u8(void* stream, void* blob, int64_t blob_bytes, const int64_t* desc_host, const int64_t* desc_dev, int n) {
  if (!blob || !desc_host || !desc_dev) return dm4d_set_error(DM4D_ERR_ARG, "capture_fill_rects: null pointer");
  if (n < 1 || n > 65535) return dm4d_set_error(DM4D_ERR_ARG, "capture_fill_rects: n outside 1..65535");
  if (blob_bytes < 1) return dm4d_set_error(DM4D_ERR_ARG, "capture_fill_rects: empty blob");
  if ((uintptr_t)desc_dev & 7) return dm4d_set_error(DM4D_ERR_ARG, "capture_fill_rects: desc_dev must be 8-byte aligned");
  int64_t max_bytes = 0;
  for (int p = 0; p < n; ++p) {
    const int64_t* d = desc_host + (int64_t)p * DM4D_CAPTURE_RECT_FIELDS;
    const int64_t off = d[R_OFF], h = d[R_H], w = d[R_W];
    if (h < 1 || w < 1 || h > kStatsMaxSide || w > kStatsMaxSide) return dm4d_set_error(DM4D_ERR_ARG, "capture_fill_rects: a plane's size is outside 1..32768");
    if (off < 0 || off > blob_bytes || h * w > blob_bytes - off) return dm4d_set_error(DM4D_ERR_ARG, "capture_fill_rects: a plane lies outside the blob");
    if (d[R_C0] < 0 || d[R_C0] > d[R_C1] || d[R_C1] > w || d[R_R0] < 0 || d[R_R0] > d[R_R1] || d[R_R1] > h)
      return dm4d_set_error(DM4D_ERR_ARG, "capture_fill_rects: a rectangle lies outside its plane");
    if (h * w > max_bytes) max_bytes = h * w;
  }
  hipLaunchKernelGGL(capture_fill_rects_kernel, dim3(stats_blocks(max_bytes), n), dim3(kStatsThreads), 0, (hipStream_t)stream, (uint8_t*)blob,
                     desc_dev);
  return dm4d_check_launch("capture_fill_rects_kernel");
}
