// Foreground-mask prediction around a caller-named matting network (diffuman4d_amd/host/matting.py; the reference's remove_background
// stage: scripts/preprocess/remove_background.py transform_image / extract_object / inference_batch).  The network is the caller's;
// the two entries here are the arithmetic on either side of it.
//
//   dm4d_matting_input_u8      rotation (an index map), Pillow's two-pass bilinear resize to the network's size, and the normalisation
//                              as a 3 x 256 table of the output type: at most two launches for a batch of images of different sizes
//   dm4d_matting_mask_f16_u8   fp16 logit -> byte through a 65536-entry table (no exp here), Pillow's two-pass bicubic resize to each
//                              image's size, the rotation back, into one packed blob: at most two launches
//
// Pillow's separable filter by the rule of image_common.h: a horizontal pass whose result is rounded to uint8 (kept in scratch), then a
// vertical pass over it; an axis whose size does not change is not filtered.  Integer arithmetic apart from the table lookups, no
// atomics, no workgroup waits on another; a lane owns consecutive output columns of one row and stores 16 bytes where alignment allows.
#include <stdint.h>
#include <stdio.h>

#include "common.h"
#include "dm4d.h"
#include "errors.h"
#include "image_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kInCols = 4;     // output columns per lane of the input's horizontal pass: 16 bytes of packed scratch words
constexpr int kMaskCols = 16;  // output columns per lane of both mask passes: 16 bytes

// descriptor fields (int64 each, DM4D_MATTING_FIELDS per image), see dm4d.h
enum { F_PLANE = 0, F_H, F_W, F_HTAB, F_HK, F_VTAB, F_VK, F_SCRATCH };

// Image.rotate(-90 rot, expand=True) without a copy: pixel (y, x) of the rotated image is pixel base + y * sy + x * sx of the stored one
struct RotMap {
  int64_t base, sy, sx;
};

__host__ __device__ inline RotMap rot_map(int h, int w, int rot) {
  switch (rot) {
    case 1: return RotMap{(int64_t)(h - 1) * w, 1, -(int64_t)w};
    case 2: return RotMap{(int64_t)(h - 1) * w + (w - 1), -(int64_t)w, -1};
    case 3: return RotMap{(int64_t)w - 1, -1, (int64_t)w};
    default: return RotMap{0, (int64_t)w, 1};
  }
}

__device__ __forceinline__ uint32_t pack_rgb(const uint32_t (&c)[3]) { return c[0] | (c[1] << 8) | (c[2] << 16); }

// ------------------------------------------------------------------------------------------------------------------- network input
// Horizontal pass, grid (lanes over S_w / 4, rows of the tallest rotated image, n): one lane = 4 consecutive columns of one scratch row
__global__ void __launch_bounds__(kThreads) matting_in_hpass_kernel(const uint8_t* __restrict__ stage, const int64_t* __restrict__ desc,
                                                                    const int32_t* __restrict__ tab, uint8_t* __restrict__ scratch, int S_w,
                                                                    int rot) {
  const int64_t* d = desc + (int64_t)blockIdx.z * DM4D_MATTING_FIELDS;
  if (d[F_HTAB] < 0) return;
  const int h = (int)d[F_H], w = (int)d[F_W], rh = (rot & 1) ? w : h;
  const int r = blockIdx.y, x0 = (blockIdx.x * kThreads + threadIdx.x) * kInCols;
  if (r >= rh || x0 >= S_w) return;
  const int ksize = (int)d[F_HK];
  const int32_t* bounds = tab + d[F_HTAB];
  const int32_t* coefs = bounds + 2 * S_w;
  const RotMap m = rot_map(h, w, rot);
  const uint8_t* line = stage + d[F_PLANE] + 3 * (m.base + r * m.sy);
  uint32_t px[kInCols];
#pragma unroll
  for (int j = 0; j < kInCols; ++j) {
    const int ox = x0 + j;
    px[j] = 0;
    if (ox < S_w) {
      const int xmin = bounds[2 * ox], cnt = bounds[2 * ox + 1];
      uint32_t c[3];
      pillow_rgb(ByteRgb{line + 3 * (xmin * m.sx), 3 * m.sx}, coefs + (int64_t)ox * ksize, cnt, c);
      px[j] = pack_rgb(c);
    }
  }
  uint32_t* dst = reinterpret_cast<uint32_t*>(scratch + d[F_SCRATCH]) + (int64_t)r * S_w + x0;
  if ((S_w & 3) == 0) {
    stg16(dst, U4{px[0], px[1], px[2], px[3]});
  } else {
#pragma unroll
    for (int j = 0; j < kInCols; ++j)
      if (x0 + j < S_w) dst[j] = px[j];
  }
}

// Vertical pass + normalisation, grid (lanes over S_w / COLS, S_h, n): one lane = COLS consecutive columns of one output row, 16 bytes of
// each of the three planes.  The source is the scratch, or the image itself where the horizontal pass is skipped.
template <typename T>
__global__ void __launch_bounds__(kThreads) matting_in_vpass_kernel(const uint8_t* __restrict__ stage, const int64_t* __restrict__ desc,
                                                                    const int32_t* __restrict__ tab, const uint8_t* __restrict__ scratch,
                                                                    const T* __restrict__ lut, T* __restrict__ out, int S_h, int S_w, int rot) {
  constexpr int COLS = 16 / (int)sizeof(T);
  const int f = blockIdx.z, oy = blockIdx.y, x0 = (blockIdx.x * kThreads + threadIdx.x) * COLS;
  if (x0 >= S_w) return;
  const int64_t* d = desc + (int64_t)f * DM4D_MATTING_FIELDS;
  const int h = (int)d[F_H], w = (int)d[F_W];
  const bool has_h = d[F_HTAB] >= 0, has_v = d[F_VTAB] >= 0;
  int ymin = oy, cnt = 1;
  const int32_t* k = nullptr;
  if (has_v) {
    const int32_t* bounds = tab + d[F_VTAB];
    ymin = bounds[2 * oy], cnt = bounds[2 * oy + 1];
    k = bounds + 2 * S_h + (int64_t)oy * (int)d[F_VK];
  }
  const uint32_t* scr = reinterpret_cast<const uint32_t*>(scratch + d[F_SCRATCH]) + (int64_t)ymin * S_w + x0;
  const bool vec = (S_w % COLS) == 0;  // then every lane's columns are inside the row and its stores are 16-byte aligned
  uint32_t px[COLS];
  if (has_h && has_v && vec) {  // the usual case: 16-byte loads of the scratch rows of the window
    int32_t acc[COLS][3];
#pragma unroll
    for (int j = 0; j < COLS; ++j) acc[j][0] = acc[j][1] = acc[j][2] = kPillowHalf;
    for (int t = 0; t < cnt; ++t) {
      const U4* row = reinterpret_cast<const U4*>(scr + (int64_t)t * S_w);
      const int32_t wt = k[t];
#pragma unroll
      for (int q = 0; q < COLS / 4; ++q) {
        const U4 v = row[q];
        const uint32_t p[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          acc[4 * q + j][0] += (int32_t)(p[j] & 0xffu) * wt;
          acc[4 * q + j][1] += (int32_t)((p[j] >> 8) & 0xffu) * wt;
          acc[4 * q + j][2] += (int32_t)((p[j] >> 16) & 0xffu) * wt;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < COLS; ++j) px[j] = clip8(acc[j][0]) | (clip8(acc[j][1]) << 8) | (clip8(acc[j][2]) << 16);
  } else {
    const RotMap m = rot_map(h, w, rot);
    const uint8_t* img = stage + d[F_PLANE] + 3 * (m.base + ymin * m.sy);
#pragma unroll
    for (int j = 0; j < COLS; ++j) {
      px[j] = 0;
      if (x0 + j >= S_w) continue;
      uint32_t c[3];
      if (has_h) {
        const PackedRgb src{scr + j, S_w};
        if (has_v) pillow_rgb(src, k, cnt, c); else src(0, c);
      } else {
        const ByteRgb src{img + 3 * ((x0 + j) * m.sx), 3 * m.sy};
        if (has_v) pillow_rgb(src, k, cnt, c); else src(0, c);
      }
      px[j] = pack_rgb(c);
    }
  }
  const int64_t plane = (int64_t)S_h * S_w;
  T* o = out + (int64_t)f * 3 * plane + (int64_t)oy * S_w + x0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    T v[COLS];
#pragma unroll
    for (int j = 0; j < COLS; ++j) v[j] = lut[c * 256 + ((px[j] >> (8 * c)) & 0xffu)];
    if (vec) {
      U4 q;
      __builtin_memcpy(&q, v, 16);
      stg16(o + c * plane, q);
    } else {
#pragma unroll
      for (int j = 0; j < COLS; ++j)
        if (x0 + j < S_w) o[c * plane + j] = v[j];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------- mask
// Horizontal pass with the quantiser in it, grid (lanes over the widest rw / 16, S_h, n): one lane = 16 consecutive columns of one
// scratch row; a tap is qtab[bit pattern of the logit], so the S_h x S_w byte plane exists in registers only
__global__ void __launch_bounds__(kThreads) matting_mask_hpass_kernel(const uint16_t* __restrict__ logits, const int64_t* __restrict__ desc,
                                                                      const int32_t* __restrict__ tab, const uint8_t* __restrict__ qtab,
                                                                      uint8_t* __restrict__ scratch, int S_h, int S_w, int rot) {
  const int64_t* d = desc + (int64_t)blockIdx.z * DM4D_MATTING_FIELDS;
  if (d[F_HTAB] < 0) return;
  const int rw = (rot & 1) ? (int)d[F_H] : (int)d[F_W];
  const int r = blockIdx.y, x0 = (blockIdx.x * kThreads + threadIdx.x) * kMaskCols;
  if (x0 >= rw) return;
  const int ksize = (int)d[F_HK];
  const int32_t* bounds = tab + d[F_HTAB];
  const int32_t* coefs = bounds + 2 * rw;
  const uint16_t* line = logits + ((int64_t)blockIdx.z * S_h + r) * S_w;
  uint32_t o[kMaskCols];
#pragma unroll
  for (int j = 0; j < kMaskCols; ++j) {
    const int ox = x0 + j;
    o[j] = 0;
    if (ox < rw) {
      const int xmin = bounds[2 * ox], cnt = bounds[2 * ox + 1];
      const int32_t* k = coefs + (int64_t)ox * ksize;
      int32_t acc = kPillowHalf;
      for (int t = 0; t < cnt; ++t) acc += (int32_t)qtab[line[xmin + t]] * k[t];
      o[j] = clip8(acc);
    }
  }
  uint8_t* dst = scratch + d[F_SCRATCH] + (int64_t)r * rw + x0;
  if ((rw % kMaskCols) == 0) {
    uint32_t q[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = o[4 * i] | (o[4 * i + 1] << 8) | (o[4 * i + 2] << 16) | (o[4 * i + 3] << 24);
    stg16(dst, U4{q[0], q[1], q[2], q[3]});
  } else {
#pragma unroll
    for (int j = 0; j < kMaskCols; ++j)
      if (x0 + j < rw) dst[j] = (uint8_t)o[j];
  }
}

// Vertical pass + the rotation back, grid (lanes over the widest rw / 16, rows of the tallest rotated mask, n): one lane = 16 consecutive
// columns of one row of the rotated mask.  The source is the scratch, or the quantised logits where the horizontal pass is skipped.
__global__ void __launch_bounds__(kThreads) matting_mask_vpass_kernel(const uint16_t* __restrict__ logits, const int64_t* __restrict__ desc,
                                                                      const int32_t* __restrict__ tab, const uint8_t* __restrict__ qtab,
                                                                      const uint8_t* __restrict__ scratch, uint8_t* __restrict__ blob, int S_h,
                                                                      int S_w, int rot) {
  const int f = blockIdx.z;
  const int64_t* d = desc + (int64_t)f * DM4D_MATTING_FIELDS;
  const int h = (int)d[F_H], w = (int)d[F_W], rh = (rot & 1) ? w : h, rw = (rot & 1) ? h : w;
  const int oy = blockIdx.y, x0 = (blockIdx.x * kThreads + threadIdx.x) * kMaskCols;
  if (oy >= rh || x0 >= rw) return;
  const bool has_h = d[F_HTAB] >= 0, has_v = d[F_VTAB] >= 0;
  int ymin = oy, cnt = 1;
  const int32_t* k = nullptr;
  if (has_v) {
    const int32_t* bounds = tab + d[F_VTAB];
    ymin = bounds[2 * oy], cnt = bounds[2 * oy + 1];
    k = bounds + 2 * rh + (int64_t)oy * (int)d[F_VK];
  }
  const uint8_t* scr = scratch + d[F_SCRATCH] + (int64_t)ymin * rw + x0;
  const bool vec = (rw % kMaskCols) == 0;  // then every lane's columns are inside the row and scratch loads are 16-byte aligned
  uint32_t o[kMaskCols];
  if (has_h && has_v && vec) {  // the usual case: one 16-byte load per scratch row of the window
    int32_t acc[kMaskCols];
#pragma unroll
    for (int j = 0; j < kMaskCols; ++j) acc[j] = kPillowHalf;
    for (int t = 0; t < cnt; ++t) {
      const U4 v = ldg16(scr + (int64_t)t * rw);
      const uint32_t p[4] = {v.x, v.y, v.z, v.w};
      const int32_t wt = k[t];
#pragma unroll
      for (int j = 0; j < kMaskCols; ++j) acc[j] += (int32_t)((p[j >> 2] >> (8 * (j & 3))) & 0xffu) * wt;
    }
#pragma unroll
    for (int j = 0; j < kMaskCols; ++j) o[j] = clip8(acc[j]);
  } else {
    const uint16_t* lg = logits + ((int64_t)f * S_h + ymin) * S_w + x0;  // read where !has_h only: then rw == S_w
#pragma unroll
    for (int j = 0; j < kMaskCols; ++j) {
      o[j] = 0;
      if (x0 + j >= rw) continue;
      if (has_v) {
        int32_t acc = kPillowHalf;
        for (int t = 0; t < cnt; ++t)
          acc += (int32_t)(has_h ? scr[(int64_t)t * rw + j] : qtab[lg[(int64_t)t * S_w + j]]) * k[t];
        o[j] = clip8(acc);
      } else {
        o[j] = has_h ? scr[j] : qtab[lg[j]];
      }
    }
  }
  const RotMap m = rot_map(h, w, rot);
  uint8_t* dst = blob + d[F_PLANE] + m.base + oy * m.sy + x0 * m.sx;
  if (rot == 0 && vec) {  // w == rw is a multiple of 16 and the plane is 16-byte aligned
    uint32_t q[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = o[4 * i] | (o[4 * i + 1] << 8) | (o[4 * i + 2] << 16) | (o[4 * i + 3] << 24);
    stg16(dst, U4{q[0], q[1], q[2], q[3]});
  } else {
#pragma unroll
    for (int j = 0; j < kMaskCols; ++j)
      if (x0 + j < rw) dst[j * m.sx] = (uint8_t)o[j];
  }
}

// ---------------------------------------------------------------------------------------------------------------------- validation
// Every descriptor against the host copy of the tables.  input: planes of 3 bytes per pixel anywhere in `plane_bytes`, tables rw -> S_w
// and rh -> S_h, scratch rh x S_w x 4 bytes; else: planes of 1 byte per pixel at 16-byte aligned offsets, tables S_w -> rw and S_h -> rh,
// scratch S_h x rw bytes.  -> the tallest and widest rotated image and whether any image has a horizontal pass.
int check_rows(const char* what, bool input, const int64_t* desc_host, int n, const int32_t* tab_host, int64_t tab_len, int64_t plane_bytes,
               int64_t scratch_bytes, int S_h, int S_w, int rot, int* max_rh, int* max_rw, bool* any_h) {
  static thread_local char msg[192];
  *max_rh = 0, *max_rw = 0, *any_h = false;
  for (int r = 0; r < n; ++r) {
    const int64_t* d = desc_host + (int64_t)r * DM4D_MATTING_FIELDS;
    const int64_t h = d[F_H], w = d[F_W];
    const char* bad = nullptr;
    if (h < 1 || h > DM4D_MATTING_MAX_SIDE || w < 1 || w > DM4D_MATTING_MAX_SIDE) {
      bad = "image size outside 1..16384";
    } else {
      const int64_t rh = (rot & 1) ? w : h, rw = (rot & 1) ? h : w, bytes = h * w * (input ? 3 : 1);
      const int64_t h_out = input ? S_w : rw, h_in = input ? rw : S_w, v_out = input ? S_h : rh, v_in = input ? rh : S_h;
      const int64_t need = input ? rh * S_w * 4 : S_h * rw;
      if (d[F_PLANE] < 0 || d[F_PLANE] > plane_bytes || bytes > plane_bytes - d[F_PLANE])
        bad = input ? "image outside the staging buffer" : "mask outside the blob";
      else if (!input && (d[F_PLANE] & 15))
        bad = "mask offset is not 16-byte aligned";
      else if ((h_in == h_out) != (d[F_HTAB] < 0) || (v_in == v_out) != (d[F_VTAB] < 0))
        bad = "an axis that changes its size needs a table, one that keeps it none (-1)";
      else if (d[F_HTAB] >= 0 && !pillow_table_ok(tab_host, tab_len, d[F_HTAB], d[F_HK], 1 << 16, h_out, h_in, false))
        bad = "the horizontal table is out of range or a window leaves its axis";
      else if (d[F_VTAB] >= 0 && !pillow_table_ok(tab_host, tab_len, d[F_VTAB], d[F_VK], 1 << 16, v_out, v_in, false))
        bad = "the vertical table is out of range or a window leaves its axis";
      else if (d[F_HTAB] >= 0 && (d[F_SCRATCH] < 0 || (d[F_SCRATCH] & 15) || d[F_SCRATCH] > scratch_bytes || need > scratch_bytes - d[F_SCRATCH]))
        bad = "scratch region out of range or not 16-byte aligned";
      if (!bad) {
        if (rh > *max_rh) *max_rh = (int)rh;
        if (rw > *max_rw) *max_rw = (int)rw;
        if (d[F_HTAB] >= 0) *any_h = true;
      }
    }
    if (bad) {
      snprintf(msg, sizeof msg, "%s: image %d: %s", what, r, bad);
      return dm4d_set_error(DM4D_ERR_ARG, msg);
    }
  }
  return 0;
}

inline unsigned lanes_to_blocks(int columns, int per_lane) {
  const int lanes = (columns + per_lane - 1) / per_lane;
  return (unsigned)((lanes + kThreads - 1) / kThreads);
}

}  // namespace

extern "C" int dm4d_matting_input_u8(void* stream, const void* staging, int64_t staging_bytes, const int64_t* desc_host,
                                     const int64_t* desc_dev, int n, const int32_t* tab_host, const int32_t* tab_dev, int64_t tab_len,
                                     const void* lut_dev, void* scratch, int64_t scratch_bytes, void* out, int S_h, int S_w, int rot,
                                     int out_f32) {
  if (!staging || !desc_host || !desc_dev || !tab_host || !tab_dev || !lut_dev || !scratch || !out)
    return dm4d_set_error(DM4D_ERR_ARG, "matting_input: null pointer");
  if (n < 1 || n > 65535) return dm4d_set_error(DM4D_ERR_ARG, "matting_input: n outside 1..65535");
  if (S_h < 1 || S_w < 1 || S_h > DM4D_MATTING_MAX_SIDE || S_w > DM4D_MATTING_MAX_SIDE)
    return dm4d_set_error(DM4D_ERR_ARG, "matting_input: network input size outside 1..16384");
  if (rot < 0 || rot > 3) return dm4d_set_error(DM4D_ERR_ARG, "matting_input: rot outside 0..3 (quarter turns)");
  if (staging_bytes < 1 || tab_len < 1 || scratch_bytes < 1) return dm4d_set_error(DM4D_ERR_ARG, "matting_input: empty staging buffer, table or scratch");
  if ((((uintptr_t)out | (uintptr_t)scratch | (uintptr_t)lut_dev) & 15) || ((uintptr_t)tab_dev & 3) || ((uintptr_t)desc_dev & 7))
    return dm4d_set_error(DM4D_ERR_ARG, "matting_input: out, scratch, lut_dev (16 bytes), tab_dev (4) and desc_dev (8) must be aligned");
  int max_rh, max_rw;
  bool any_h;
  const int rc = check_rows("matting_input", true, desc_host, n, tab_host, tab_len, staging_bytes, scratch_bytes, S_h, S_w, rot, &max_rh, &max_rw, &any_h);
  if (rc) return rc;
  const dim3 block(kThreads);
  if (any_h) {
    hipLaunchKernelGGL(matting_in_hpass_kernel, dim3(lanes_to_blocks(S_w, kInCols), max_rh, n), block, 0, (hipStream_t)stream,
                       (const uint8_t*)staging, desc_dev, tab_dev, (uint8_t*)scratch, S_w, rot);
    const int rc2 = dm4d_check_launch("matting_in_hpass_kernel");
    if (rc2) return rc2;
  }
  if (out_f32)
    hipLaunchKernelGGL(matting_in_vpass_kernel<float>, dim3(lanes_to_blocks(S_w, 4), S_h, n), block, 0, (hipStream_t)stream,
                       (const uint8_t*)staging, desc_dev, tab_dev, (const uint8_t*)scratch, (const float*)lut_dev, (float*)out, S_h, S_w, rot);
  else
    hipLaunchKernelGGL(matting_in_vpass_kernel<_Float16>, dim3(lanes_to_blocks(S_w, 8), S_h, n), block, 0, (hipStream_t)stream,
                       (const uint8_t*)staging, desc_dev, tab_dev, (const uint8_t*)scratch, (const _Float16*)lut_dev, (_Float16*)out, S_h, S_w,
                       rot);
  return dm4d_check_launch("matting_in_vpass_kernel");
}

extern "C" int dm4d_matting_mask_f16_u8(void* stream, const void* logits, const int64_t* desc_host, const int64_t* desc_dev, int n,
                                        const int32_t* tab_host, const int32_t* tab_dev, int64_t tab_len, const void* qtab_dev, void* scratch,
                                        int64_t scratch_bytes, void* blob, int64_t blob_bytes, int S_h, int S_w, int rot) {
  if (!logits || !desc_host || !desc_dev || !tab_host || !tab_dev || !qtab_dev || !scratch || !blob)
    return dm4d_set_error(DM4D_ERR_ARG, "matting_mask: null pointer");
  if (n < 1 || n > 65535) return dm4d_set_error(DM4D_ERR_ARG, "matting_mask: n outside 1..65535");
  if (S_h < 1 || S_w < 1 || S_h > DM4D_MATTING_MAX_SIDE || S_w > DM4D_MATTING_MAX_SIDE)
    return dm4d_set_error(DM4D_ERR_ARG, "matting_mask: network output size outside 1..16384");
  if (rot < 0 || rot > 3) return dm4d_set_error(DM4D_ERR_ARG, "matting_mask: rot outside 0..3 (quarter turns)");
  if (blob_bytes < 1 || tab_len < 1 || scratch_bytes < 1) return dm4d_set_error(DM4D_ERR_ARG, "matting_mask: empty blob, table or scratch");
  if ((((uintptr_t)blob | (uintptr_t)scratch) & 15) || ((uintptr_t)logits & 1) || ((uintptr_t)tab_dev & 3) || ((uintptr_t)desc_dev & 7))
    return dm4d_set_error(DM4D_ERR_ARG, "matting_mask: blob, scratch (16 bytes), logits (2), tab_dev (4) and desc_dev (8) must be aligned");
  int max_rh, max_rw;
  bool any_h;
  const int rc = check_rows("matting_mask", false, desc_host, n, tab_host, tab_len, blob_bytes, scratch_bytes, S_h, S_w, rot, &max_rh, &max_rw, &any_h);
  if (rc) return rc;
  const dim3 block(kThreads);
  const unsigned gx = lanes_to_blocks(max_rw, kMaskCols);
  if (any_h) {
    hipLaunchKernelGGL(matting_mask_hpass_kernel, dim3(gx, S_h, n), block, 0, (hipStream_t)stream, (const uint16_t*)logits, desc_dev, tab_dev,
                       (const uint8_t*)qtab_dev, (uint8_t*)scratch, S_h, S_w, rot);
    const int rc2 = dm4d_check_launch("matting_mask_hpass_kernel");
    if (rc2) return rc2;
  }
  hipLaunchKernelGGL(matting_mask_vpass_kernel, dim3(gx, max_rh, n), block, 0, (hipStream_t)stream, (const uint16_t*)logits, desc_dev, tab_dev,
                     (const uint8_t*)qtab_dev, (const uint8_t*)scratch, (uint8_t*)blob, S_h, S_w, rot);
  return dm4d_check_launch("matting_mask_vpass_kernel");
}
