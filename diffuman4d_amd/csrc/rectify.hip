// Raw-capture rectification (diffuman4d_amd/host/rectify.py; the reference's scripts/download/extract_dnar_images.py calib_undist_image):
// colour correction through a 3 x 256 fp32 table, undistortion to a pinhole camera with bilinear taps, area resize and crop, for a batch of
// images of different sizes, cameras and tables, in ONE launch.  tests/rectify_model.py is the definition; this file is compiled with
// -ffp-contract=off and writes every fp32 operation in the model's order, so a result is the model's byte for byte.
//
// A workgroup owns one kTileW x kTileH tile of an image's cropped output.  The area windows of the tile's columns and rows name a patch of
// the undistorted image; the workgroup computes that patch as uint8 into LDS (a lane per patch pixel: four source gathers and twelve table
// lookups, neighbouring lanes on neighbouring source pixels), then a lane per output pixel runs the horizontal sums in fp32 and the vertical
// sum over them in registers, and the tile leaves through LDS in 16-byte stores where the row pitch allows.  The undistorted image never
// reaches memory.  A horizontal sum is recomputed by the (at most two) output rows whose windows share its patch row; it costs the same
// operations in the same order wherever it is made.  No atomics, no workgroup waits on another; a result depends on its own descriptor,
// tables and source only.
#include <stdint.h>
#include <stdio.h>

#include "common.h"
#include "dm4d.h"
#include "errors.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTileW = 32, kTileH = 8;         // output pixels of one workgroup: kThreads of them
constexpr int kLutBytes = 3 * 256 * 4;         // the image's table, in LDS
constexpr int kOutBytes = kTileH * kTileW * 3; // the tile before it is stored
constexpr int kMaxLds = 65536;
constexpr int kMaxTaps = 10;                   // a window of scale <= 8 overlaps at most 9 cells
constexpr int kCamFloats = 16;

// descriptor fields (int64 each, DM4D_RECTIFY_FIELDS per image), see dm4d.h
enum { F_SRC = 0, F_H, F_W, F_UH, F_UW, F_RH, F_RW, F_TOP, F_LEFT, F_CH, F_CW, F_HTAB, F_HK, F_VTAB, F_VK, F_CAM, F_OUT };
// camera constants (fp32 each, kCamFloats per image)
enum { C_FX = 0, C_FY, C_CX, C_CY, C_K1, C_K2, C_P1, C_P2, C_K3, C_CXU, C_CYU, C_IFXU, C_IFYU };

__host__ __device__ inline int patch_bytes(int pw, int ph) { return (pw * ph * 3 + 15) & ~15; }

__global__ void __launch_bounds__(kThreads) rectify_kernel(const uint8_t* __restrict__ stage, const int64_t* __restrict__ desc,
                                                           const int32_t* __restrict__ tab, const float* __restrict__ luts,
                                                           uint8_t* __restrict__ out, int patch_cap) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  float* lut = reinterpret_cast<float*>(lds);
  uint8_t* tile = lds + kLutBytes;
  uint8_t* patch = tile + kOutBytes;

  const int f = blockIdx.z, tid = threadIdx.x;
  const int64_t* d = desc + (int64_t)f * DM4D_RECTIFY_FIELDS;
  const int cw = (int)d[F_CW], ch = (int)d[F_CH];
  const int tx0 = blockIdx.x * kTileW, ty0 = blockIdx.y * kTileH;
  if (tx0 >= cw || ty0 >= ch) return;  // the grid is sized for the largest image of the batch
  const int tw = min(kTileW, cw - tx0), th = min(kTileH, ch - ty0);
  const int rw = (int)d[F_RW], rh = (int)d[F_RH], hk = (int)d[F_HK], vk = (int)d[F_VK];
  const int32_t* hwin = tab + d[F_HTAB];
  const int32_t* vwin = tab + d[F_VTAB];
  const float* hwt = reinterpret_cast<const float*>(hwin + 2 * rw);
  const float* vwt = reinterpret_cast<const float*>(vwin + 2 * rh);
  const int ox0 = (int)d[F_LEFT] + tx0, oy0 = (int)d[F_TOP] + ty0;
  // windows are validated to start and end in ascending order: the first one's start and the last one's end bound the patch
  const int px0 = hwin[2 * ox0], px1 = hwin[2 * (ox0 + tw - 1)] + hwin[2 * (ox0 + tw - 1) + 1];
  const int py0 = vwin[2 * oy0], py1 = vwin[2 * (oy0 + th - 1)] + vwin[2 * (oy0 + th - 1) + 1];
  const int pw = px1 - px0, ph = py1 - py0;
  if (patch_bytes(pw, ph) > patch_cap) return;  // never taken: the host sized patch_cap from these very windows

  const float* src_lut = luts + (int64_t)f * 768;
  for (int i = tid; i < 768; i += kThreads) lut[i] = src_lut[i];
  __syncthreads();

  // ---- the undistorted patch, uint8 RGB, into LDS
  {
    const float* cam = reinterpret_cast<const float*>(tab + d[F_CAM]);
    const float fx = cam[C_FX], fy = cam[C_FY], cx = cam[C_CX], cy = cam[C_CY];
    const float k1 = cam[C_K1], k2 = cam[C_K2], p1 = cam[C_P1], p2 = cam[C_P2], k3 = cam[C_K3];
    const float cxu = cam[C_CXU], cyu = cam[C_CYU], ifxu = cam[C_IFXU], ifyu = cam[C_IFYU];
    const int h = (int)d[F_H], w = (int)d[F_W];
    const float wm1 = (float)(w - 1), hm1 = (float)(h - 1);
    const uint8_t* src = stage + d[F_SRC];
    const int lane = tid & 63, wave = tid >> 6;
    for (int r = wave; r < ph; r += kThreads / 64) {
      const float v = (((float)(py0 + r) + 0.5f) - cyu) * ifyu;
      for (int c = lane; c < pw; c += 64) {
        const float u = (((float)(px0 + c) + 0.5f) - cxu) * ifxu;
        const float r2 = u * u + v * v;
        const float rad = 1.0f + r2 * (k1 + r2 * (k2 + r2 * k3));
        const float du = (u * rad + ((2.0f * p1) * u) * v) + p2 * (r2 + (2.0f * u) * u);
        const float dv = (v * rad + p1 * (r2 + (2.0f * v) * v)) + ((2.0f * p2) * u) * v;
        const float xs = (fx * du + cx) - 0.5f;
        const float ys = (fy * dv + cy) - 0.5f;
        uint32_t px[3] = {0, 0, 0};
        if (xs >= 0.0f && ys >= 0.0f && xs <= wm1 && ys <= hm1) {  // false for NaN too
          const float x0f = floorf(xs), y0f = floorf(ys);
          const float ax = xs - x0f, ay = ys - y0f;
          const float bx = 1.0f - ax, by = 1.0f - ay;
          const int x0 = (int)x0f, y0 = (int)y0f;
          const int x1 = min(x0 + 1, w - 1), y1 = min(y0 + 1, h - 1);
          const uint8_t* s00 = src + ((int64_t)y0 * w + x0) * 3;
          const uint8_t* s01 = src + ((int64_t)y0 * w + x1) * 3;
          const uint8_t* s10 = src + ((int64_t)y1 * w + x0) * 3;
          const uint8_t* s11 = src + ((int64_t)y1 * w + x1) * 3;
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const float* t = lut + 256 * k;
            const float val = (bx * t[s00[k]] + ax * t[s01[k]]) * by + (bx * t[s10[k]] + ax * t[s11[k]]) * ay;
            px[k] = (uint32_t)min((int)val, 255);
          }
        }
        uint8_t* p = patch + (r * pw + c) * 3;
        p[0] = (uint8_t)px[0], p[1] = (uint8_t)px[1], p[2] = (uint8_t)px[2];
      }
    }
  }
  __syncthreads();

  // ---- the area sums: a lane per output pixel of the tile
  {
    const int lx = tid % kTileW, ly = tid / kTileW;
    if (lx < tw && ly < th) {
      const int ox = ox0 + lx, oy = oy0 + ly;
      const int hs = hwin[2 * ox] - px0, hc = hwin[2 * ox + 1];
      const int vs = vwin[2 * oy] - py0, vc = vwin[2 * oy + 1];
      const float* hw_ = hwt + (int64_t)ox * hk;
      const float* vw_ = vwt + (int64_t)oy * vk;
      float acc[3] = {0.0f, 0.0f, 0.0f};
      for (int t = 0; t < vc; ++t) {
        const uint8_t* row = patch + ((vs + t) * pw + hs) * 3;
        float s[3] = {0.0f, 0.0f, 0.0f};
        for (int j = 0; j < hc; ++j) {
          const float wj = hw_[j];
#pragma unroll
          for (int k = 0; k < 3; ++k) s[k] = s[k] + wj * (float)row[3 * j + k];
        }
        const float wt = vw_[t];
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[k] = acc[k] + wt * s[k];
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) tile[(ly * kTileW + lx) * 3 + k] = (uint8_t)fminf(fmaxf(rintf(acc[k]), 0.0f), 255.0f);
    }
  }
  __syncthreads();

  // ---- the tile's rows to memory: 16 bytes a lane where every row of the image starts on a 16-byte boundary, bytes otherwise
  {
    uint8_t* dst = out + d[F_OUT] + ((int64_t)ty0 * cw + tx0) * 3;
    const int row_bytes = tw * 3;
    if ((cw & 15) == 0) {  // then cw * 3 and tx0 * 3 are multiples of 16, and so is tw * 3 (tw is 32, or cw % 32 = 16)
      constexpr int kVecs = kTileW * 3 / 16;
      const int r = tid / kVecs, q = tid % kVecs;
      if (r < th && q * 16 < row_bytes) stg16(dst + (int64_t)r * cw * 3 + q * 16, *reinterpret_cast<const U4*>(tile + r * kTileW * 3 + q * 16));
    } else {
      for (int i = tid; i < th * row_bytes; i += kThreads) {
        const int r = i / row_bytes, b = i % row_bytes;
        dst[(int64_t)r * cw * 3 + b] = tile[r * kTileW * 3 + b];
      }
    }
  }
}

// A table of `n_out` windows {start, length} then n_out x k fp32 weights at int32 offset `off` of the host table: inside the table,
// every window inside 0..n_in, of 1..k taps, starts and ends ascending.
bool table_ok(const int32_t* tab, int64_t tab_len, int64_t off, int64_t k, int64_t n_out, int64_t n_in) {
  if (off < 0 || k < 1 || k > kMaxTaps || off > tab_len || n_out * (2 + k) > tab_len - off) return false;
  const int32_t* win = tab + off;
  int64_t prev_s = 0, prev_e = 0;
  for (int64_t i = 0; i < n_out; ++i) {
    const int64_t s = win[2 * i], c = win[2 * i + 1];
    if (s < 0 || c < 1 || c > k || s + c > n_in || s < prev_s || s + c < prev_e) return false;
    prev_s = s, prev_e = s + c;
  }
  return true;
}

// the widest patch extent along one axis over the tiles [first, first + count) cut every `tile` outputs
int64_t max_extent(const int32_t* win, int64_t first, int64_t count, int tile) {
  int64_t best = 0;
  for (int64_t t0 = 0; t0 < count; t0 += tile) {
    const int64_t a = first + t0, b = first + (t0 + tile < count ? t0 + tile : count) - 1;
    const int64_t e = (int64_t)win[2 * b] + win[2 * b + 1] - win[2 * a];
    if (e > best) best = e;
  }
  return best;
}

}  // namespace

extern "C" int dm4d_rectify_u8(void* stream, const void* staging, int64_t staging_bytes, const int64_t* desc_host, const int64_t* desc_dev,
                               int n, const int32_t* tab_host, const int32_t* tab_dev, int64_t tab_len, const void* lut_dev, void* out,
                               int64_t out_bytes) {
  static thread_local char msg[192];
  if (!staging || !desc_host || !desc_dev || !tab_host || !tab_dev || !lut_dev || !out)
    return dm4d_set_error(DM4D_ERR_ARG, "rectify: null pointer");
  if (n < 1 || n > 65535) return dm4d_set_error(DM4D_ERR_ARG, "rectify: n outside 1..65535");
  if (staging_bytes < 1 || tab_len < 1 || out_bytes < 1) return dm4d_set_error(DM4D_ERR_ARG, "rectify: empty staging buffer, table or output");
  if ((((uintptr_t)staging | (uintptr_t)out | (uintptr_t)lut_dev) & 15) || ((uintptr_t)tab_dev & 3) || ((uintptr_t)desc_dev & 7))
    return dm4d_set_error(DM4D_ERR_ARG, "rectify: staging, out, lut_dev (16 bytes), tab_dev (4) and desc_dev (8) must be aligned");
  int64_t max_cw = 0, max_ch = 0;
  int cap = 0;
  for (int r = 0; r < n; ++r) {
    const int64_t* d = desc_host + (int64_t)r * DM4D_RECTIFY_FIELDS;
    const char* bad = nullptr;
    bool sizes = true;
    for (int k = F_H; k <= F_RW; ++k) sizes = sizes && d[k] >= 1 && d[k] <= DM4D_RECTIFY_MAX_SIDE;
    if (!sizes) {
      bad = "a source, undistorted or resized size is outside 1..16384";
    } else if (d[F_SRC] < 0 || (d[F_SRC] & 15) || d[F_OUT] < 0 || (d[F_OUT] & 15)) {
      bad = "a source or output offset is negative or not 16-byte aligned";
    } else if (d[F_SRC] > staging_bytes || d[F_H] * d[F_W] * 3 > staging_bytes - d[F_SRC]) {
      bad = "source outside the staging buffer";
    } else if (d[F_RW] > d[F_UW] || d[F_UW] > DM4D_RECTIFY_MAX_SCALE * d[F_RW] || d[F_RH] > d[F_UH] || d[F_UH] > DM4D_RECTIFY_MAX_SCALE * d[F_RH]) {
      bad = "the resize scale of an axis is outside 1..8";
    } else if (d[F_TOP] < 0 || d[F_LEFT] < 0 || d[F_CH] < 1 || d[F_CW] < 1 || d[F_CH] > d[F_RH] - d[F_TOP] || d[F_CW] > d[F_RW] - d[F_LEFT]) {
      bad = "the crop is empty or lies outside the resized image";
    } else if (d[F_OUT] > out_bytes || d[F_CH] * d[F_CW] * 3 > out_bytes - d[F_OUT]) {
      bad = "output outside the output buffer";
    } else if (!table_ok(tab_host, tab_len, d[F_HTAB], d[F_HK], d[F_RW], d[F_UW])) {
      bad = "the horizontal table is out of range or a tap window lies outside the undistorted image";
    } else if (!table_ok(tab_host, tab_len, d[F_VTAB], d[F_VK], d[F_RH], d[F_UH])) {
      bad = "the vertical table is out of range or a tap window lies outside the undistorted image";
    } else if (d[F_CAM] < 0 || d[F_CAM] > tab_len || kCamFloats > tab_len - d[F_CAM]) {
      bad = "the camera constants lie outside the table";
    } else {
      const int64_t pw = max_extent(tab_host + d[F_HTAB], d[F_LEFT], d[F_CW], kTileW);
      const int64_t ph = max_extent(tab_host + d[F_VTAB], d[F_TOP], d[F_CH], kTileH);
      if (pw * ph * 3 + 15 > kMaxLds - kLutBytes - kOutBytes) {
        bad = "a tile's undistorted patch does not fit in LDS";
      } else {
        const int need = patch_bytes((int)pw, (int)ph);
        if (need > cap) cap = need;
        if (d[F_CW] > max_cw) max_cw = d[F_CW];
        if (d[F_CH] > max_ch) max_ch = d[F_CH];
      }
    }
    if (bad) {
      snprintf(msg, sizeof msg, "rectify: image %d: %s", r, bad);
      return dm4d_set_error(DM4D_ERR_ARG, msg);
    }
  }
  const dim3 grid((unsigned)((max_cw + kTileW - 1) / kTileW), (unsigned)((max_ch + kTileH - 1) / kTileH), (unsigned)n);
  hipLaunchKernelGGL(rectify_kernel, grid, dim3(kThreads), (size_t)(kLutBytes + kOutBytes + cap), (hipStream_t)stream, (const uint8_t*)staging,
                     desc_dev, tab_dev, (const float*)lut_dev, (uint8_t*)out, cap);
  return dm4d_check_launch("rectify_kernel");
}
