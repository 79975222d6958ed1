// Result evaluation (the reference's ImageEvaluator, data/utils/metric_utils.py:98-137): for each of N (predicted, ground-truth) image
// pairs -- composite over the background through the foreground masks, nearest-neighbour resize to the canvas, the padded bounding
// box of the resized masks, crop, PSNR and SSIM (torchmetrics' defaults: 11 x 11 Gaussian window, sigma 1.5, data range 1).
//
// Three launches for a whole batch, every pair described by DM4D_EVAL_FIELDS int64 values (so pairs of different sizes and crops,
// which the reference evaluates one by one, share the launches):
//   eval_bbox_kernel     the bounding box of the masks' non-zero pixels in the resized index space (integer atomics);
//   eval_tile_kernel     one workgroup = one 32 x 16 tile of the crop with its 5-pixel halo: gather (crop offset + nearest index) and
//                        composite into LDS, the separable Gaussian of p, t, p^2, t^2, p t, the SSIM map value and the squared error of
//                        every pixel, summed over the tile in a fixed tree order -> one partial record per tile;
//   eval_reduce_kernel   one workgroup per pair: the pair's own tile records summed in a fixed order -> PSNR, SSIM, value ranges.
// No floating-point atomics: a pair's result is the same bits on every run and does not depend on the rest of the batch (tiles are
// laid out from the crop's own corner; the sums of a pair visit only that pair's tiles, in tile order).
//
// Arithmetic.  The composite is the reference's fp32 expression, each operation rounded on its own (this translation unit is compiled
// with -ffp-contract=off, as capture.hip): image * m + (1 - m) * bg.  Everything behind it -- window sums, the SSIM map, all means -- is
// fp64: with a flat background E[p^2] - mu^2 cancels, and the fp32 form of that difference carries an error near 1e-5 in the mean SSIM
// (torchmetrics' own uncertainty).  The SSIM map is defined where the window fits (torchmetrics reflect-pads by 5 and then drops a
// 5-pixel border: no padded value reaches the mean), so the kernel pads nothing and averages over the interior (h - 10) x (w - 10).
#include <math.h>
#include <stdint.h>

#include "dm4d.h"
#include "errors.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTileW = 32, kTileH = 16, kHalo = 5, kTaps = 2 * kHalo + 1;
constexpr int kInW = kTileW + 2 * kHalo, kInH = kTileH + 2 * kHalo;  // 42 x 26 pixels read per tile
constexpr int kPart = 6;                                           // doubles per tile record: sse, ssim sum, pred min/max, gt min/max
constexpr int kEmpty = 0x7f7f7f7f;                                 // raw box words after the byte fill: nothing found yet
constexpr int kBoxRows = 8;                                        // rows per lane of the bounding-box kernel
constexpr int kPadding = 8;                                        // mask_to_bbox(padding=8)

// descriptor fields (int64 each, DM4D_EVAL_FIELDS per pair), see dm4d.h
enum { F_PRED = 0, F_GT, F_PMASK, F_GMASK, F_SRC_H, F_SRC_W, F_OUT_H, F_OUT_W, F_FLAGS, F_LEFT, F_TOP, F_RIGHT, F_BOTTOM };

struct Weights { double w[kTaps]; };

// F.interpolate(mode="nearest") index: scale = (float)in / out, src = min((int)floorf(dst * scale), in - 1)
__device__ __forceinline__ int nearest(int dst, float scale, int in) {
  const int s = (int)floorf((float)dst * scale);
  return s < in - 1 ? s : in - 1;
}

__device__ __forceinline__ float load_mask(const uint8_t* blob, int64_t off, bool f32, int64_t idx) {
  if (f32) return reinterpret_cast<const float*>(blob + off)[idx];
  return __fdiv_rn((float)blob[off + idx], 255.0f);  // TF.to_tensor
}

__device__ __forceinline__ float load_pixel(const uint8_t* blob, int64_t off, bool f32, int64_t plane, int64_t idx, int c) {
  if (f32) return reinterpret_cast<const float*>(blob + off)[c * plane + idx];  // CHW fp32
  return __fdiv_rn((float)blob[off + idx * 3 + c], 255.0f);                    // HWC uint8
}

// apply_fmask(image, fmask, background_color): 0 black, 1 white, 2 grey
__device__ __forceinline__ float composite(float x, float m, int bg) {
  if (bg == 0) return x * m;
  if (bg == 1) return x * m + (1.0f - m);
  return x * m + (1.0f - m) * 0.5f;
}

// ---- (a) bounding box of the non-zero mask pixels, resized index space ------------------------------------------------------------
// raw[4 n] int32, byte-filled with 0x7f before the launch: {min x, min y, min -(x + 1), min -(y + 1)}.
__global__ void __launch_bounds__(kThreads) eval_bbox_kernel(const uint8_t* __restrict__ blob, const int64_t* __restrict__ desc,
                                                             int* __restrict__ raw) {
  const int64_t* d = desc + (int64_t)blockIdx.z * DM4D_EVAL_FIELDS;
  const int flags = (int)d[F_FLAGS];
  if (!(flags & DM4D_EVAL_CROP_MASKS)) return;
  const int oh = (int)d[F_OUT_H], ow = (int)d[F_OUT_W], sh = (int)d[F_SRC_H], sw = (int)d[F_SRC_W];
  const int y0 = blockIdx.y * kBoxRows;
  if (y0 >= oh || (int)(blockIdx.x * kThreads) >= ow) return;  // uniform over the workgroup
  __shared__ int box[4];
  if (threadIdx.x < 4) box[threadIdx.x] = kEmpty;
  __syncthreads();
  const int x = blockIdx.x * kThreads + threadIdx.x;
  if (x < ow) {
    const float sx_scale = (float)sw / (float)ow, sy_scale = (float)sh / (float)oh;
    const int sx = nearest(x, sx_scale, sw);
    const bool mf32 = flags & DM4D_EVAL_MASK_F32;
    int ymin = kEmpty, ymax = -1;
    for (int j = 0; j < kBoxRows && y0 + j < oh; ++j) {
      const int64_t idx = (int64_t)nearest(y0 + j, sy_scale, sh) * sw + sx;
      bool nz = false;
      if (d[F_PMASK] >= 0) nz = nz || (mf32 ? reinterpret_cast<const float*>(blob + d[F_PMASK])[idx] != 0.0f : blob[d[F_PMASK] + idx] != 0);
      if (d[F_GMASK] >= 0) nz = nz || (mf32 ? reinterpret_cast<const float*>(blob + d[F_GMASK])[idx] != 0.0f : blob[d[F_GMASK] + idx] != 0);
      if (nz) {
        if (ymin == kEmpty) ymin = y0 + j;
        ymax = y0 + j;
      }
    }
    if (ymax >= 0) {
      atomicMin(&box[0], x);
      atomicMin(&box[1], ymin);
      atomicMin(&box[2], -(x + 1));
      atomicMin(&box[3], -(ymax + 1));
    }
  }
  __syncthreads();
  if (threadIdx.x < 4 && box[threadIdx.x] != kEmpty) atomicMin(&raw[4 * blockIdx.z + threadIdx.x], box[threadIdx.x]);
}

// The crop of a pair: mask_to_bbox(padding=8) of the raw box (left, top, right, bottom; right / bottom exclusive; an empty mask
// gives the empty box), or the descriptor's own box, which the C entry has checked.  Always inside [0, ow] x [0, oh].
__device__ __forceinline__ void crop_box(const int64_t* d, const int* raw, int& l, int& t, int& r, int& b) {
  const int oh = (int)d[F_OUT_H], ow = (int)d[F_OUT_W];
  if ((int)d[F_FLAGS] & DM4D_EVAL_CROP_MASKS) {
    if (raw[0] == kEmpty) {
      l = t = r = b = 0;
      return;
    }
    l = max(min(raw[0], ow - 1) - kPadding, 0);
    t = max(min(raw[1], oh - 1) - kPadding, 0);
    r = min(max(-raw[2], l + 1) + kPadding, ow);
    b = min(max(-raw[3], t + 1) + kPadding, oh);
  } else {
    l = (int)d[F_LEFT], t = (int)d[F_TOP], r = (int)d[F_RIGHT], b = (int)d[F_BOTTOM];
  }
}

// fixed-order tree sums / extrema over the workgroup; `red` holds kThreads doubles
__device__ __forceinline__ double block_sum(double v, double* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

__device__ __forceinline__ double block_min(double v, double* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = fmin(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  return red[0];
}

// ---- (b) composite + gather + separable Gaussian + SSIM map + squared error, one tile per workgroup ----------------------------
__global__ void __launch_bounds__(kThreads) eval_tile_kernel(const uint8_t* __restrict__ blob, const int64_t* __restrict__ desc,
                                                             const int* __restrict__ raw, double* __restrict__ partials,
                                                             int tiles_per_item, float* __restrict__ debug, int dbg_h, int dbg_w,
                                                             Weights wt) {
  __shared__ float sp[3][kInH * kInW], st[3][kInH * kInW];  // composited pred / gt, 3 channels, tile + halo
  __shared__ double hb[5][kInH * kTileW];                   // horizontal window sums of p, t, pp, tt, pt (one channel at a time)
  const int n = blockIdx.z;
  const int64_t* d = desc + (int64_t)n * DM4D_EVAL_FIELDS;
  int l, t, r, b;
  crop_box(d, raw + 4 * n, l, t, r, b);
  const int cw = r - l, ch = b - t;
  const int ntx = (cw + kTileW - 1) / kTileW, nty = (ch + kTileH - 1) / kTileH;
  if ((int)blockIdx.x >= ntx || (int)blockIdx.y >= nty) return;  // uniform over the workgroup; also every tile of an empty box
  const int flags = (int)d[F_FLAGS];
  const bool if32 = flags & DM4D_EVAL_IMAGE_F32, mf32 = flags & DM4D_EVAL_MASK_F32;
  const int bg = (flags >> DM4D_EVAL_BG_SHIFT) & 3;
  const int oh = (int)d[F_OUT_H], ow = (int)d[F_OUT_W], sh = (int)d[F_SRC_H], sw = (int)d[F_SRC_W];
  const float sx_scale = (float)sw / (float)ow, sy_scale = (float)sh / (float)oh;
  const int64_t plane = (int64_t)sh * sw;
  const int tx0 = blockIdx.x * kTileW, ty0 = blockIdx.y * kTileH;  // tile origin inside the crop

  for (int i = threadIdx.x; i < kInH * kInW; i += kThreads) {
    const int cy = ty0 - kHalo + i / kInW, cx = tx0 - kHalo + i % kInW;
    float p[3] = {0.0f, 0.0f, 0.0f}, g[3] = {0.0f, 0.0f, 0.0f};
    if (cy >= 0 && cy < ch && cx >= 0 && cx < cw) {
      const int64_t idx = (int64_t)nearest(t + cy, sy_scale, sh) * sw + nearest(l + cx, sx_scale, sw);
      const bool pm = d[F_PMASK] >= 0, gm = d[F_GMASK] >= 0;
      const float mp = pm ? load_mask(blob, d[F_PMASK], mf32, idx) : 0.0f;
      const float mg = gm ? load_mask(blob, d[F_GMASK], mf32, idx) : 0.0f;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float xp = load_pixel(blob, d[F_PRED], if32, plane, idx, c);
        const float xg = load_pixel(blob, d[F_GT], if32, plane, idx, c);
        p[c] = pm ? composite(xp, mp, bg) : xp;
        g[c] = gm ? composite(xg, mg, bg) : xg;
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      sp[c][i] = p[c];
      st[c][i] = g[c];
    }
  }
  __syncthreads();

  // this lane's two pixels of the tile: (py, px) and (py + 8, px)
  const int px = threadIdx.x & (kTileW - 1), py = threadIdx.x / kTileW;
  double sse = 0.0, ssim = 0.0;
  float pmin = INFINITY, pmax = -INFINITY, gmin = INFINITY, gmax = -INFINITY;
  for (int c = 0; c < 3; ++c) {
    for (int i = threadIdx.x; i < kInH * kTileW; i += kThreads) {
      const int row = i / kTileW, col = i % kTileW;
      const float* rp = &sp[c][row * kInW + col];
      const float* rt = &st[c][row * kInW + col];
      double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0;
#pragma unroll
      for (int k = 0; k < kTaps; ++k) {
        const double w = wt.w[k], vp = (double)rp[k], vt = (double)rt[k];
        a0 += w * vp;
        a1 += w * vt;
        a2 += w * (vp * vp);
        a3 += w * (vt * vt);
        a4 += w * (vp * vt);
      }
      hb[0][i] = a0, hb[1][i] = a1, hb[2][i] = a2, hb[3][i] = a3, hb[4][i] = a4;
    }
    __syncthreads();
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int y = py + half * (kTileH / 2);
      const int cy = ty0 + y, cx = tx0 + px;
      if (cy < ch && cx < cw) {
        const float vp = sp[c][(y + kHalo) * kInW + px + kHalo], vt = st[c][(y + kHalo) * kInW + px + kHalo];
        const double e = (double)vp - (double)vt;
        sse += e * e;
        pmin = fminf(pmin, vp), pmax = fmaxf(pmax, vp), gmin = fminf(gmin, vt), gmax = fmaxf(gmax, vt);
        if (debug) {
          float* o = debug + (((int64_t)n * 2 * 3 + c) * dbg_h + cy) * dbg_w + cx;
          o[0] = vp;
          o[(int64_t)3 * dbg_h * dbg_w] = vt;
        }
        if (cy >= kHalo && cy < ch - kHalo && cx >= kHalo && cx < cw - kHalo) {  // the window fits: an interior pixel
          double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int k = 0; k < kTaps; ++k) {
            const double w = wt.w[k];
#pragma unroll
            for (int q = 0; q < 5; ++q) m[q] += w * hb[q][(y + k) * kTileW + px];
          }
          const double c1 = 1e-4, c2 = 9e-4;  // (0.01 data_range)^2, (0.03 data_range)^2
          const double mu_pp = m[0] * m[0], mu_tt = m[1] * m[1], mu_pt = m[0] * m[1];
          const double s_pp = fmax(m[2] - mu_pp, 0.0), s_tt = fmax(m[3] - mu_tt, 0.0), s_pt = m[4] - mu_pt;
          ssim += ((2.0 * mu_pt + c1) * (2.0 * s_pt + c2)) / ((mu_pp + mu_tt + c1) * (s_pp + s_tt + c2));
        }
      }
    }
    __syncthreads();  // hb is rewritten for the next channel
  }

  double* red = &hb[0][0];
  const double r_sse = block_sum(sse, red), r_ssim = block_sum(ssim, red);
  const double r_pmin = block_min((double)pmin, red), r_pmax = -block_min(-(double)pmax, red);
  const double r_gmin = block_min((double)gmin, red), r_gmax = -block_min(-(double)gmax, red);
  if (threadIdx.x == 0) {
    double* o = partials + ((int64_t)n * tiles_per_item + (int64_t)blockIdx.y * ntx + blockIdx.x) * kPart;
    o[0] = r_sse, o[1] = r_ssim, o[2] = r_pmin, o[3] = r_pmax, o[4] = r_gmin, o[5] = r_gmax;
  }
}

// ---- (c) the pair's tile records, in tile order -> {psnr, ssim, pred min, pred max, gt min, gt max, sse, ssim sum}; box -> boxes ------
__global__ void __launch_bounds__(kThreads) eval_reduce_kernel(const int64_t* __restrict__ desc, const int* __restrict__ raw,
                                                               const double* __restrict__ partials, int tiles_per_item,
                                                               double* __restrict__ out, int* __restrict__ boxes) {
  __shared__ double red[kThreads];
  const int n = blockIdx.x;
  const int64_t* d = desc + (int64_t)n * DM4D_EVAL_FIELDS;
  int l, t, r, b;
  crop_box(d, raw + 4 * n, l, t, r, b);
  const int cw = r - l, ch = b - t;
  const int tiles = ((cw + kTileW - 1) / kTileW) * ((ch + kTileH - 1) / kTileH);  // <= tiles_per_item: the box lies inside the image
  const double* p = partials + (int64_t)n * tiles_per_item * kPart;
  double sse = 0.0, ssim = 0.0, pmin = INFINITY, pmax = -INFINITY, gmin = INFINITY, gmax = -INFINITY;
  for (int i = threadIdx.x; i < tiles; i += kThreads) {
    const double* q = p + (int64_t)i * kPart;
    sse += q[0], ssim += q[1];
    pmin = fmin(pmin, q[2]), pmax = fmax(pmax, q[3]), gmin = fmin(gmin, q[4]), gmax = fmax(gmax, q[5]);
  }
  sse = block_sum(sse, red), ssim = block_sum(ssim, red);
  pmin = block_min(pmin, red), pmax = -block_min(-pmax, red), gmin = block_min(gmin, red), gmax = -block_min(-gmax, red);
  if (threadIdx.x == 0) {
    const double count = 3.0 * (double)cw * (double)ch;
    const double interior = 3.0 * (double)max(cw - 2 * kHalo, 0) * (double)max(ch - 2 * kHalo, 0);
    double* o = out + (int64_t)n * DM4D_EVAL_OUT;
    o[0] = 10.0 * log10(1.0 / (sse / count));  // identical images: 1 / 0 = inf; an empty box: NaN (the host raises on the box first)
    o[1] = ssim / interior;                    // crops of 10 pixels or less on an edge: NaN (the host raises)
    o[2] = pmin, o[3] = pmax, o[4] = gmin, o[5] = gmax, o[6] = sse, o[7] = ssim;
    int* bo = boxes + 4 * n;
    bo[0] = l, bo[1] = t, bo[2] = r, bo[3] = b;
  }
}

}  // namespace

extern "C" int dm4d_eval_psnr_ssim_f64(void* stream, const void* blob, int64_t blob_bytes, const int64_t* desc_host,
                                       const int64_t* desc_dev, int n_pairs, void* workspace, int64_t workspace_bytes, double* out,
                                       int32_t* boxes, float* debug, int dbg_h, int dbg_w) {
  if (!blob || !desc_host || !desc_dev || !workspace || !out || !boxes) return dm4d_set_error(DM4D_ERR_ARG, "eval_psnr_ssim: null pointer");
  if (n_pairs <= 0 || n_pairs > 65535 || blob_bytes <= 0) return dm4d_set_error(DM4D_ERR_ARG, "eval_psnr_ssim: empty or oversized batch");
  if (((uintptr_t)blob | (uintptr_t)workspace | (uintptr_t)out) & 15)
    return dm4d_set_error(DM4D_ERR_ARG, "eval_psnr_ssim: blob, workspace and out must be 16-byte aligned");
  int max_h = 0, max_w = 0;
  bool any_masks = false;
  for (int n = 0; n < n_pairs; ++n) {
    const int64_t* d = desc_host + (int64_t)n * DM4D_EVAL_FIELDS;
    const int64_t sh = d[F_SRC_H], sw = d[F_SRC_W], oh = d[F_OUT_H], ow = d[F_OUT_W], flags = d[F_FLAGS];
    if (sh <= 0 || sw <= 0 || oh <= 0 || ow <= 0 || sh > (1 << 15) || sw > (1 << 15) || oh > (1 << 15) || ow > (1 << 15))
      return dm4d_set_error(DM4D_ERR_ARG, "eval_psnr_ssim: bad source or resized size in a descriptor");
    if (flags < 0 || flags >= (1 << (DM4D_EVAL_BG_SHIFT + 2)) || ((flags >> DM4D_EVAL_BG_SHIFT) & 3) > 2)
      return dm4d_set_error(DM4D_ERR_ARG, "eval_psnr_ssim: bad flags in a descriptor");
    const int64_t img_bytes = sh * sw * 3 * ((flags & DM4D_EVAL_IMAGE_F32) ? 4 : 1), img_align = (flags & DM4D_EVAL_IMAGE_F32) ? 3 : 0;
    const int64_t mask_bytes = sh * sw * ((flags & DM4D_EVAL_MASK_F32) ? 4 : 1), mask_align = (flags & DM4D_EVAL_MASK_F32) ? 3 : 0;
    for (int f : {F_PRED, F_GT})
      if (d[f] < 0 || (d[f] & img_align) || d[f] + img_bytes > blob_bytes)
        return dm4d_set_error(DM4D_ERR_ARG, "eval_psnr_ssim: an image lies outside the blob or is misaligned");
    for (int f : {F_PMASK, F_GMASK})
      if (d[f] != -1 && (d[f] < 0 || (d[f] & mask_align) || d[f] + mask_bytes > blob_bytes))
        return dm4d_set_error(DM4D_ERR_ARG, "eval_psnr_ssim: a mask lies outside the blob or is misaligned");
    if (flags & DM4D_EVAL_CROP_MASKS) {
      if (d[F_PMASK] < 0 && d[F_GMASK] < 0) return dm4d_set_error(DM4D_ERR_ARG, "eval_psnr_ssim: crop by masks asked for without a mask");
      any_masks = true;
    } else if (d[F_LEFT] < 0 || d[F_TOP] < 0 || d[F_RIGHT] <= d[F_LEFT] || d[F_BOTTOM] <= d[F_TOP] || d[F_RIGHT] > ow || d[F_BOTTOM] > oh) {
      return dm4d_set_error(DM4D_ERR_ARG, "eval_psnr_ssim: a crop box is empty or leaves the resized image");
    }
    if (oh > max_h) max_h = (int)oh;
    if (ow > max_w) max_w = (int)ow;
  }
  if (debug && (dbg_h < max_h || dbg_w < max_w)) return dm4d_set_error(DM4D_ERR_ARG, "eval_psnr_ssim: debug planes smaller than a resized image");
  const unsigned gx = (unsigned)((max_w + kTileW - 1) / kTileW), gy = (unsigned)((max_h + kTileH - 1) / kTileH);
  const int tiles_per_item = (int)(gx * gy);
  // workspace: raw boxes (16 bytes per pair, rounded up to 16) | tile records
  const int64_t raw_bytes = ((int64_t)n_pairs * 16 + 15) / 16 * 16;
  if (workspace_bytes < raw_bytes + (int64_t)n_pairs * tiles_per_item * kPart * 8)
    return dm4d_set_error(DM4D_ERR_ARG, "eval_psnr_ssim: workspace too small (dm4d_eval_ws_bytes)");
  int* raw = (int*)workspace;
  double* partials = (double*)((char*)workspace + raw_bytes);
  hipStream_t st = (hipStream_t)stream;
  if (any_masks) {
    if (hipMemsetAsync(raw, 0x7f, (size_t)raw_bytes, st) != hipSuccess) return dm4d_set_error(DM4D_ERR_LAUNCH, "eval_psnr_ssim: hipMemsetAsync failed");
    hipLaunchKernelGGL(eval_bbox_kernel, dim3((max_w + kThreads - 1) / kThreads, (max_h + kBoxRows - 1) / kBoxRows, n_pairs), dim3(kThreads),
                       0, st, (const uint8_t*)blob, desc_dev, raw);
    int rc = dm4d_check_launch("eval_bbox_kernel");
    if (rc) return rc;
  }
  Weights wt;
  double total = 0.0;
  for (int k = 0; k < kTaps; ++k) total += (wt.w[k] = exp(-((k - kHalo) / 1.5) * ((k - kHalo) / 1.5) / 2.0));
  for (int k = 0; k < kTaps; ++k) wt.w[k] /= total;
  hipLaunchKernelGGL(eval_tile_kernel, dim3(gx, gy, n_pairs), dim3(kThreads), 0, st, (const uint8_t*)blob, desc_dev, raw, partials,
                     tiles_per_item, debug, dbg_h, dbg_w, wt);
  int rc = dm4d_check_launch("eval_tile_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(eval_reduce_kernel, dim3(n_pairs), dim3(kThreads), 0, st, desc_dev, raw, partials, tiles_per_item, out, boxes);
  return dm4d_check_launch("eval_reduce_kernel");
}

extern "C" size_t dm4d_eval_ws_bytes(int n_pairs, int max_h, int max_w) {
  if (n_pairs <= 0 || max_h <= 0 || max_w <= 0) return 0;
  const size_t tiles = (size_t)((max_w + kTileW - 1) / kTileW) * (size_t)((max_h + kTileH - 1) / kTileH);
  return ((size_t)n_pairs * 16 + 15) / 16 * 16 + (size_t)n_pairs * tiles * kPart * 8;
}
