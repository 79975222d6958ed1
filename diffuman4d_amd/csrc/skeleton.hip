// Skeleton maps (scripts/preprocess/draw_skeleton.py): a frame's ordered list of thick lines and filled circles is painted on a canvas
// of up to 2048 x 2048 pixels and the canvas is reduced with Pillow's Image.resize (BICUBIC) -- one launch for a batch of frames, and
// the canvas never reaches memory: a workgroup owns one T x T tile of the OUTPUT and holds only the part of the canvas that the tile's
// bicubic windows read (its footprint) in LDS.
//
//   cull        one lane per primitive: does its bounding box (grown by half the thickness, or the radius) meet the footprint?  A ballot
//               per wave and the waves' counts give every kept primitive its place, so the list in LDS keeps the frame's order.  The list
//               has room for all of a frame's primitives (DM4D_SKEL_MAX_PRIMS, checked on the host): nothing is ever left out.
//   rasterise   one lane per footprint pixel: the list is walked from the back, the first primitive that covers the pixel gives its
//               colour (= the last one painted wins), an uncovered pixel is black.  Coverage is the integer rule of dm4d.h, evaluated
//               in int64: with coordinates in [-8192, 8191] and pixels in [0, 4096) the largest term, 4 (v x d)^2, stays below 2^61.
//   horizontal  Pillow's pass along x over the footprint rows, rounded and clipped to uint8 (pillow_rgb, image_common.h), into LDS
//   vertical    the pass along y over those bytes; the tile's RGB bytes are staged in LDS and stored row by row
//
// A tile with an empty list stores zeros and skips the passes (most of a map is black).  The result is a function of the frame's own
// list only: no atomics, nothing depends on the order of blocks, on the batch or on the tile size.  Integer arithmetic throughout.
//
// The list comes either from the host (dm4d_skeleton_draw_u8: records and offsets validated there) or from a plan made on the device
// (dm4d_skeleton_draw_planned_u8: a fixed stride per frame, the count clamped in the kernel); the plan kernel, which projects a scene's
// 3-D keypoints and does host/skeleton.py plan_draw_calls' arithmetic in fp64 / fp32, is at the end of this file.
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "common.h"
#include "dm4d.h"
#include "errors.h"
#include "image_common.h"
#include "project_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kLdsLimit = 64 * 1024;  // per workgroup: what a launch gets without asking for more; two or more tiles per CU
constexpr int kMaxCanvas = 4096;
constexpr int kMaxTaps = 4096;

enum { P_KIND = 0, P_X1, P_Y1, P_X2, P_Y2, P_SIZE, P_COLOR };

struct Prim {
  int kind, x1, y1, x2, y2, size;
  uint32_t color;
};

__device__ __forceinline__ Prim load_prim(const int32_t* p) {
  const U4 a = *reinterpret_cast<const U4*>(p), b = *reinterpret_cast<const U4*>(p + 4);
  return Prim{(int)a.x, (int)a.y, (int)a.z, (int)a.w, (int)b.x, (int)b.y, b.z};
}

// the coverage rule of dm4d.h ("Rasteriser")
__device__ __forceinline__ bool covers(const Prim& p, int x, int y) {
  const int64_t vx = x - p.x1, vy = y - p.y1, s = p.size;
  const int64_t r1 = vx * vx + vy * vy;
  if (p.kind == DM4D_SKEL_CIRCLE) return r1 <= s * s;
  const int64_t t2 = s * s;
  if (4 * r1 <= t2) return true;
  const int64_t wx = x - p.x2, wy = y - p.y2;
  if (4 * (wx * wx + wy * wy) <= t2) return true;
  const int64_t dx = p.x2 - p.x1, dy = p.y2 - p.y1, l2 = dx * dx + dy * dy;
  if (l2 == 0) return false;
  const int64_t dot = vx * dx + vy * dy;
  if (dot < 0 || dot > l2) return false;
  const int64_t cr = vx * dy - vy * dx;
  return 4 * cr * cr <= t2 * l2;
}

// LDS of one workgroup: the list, the footprint, the rows after the horizontal pass, the tile's bytes, the waves' counts
__host__ __device__ inline size_t lds_bytes(int T, int cap, int fh, int fw) {
  return (size_t)cap * DM4D_SKEL_FIELDS * 4 + (size_t)fh * fw * 4 + (size_t)fh * T * 4 + (size_t)T * T * 3 + 64;
}

template <int T>
__global__ void __launch_bounds__(kThreads) skeleton_draw_kernel(const int32_t* __restrict__ prims, const int32_t* __restrict__ offsets,
                                                                 const int32_t* __restrict__ htab, int hk, const int32_t* __restrict__ vtab,
                                                                 int vk, int h, int w, int cap, int fh_max, int fw_max, int stride,
                                                                 uint8_t* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int32_t* s_list = reinterpret_cast<int32_t*>(smem);                      // [cap][DM4D_SKEL_FIELDS]
  uint32_t* s_canvas = reinterpret_cast<uint32_t*>(s_list + (size_t)cap * DM4D_SKEL_FIELDS);  // [fh][fw] r | g << 8 | b << 16
  uint32_t* s_rows = s_canvas + (size_t)fh_max * fw_max;                   // [fh][T] after the horizontal pass
  uint8_t* s_tile = reinterpret_cast<uint8_t*>(s_rows + (size_t)fh_max * T);  // [T][3 T]
  int* s_cnt = reinterpret_cast<int*>(s_tile + T * T * 3);                 // [kWaves]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int f = blockIdx.z;
  const int ox0 = blockIdx.x * T, oy0 = blockIdx.y * T;
  const int ncols = min(T, w - ox0), nrows = min(T, h - oy0);
  const int32_t* hcoef = htab + 2 * w;
  const int32_t* vcoef = vtab + 2 * h;
  // window starts and ends do not decrease along an axis (checked on the host): the first and the last window bound the footprint
  const int fx0 = htab[2 * ox0], fx1 = htab[2 * (ox0 + ncols - 1)] + htab[2 * (ox0 + ncols - 1) + 1];
  const int fy0 = vtab[2 * oy0], fy1 = vtab[2 * (oy0 + nrows - 1)] + vtab[2 * (oy0 + nrows - 1) + 1];
  const int fw = fx1 - fx0, fh = fy1 - fy0;

  // cull, keeping the order.  The two front ends differ here only: stride == 0: frame f owns records offsets[f] .. offsets[f + 1] - 1
  // (validated on the host); stride > 0 (a device plan): records f * stride .. + offsets[f] - 1, the count clamped to the stride
  const int p0 = stride ? f * stride : offsets[f];
  const int np = stride ? min(max(offsets[f], 0), stride) : offsets[f + 1] - p0;
  int n = 0;
  for (int base = 0; base < np; base += kThreads) {
    const int i = base + tid;
    bool keep = false;
    Prim p{};
    if (i < np) {
      p = load_prim(prims + (int64_t)(p0 + i) * DM4D_SKEL_FIELDS);
      const int grow = p.kind == DM4D_SKEL_CIRCLE ? p.size : (p.size + 1) / 2;
      keep = min(p.x1, p.x2) - grow < fx1 && max(p.x1, p.x2) + grow >= fx0 && min(p.y1, p.y2) - grow < fy1 && max(p.y1, p.y2) + grow >= fy0;
    }
    const uint64_t mask = __ballot(keep);
    if (lane == 0) s_cnt[wave] = __popcll(mask);
    __syncthreads();
    int before = n, total = n;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
      const int c = s_cnt[k];
      if (k < wave) before += c;
      total += c;
    }
    if (keep) {
      int32_t* dst = s_list + (size_t)(before + __popcll(mask & ((1ull << lane) - 1))) * DM4D_SKEL_FIELDS;
      *reinterpret_cast<U4*>(dst) = U4{(uint32_t)p.kind, (uint32_t)p.x1, (uint32_t)p.y1, (uint32_t)p.x2};
      *reinterpret_cast<U4*>(dst + 4) = U4{(uint32_t)p.y2, (uint32_t)p.size, p.color, 0u};
    }
    n = total;
    __syncthreads();
  }

  uint8_t* tile_out = out + (((int64_t)f * h + oy0) * w + ox0) * 3;
  const int row_bytes = ncols * 3;
  if (n == 0) {  // the same for every thread
    for (int i = tid; i < nrows * row_bytes; i += kThreads) tile_out[(int64_t)(i / row_bytes) * w * 3 + i % row_bytes] = 0;
    return;
  }

  // rasterise the footprint
  const int npx = fh * fw;
  for (int base = 0; base < npx; base += kThreads) {
    const int i = base + tid;
    const int y = fy0 + i / fw, x = fx0 + i % fw;
    bool open = i < npx;
    uint32_t color = 0;
    for (int k = n - 1; k >= 0; --k) {  // all lanes of a wave read the same record
      const Prim p = load_prim(s_list + (size_t)k * DM4D_SKEL_FIELDS);
      if (open && covers(p, x, y)) {
        color = p.color;
        open = false;
      }
      if (__ballot(open) == 0) break;
    }
    if (i < npx) s_canvas[i] = color;
  }
  __syncthreads();

  // horizontal pass: rows of the footprint x columns of the tile
  for (int i = tid; i < fh * T; i += kThreads) {
    const int r = i / T, j = i % T;
    if (j >= ncols) continue;
    const int ox = ox0 + j;
    const int xmin = htab[2 * ox] - fx0, cnt = htab[2 * ox + 1];
    const int32_t* k = hcoef + (int64_t)ox * hk;
    uint32_t o[3];
    pillow_rgb(PackedRgb{s_canvas + r * fw + xmin, 1}, k, cnt, o);
    s_rows[r * T + j] = o[0] | (o[1] << 8) | (o[2] << 16);
  }
  __syncthreads();

  // vertical pass
  for (int i = tid; i < T * T; i += kThreads) {
    const int r = i / T, j = i % T;
    if (r >= nrows || j >= ncols) continue;
    const int oy = oy0 + r;
    const int ymin = vtab[2 * oy] - fy0, cnt = vtab[2 * oy + 1];
    const int32_t* k = vcoef + (int64_t)oy * vk;
    uint32_t o[3];
    pillow_rgb(PackedRgb{s_rows + ymin * T + j, T}, k, cnt, o);
    uint8_t* dst = s_tile + (r * T + j) * 3;
    dst[0] = (uint8_t)o[0];
    dst[1] = (uint8_t)o[1];
    dst[2] = (uint8_t)o[2];
  }
  __syncthreads();
  for (int i = tid; i < nrows * row_bytes; i += kThreads) {
    const int r = i / row_bytes, c = i % row_bytes;
    tile_out[(int64_t)r * w * 3 + c] = s_tile[r * T * 3 + c];
  }
}

// the largest footprint extent along one axis over tiles of T outputs
int max_extent(const int32_t* tab, int n, int T) {
  int best = 0;
  for (int o0 = 0; o0 < n; o0 += T) {
    const int last = (o0 + T < n ? o0 + T : n) - 1;
    const int ext = tab[2 * last] + tab[2 * last + 1] - tab[2 * o0];
    if (ext > best) best = ext;
  }
  return best;
}

template <int T>
int launch(hipStream_t stream, const int32_t* prims, const int32_t* offsets, int n_frames, const int32_t* htab, int hk, const int32_t* vtab,
           int vk, int h, int w, int cap, int fh, int fw, int stride, uint8_t* out) {
  const dim3 grid((unsigned)((w + T - 1) / T), (unsigned)((h + T - 1) / T), (unsigned)n_frames);
  hipLaunchKernelGGL(skeleton_draw_kernel<T>, grid, dim3(kThreads), lds_bytes(T, cap, fh, fw), stream, prims, offsets, htab, hk, vtab, vk, h,
                     w, cap, fh, fw, stride, out);
  return dm4d_check_launch("skeleton_draw_kernel");
}

// what both draw entries know on the host: shapes and alignment, then (after an entry's own checks) tables and windows
int draw_error(const char* who, const char* what) {
  static thread_local char msg[256];
  snprintf(msg, sizeof(msg), "%s: %s", who, what);
  return dm4d_set_error(DM4D_ERR_ARG, msg);
}

int check_draw_shapes(const char* who, const void* prims_dev, const void* counts_dev, int n_frames, const void* htab_dev, int hk,
                      const void* vtab_dev, int vk, int H, int W, int h, int w) {
  if (n_frames <= 0 || n_frames > 65535 || H <= 0 || W <= 0 || H > kMaxCanvas || W > kMaxCanvas || h <= 0 || w <= 0 || h > (1 << 15) ||
      w > (1 << 15) || hk < 1 || vk < 1 || hk > kMaxTaps || vk > kMaxTaps)
    return draw_error(who, "empty or oversized shape");
  if (((uintptr_t)prims_dev & 15) || ((uintptr_t)counts_dev & 3) || ((uintptr_t)htab_dev & 3) || ((uintptr_t)vtab_dev & 3))
    return draw_error(who, "the records must be 16-byte aligned, offsets and tables 4-byte aligned");
  return 0;
}

int check_draw_tables(const char* who, const int32_t* htab_host, int hk, const int32_t* vtab_host, int vk, int H, int W, int h, int w) {
  if (!pillow_table_ok(htab_host, (int64_t)w * (2 + hk), 0, hk, kMaxTaps, w, W, true) ||
      !pillow_table_ok(vtab_host, (int64_t)h * (2 + vk), 0, vk, kMaxTaps, h, H, true))
    return draw_error(who, "a coefficient table's windows leave the canvas, exceed ksize or are not ordered");
  return 0;
}

// the largest tile whose footprint fits in LDS beside a list of `cap` records; stride as skeleton_draw_kernel takes it
int launch_draw(const char* who, void* stream, const int32_t* prims_dev, const int32_t* counts_dev, int n_frames, int cap, int stride,
                const int32_t* htab_host, const int32_t* htab_dev, int hk, const int32_t* vtab_host, const int32_t* vtab_dev, int vk, int h,
                int w, uint8_t* out) {
  const hipStream_t s = (hipStream_t)stream;
  for (int T : {32, 16, 8}) {
    const int fw = max_extent(htab_host, w, T), fh = max_extent(vtab_host, h, T);
    if (lds_bytes(T, cap, fh, fw) > (size_t)kLdsLimit || (w + T - 1) / T > 65535 || (h + T - 1) / T > 65535) continue;
    if (T == 32) return launch<32>(s, prims_dev, counts_dev, n_frames, htab_dev, hk, vtab_dev, vk, h, w, cap, fh, fw, stride, out);
    if (T == 16) return launch<16>(s, prims_dev, counts_dev, n_frames, htab_dev, hk, vtab_dev, vk, h, w, cap, fh, fw, stride, out);
    return launch<8>(s, prims_dev, counts_dev, n_frames, htab_dev, hk, vtab_dev, vk, h, w, cap, fh, fw, stride, out);
  }
  return draw_error(who, "the canvas is too large for the output: an 8 x 8 tile's footprint does not fit in LDS");
}

}  // namespace

extern "C" int dm4d_skeleton_draw_u8(void* stream, const int32_t* prims_host, const int32_t* prims_dev, const int32_t* offsets_host,
                                     const int32_t* offsets_dev, int n_frames, const int32_t* htab_host, const int32_t* htab_dev, int hk,
                                     const int32_t* vtab_host, const int32_t* vtab_dev, int vk, int H, int W, int h, int w, uint8_t* out) {
  if (!prims_host || !prims_dev || !offsets_host || !offsets_dev || !htab_host || !htab_dev || !vtab_host || !vtab_dev || !out)
    return dm4d_set_error(DM4D_ERR_ARG, "skeleton_draw: null pointer");
  if (const int rc = check_draw_shapes("skeleton_draw", prims_dev, offsets_dev, n_frames, htab_dev, hk, vtab_dev, vk, H, W, h, w)) return rc;
  if (offsets_host[0] != 0) return dm4d_set_error(DM4D_ERR_ARG, "skeleton_draw: offsets[0] must be 0");
  int cap = 1;
  for (int f = 0; f < n_frames; ++f) {
    const int64_t np = (int64_t)offsets_host[f + 1] - offsets_host[f];
    if (np < 0 || np > DM4D_SKEL_MAX_PRIMS || offsets_host[f + 1] > (1 << 28))
      return dm4d_set_error(DM4D_ERR_ARG, "skeleton_draw: a frame's primitive count is negative or above DM4D_SKEL_MAX_PRIMS");
    if (np > cap) cap = (int)np;
  }
  for (int64_t i = 0; i < offsets_host[n_frames]; ++i) {
    const int32_t* p = prims_host + i * DM4D_SKEL_FIELDS;
    if (p[P_KIND] != DM4D_SKEL_LINE && p[P_KIND] != DM4D_SKEL_CIRCLE) return dm4d_set_error(DM4D_ERR_ARG, "skeleton_draw: unknown primitive kind");
    for (int c = P_X1; c <= P_Y2; ++c)
      if (p[c] < DM4D_SKEL_COORD_MIN || p[c] > DM4D_SKEL_COORD_MAX)
        return dm4d_set_error(DM4D_ERR_ARG, "skeleton_draw: a coordinate lies outside [DM4D_SKEL_COORD_MIN, DM4D_SKEL_COORD_MAX]");
    if (p[P_SIZE] < (p[P_KIND] == DM4D_SKEL_LINE ? 1 : 0) || p[P_SIZE] > DM4D_SKEL_MAX_SIZE)
      return dm4d_set_error(DM4D_ERR_ARG, "skeleton_draw: a thickness below 1, a negative radius, or a size above DM4D_SKEL_MAX_SIZE");
    if ((uint32_t)p[P_COLOR] >> 24) return dm4d_set_error(DM4D_ERR_ARG, "skeleton_draw: a colour has bits above r | g << 8 | b << 16");
  }
  if (const int rc = check_draw_tables("skeleton_draw", htab_host, hk, vtab_host, vk, H, W, h, w)) return rc;
  return launch_draw("skeleton_draw", stream, prims_dev, offsets_dev, n_frames, cap, 0, htab_host, htab_dev, hk, vtab_host, vtab_dev, vk, h, w, out);
}

// the same rasteriser and reduction on a plan that dm4d_skeleton_plan_kp3d left on the device
extern "C" int dm4d_skeleton_draw_planned_u8(void* stream, const int32_t* records, const int32_t* counts, int n_frames, int stride,
                                             const int32_t* htab_host, const int32_t* htab_dev, int hk, const int32_t* vtab_host,
                                             const int32_t* vtab_dev, int vk, int H, int W, int h, int w, uint8_t* out) {
  if (!records || !counts || !htab_host || !htab_dev || !vtab_host || !vtab_dev || !out)
    return dm4d_set_error(DM4D_ERR_ARG, "skeleton_draw_planned: null pointer");
  if (stride < 3 || stride > DM4D_SKEL_MAX_PRIMS || stride % 3)
    return dm4d_set_error(DM4D_ERR_ARG, "skeleton_draw_planned: stride must be 3 L, a multiple of 3 in 3 .. DM4D_SKEL_MAX_PRIMS");
  if (const int rc = check_draw_shapes("skeleton_draw_planned", records, counts, n_frames, htab_dev, hk, vtab_dev, vk, H, W, h, w)) return rc;
  if (const int rc = check_draw_tables("skeleton_draw_planned", htab_host, hk, vtab_host, vk, H, W, h, w)) return rc;
  return launch_draw("skeleton_draw_planned", stream, records, counts, n_frames, stride, stride, htab_host, htab_dev, hk, vtab_host, vtab_dev, vk,
                     h, w, out);
}

// Bounding box and box mask of drawn maps (crop_utils.py skeleton_to_mask on the maps above, for SpaTemDataset's has_gt_target=False
// targets).  A pixel counts when any of its three bytes is non-zero.
//
//   extrema  grid (blocks per frame, frames): a block walks its share of the frame's 16-byte vectors (a scalar head of up to 15 bytes
//            before the first aligned address and a tail of up to 15 after the last vector go to block 0); a vector that is all zero
//            -- most of a map -- costs one load and one test, any other is walked byte by byte.  Shuffles reduce a wave, LDS the block,
//            and thread 0 stores the block's {first column, first row, last column, last row} in the workspace.
//   reduce   one wave per frame folds the frame's partials (a fixed assignment to lanes, then the shuffle tree) into boxes[f].
//   fill     grid (blocks per frame, frames): 255 inside the padded and clamped rectangle, 0 outside, read from boxes[f] on the device.
//
// min and max of integers: no atomics, no block waits on another, and a frame's result does not depend on the batch it is in.
namespace {

constexpr int kBoxThreads = 256;
constexpr int kBoxMaxBlocks = 256;       // per frame
constexpr int kBoxVecsPerThread = 8;     // 32 KiB of a map per block before the grid stride sets in

__host__ __device__ inline int box_blocks(int64_t frame_bytes) {
  const int64_t per_block = (int64_t)kBoxThreads * kBoxVecsPerThread * 16;
  const int64_t n = (frame_bytes + per_block - 1) / per_block;
  return (int)(n < 1 ? 1 : n > kBoxMaxBlocks ? kBoxMaxBlocks : n);
}

__global__ void __launch_bounds__(kBoxThreads) skeleton_box_partial_kernel(const uint8_t* __restrict__ maps, int64_t frame_bytes, int h, int w,
                                                                           int32_t* __restrict__ partials) {
  const int tid = threadIdx.x, f = blockIdx.y, nblocks = gridDim.x;
  Box b{w, h, -1, -1};
  box_scan_plane<3, 0xffffffffu>(maps + (int64_t)f * frame_bytes, frame_bytes, w * 3, (int64_t)blockIdx.x * kBoxThreads + tid,
                                 (int64_t)nblocks * kBoxThreads, blockIdx.x == 0, b);
  box_block_reduce<kBoxThreads>(b);
  if (tid == 0) {
    int32_t* dst = partials + ((int64_t)f * nblocks + blockIdx.x) * 4;
    dst[0] = b.fc, dst[1] = b.fr, dst[2] = b.lc, dst[3] = b.lr;
  }
}

__global__ void __launch_bounds__(64) skeleton_box_reduce_kernel(const int32_t* __restrict__ partials, int nblocks, int h, int w,
                                                                 int32_t* __restrict__ boxes) {
  const int f = blockIdx.x, lane = threadIdx.x;  // one wave per frame
  Box b{w, h, -1, -1};
  const int32_t* p = partials + (int64_t)f * nblocks * 4;
  for (int k = lane; k < nblocks; k += 64) box_merge(b, Box{p[4 * k], p[4 * k + 1], p[4 * k + 2], p[4 * k + 3]});
  box_wave_reduce(b);
  if (lane == 0) {
    int32_t* dst = boxes + (int64_t)f * 4;
    dst[0] = b.fc, dst[1] = b.fr, dst[2] = b.lc, dst[3] = b.lr;
  }
}

__global__ void __launch_bounds__(kBoxThreads) skeleton_box_fill_kernel(const int32_t* __restrict__ boxes, int h, int w, int pad_top,
                                                                        int pad_bottom, int pad_x, uint8_t* __restrict__ masks,
                                                                        int64_t mask_stride) {
  const int f = blockIdx.y;
  const int32_t* bx = boxes + (int64_t)f * 4;
  const int fc = bx[0], fr = bx[1], lc = bx[2], lr = bx[3];
  int c0 = 0, c1 = 0, r0 = 0, r1 = 0;  // an all-zero map keeps an all-zero mask
  if (lc >= 0) {
    c0 = max(fc - 1 - pad_x, 0), c1 = min(lc + 1 + pad_x, w);
    r0 = max(fr - 1 - pad_top, 0), r1 = min(lr + 1 + pad_bottom, h);
  }
  rect_fill_plane(masks + (int64_t)f * mask_stride, h, w, c0, r0, c1, r1, (int64_t)blockIdx.x * kBoxThreads + threadIdx.x,
                  (int64_t)gridDim.x * kBoxThreads, blockIdx.x == 0);
}

}  // namespace

extern "C" size_t dm4d_skeleton_box_mask_ws_bytes(int n_frames, int h, int w) {
  if (n_frames <= 0 || h <= 0 || w <= 0 || h > (1 << 15) || w > (1 << 15)) return 0;
  return (size_t)n_frames * box_blocks((int64_t)h * w * 3) * 4 * sizeof(int32_t);
}

extern "C" int dm4d_skeleton_box_mask_u8(void* stream, const uint8_t* maps, int n_frames, int h, int w, int pad_top, int pad_bottom,
                                         int pad_x, int32_t* boxes, uint8_t* masks, int64_t mask_stride, void* ws, int64_t ws_bytes) {
  if (!maps || !boxes || !masks || !ws) return dm4d_set_error(DM4D_ERR_ARG, "skeleton_box_mask: null pointer");
  if (n_frames <= 0 || n_frames > 65535 || h <= 0 || w <= 0 || h > (1 << 15) || w > (1 << 15))
    return dm4d_set_error(DM4D_ERR_ARG, "skeleton_box_mask: empty or oversized shape");
  if (pad_top < 0 || pad_bottom < 0 || pad_x < 0 || pad_top > (1 << 17) || pad_bottom > (1 << 17) || pad_x > (1 << 17))
    return dm4d_set_error(DM4D_ERR_ARG, "skeleton_box_mask: a padding is negative or oversized");
  if (mask_stride < (int64_t)h * w) return dm4d_set_error(DM4D_ERR_ARG, "skeleton_box_mask: mask_stride is below h * w: the slots overlap");
  if (((uintptr_t)boxes & 3) || ((uintptr_t)ws & 3)) return dm4d_set_error(DM4D_ERR_ARG, "skeleton_box_mask: boxes and workspace must be 4-byte aligned");
  if (ws_bytes < 0 || (size_t)ws_bytes < dm4d_skeleton_box_mask_ws_bytes(n_frames, h, w))
    return dm4d_set_error(DM4D_ERR_ARG, "skeleton_box_mask: the workspace is smaller than dm4d_skeleton_box_mask_ws_bytes");
  const hipStream_t s = (hipStream_t)stream;
  const int64_t frame_bytes = (int64_t)h * w * 3;
  const int nb = box_blocks(frame_bytes);
  hipLaunchKernelGGL(skeleton_box_partial_kernel, dim3(nb, n_frames), dim3(kBoxThreads), 0, s, maps, frame_bytes, h, w, (int32_t*)ws);
  int rc = dm4d_check_launch("skeleton_box_partial_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(skeleton_box_reduce_kernel, dim3(n_frames), dim3(64), 0, s, (const int32_t*)ws, nb, h, w, boxes);
  rc = dm4d_check_launch("skeleton_box_reduce_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(skeleton_box_fill_kernel, dim3(box_blocks((int64_t)h * w), n_frames), dim3(kBoxThreads), 0, s, (const int32_t*)boxes, h, w,
                     pad_top, pad_bottom, pad_x, masks, mask_stride);
  return dm4d_check_launch("skeleton_box_fill_kernel");
}

// A map's draw plan straight from poses_3d (host/skeleton.py plan_draw_calls on the poses_2d file that triangulate_skeleton would have
// written for the map's frame and camera; DESIGN.md "Skeleton maps from poses_3d").  One wave = one workgroup = one map.
//
//   keypoints  lanes over the k keypoints: project_point (project_common.h, the function dm4d_project_points_f64 evaluates), u, v and
//              depth rounded to fp32 (what reading the file into a float32 array does), score 0 where min(u, v) < 0, the scaling and
//              centring in fp64 on the widened fp32 values, rint, the [COORD_MIN, COORD_MAX] test -> LDS.  Ballots tell whether any
//              depth is non-zero and whether any score differs from 1 (over all keypoints, linked or not: the sort branch).
//   links      lanes over the L links: line score, the keep / non-finite / dropped / no-colour decisions and the sort key -> LDS
//   rank       a kept link's place is the number of kept links with a smaller key plus the number with an equal key earlier in the list
//              (descending depth: the key is the negated mean depth): Python's stable sorted() without a sort; every lane counts over all
//              L keys in LDS, so the result does not depend on any schedule.  The link writes its three records at 3 x rank.
//
// The slots past the map's count are zeroed: the whole output is a function of the map's own inputs.  Every loop runs to k or L.
namespace {

constexpr int kPlanThreads = 64;

__host__ __device__ inline size_t plan_lds_bytes(int k, int L) { return (size_t)L * 12 + (size_t)k * 20; }

// np.round(rgb * norm).astype(np.uint8) of one channel (norm lies in [0, 1] up to rounding; a NaN gives 0)
__device__ __forceinline__ uint32_t dim_channel(float c, float norm) {
  const float v = rintf(c * norm);
  return v >= 255.0f ? 255u : v > 0.0f ? (uint32_t)v : 0u;
}

// dimmed() of host/skeleton.py: (clip(score, low, high) - low) / span in fp32, span = fp32(high - low) formed in fp64 on the host
__device__ __forceinline__ uint32_t dimmed(const float* __restrict__ rgb, float score, float low, float high, float span) {
  const float clipped = score != score ? score : fminf(fmaxf(score, low), high);
  const float norm = (clipped - low) / span;
  return dim_channel(rgb[0], norm) | (dim_channel(rgb[1], norm) << 8) | (dim_channel(rgb[2], norm) << 16);
}

// np.minimum: a NaN wins
__device__ __forceinline__ float min_nan(float a, float b) { return a != a ? a : b != b ? b : fminf(a, b); }

__device__ __forceinline__ void store_record(int32_t* dst, int kind, int x1, int y1, int x2, int y2, int size, uint32_t color) {
  *reinterpret_cast<U4*>(dst) = U4{(uint32_t)kind, (uint32_t)x1, (uint32_t)y1, (uint32_t)x2};
  *reinterpret_cast<U4*>(dst + 4) = U4{(uint32_t)y2, (uint32_t)size, color, 0u};
}

__global__ void __launch_bounds__(kPlanThreads) skeleton_plan_kp3d_kernel(
    const double* __restrict__ kp3d, const double* __restrict__ K, const double* __restrict__ T, const int32_t* __restrict__ jobs,
    const float* __restrict__ scores, const double* __restrict__ scale, const int32_t* __restrict__ sizes, const int32_t* __restrict__ links,
    const float* __restrict__ colors, int k, int L, float low, float high, float span, int32_t* __restrict__ records,
    int32_t* __restrict__ counts, int32_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* s_key = reinterpret_cast<double*>(smem);         // [L]
  int32_t* s_keep = reinterpret_cast<int32_t*>(s_key + L); // [L]
  int32_t* s_x = s_keep + L;                               // [k] rounded, 0 when out of range
  int32_t* s_y = s_x + k;
  float* s_score = reinterpret_cast<float*>(s_y + k);
  float* s_depth = s_score + k;
  int32_t* s_flag = reinterpret_cast<int32_t*>(s_depth + k);  // 1: finite on the canvas, 2: inside [COORD_MIN, COORD_MAX]

  const int lane = threadIdx.x, map = blockIdx.x;
  const int f = jobs[2 * map], cam = jobs[2 * map + 1];
  const double ratio = scale[2 * map], offset = scale[2 * map + 1];
  const int radius = sizes[2 * map], thickness = sizes[2 * map + 1];
  const double* Kc = K + (int64_t)cam * 9;
  const double* Tc = T + (int64_t)cam * 16;

  bool any_depth = false, any_score = false;
  for (int base = 0; base < k; base += kPlanThreads) {
    const int i = base + lane;
    if (i < k) {
      const double* Xp = kp3d + ((int64_t)f * k + i) * 3;
      const double X[3] = {Xp[0], Xp[1], Xp[2]};
      double u, v, z;
      project_point(Kc, Tc, X, u, v, z);
      const float uf = (float)u, vf = (float)v, df = (float)z;
      float s = scores ? scores[(int64_t)map * k + i] : 1.0f;
      if (uf == uf && vf == vf && (uf < 0.0f || vf < 0.0f)) s = 0.0f;  // kpts.min(axis=1) < 0: a NaN makes the minimum NaN
      const double xs = (double)uf * ratio + offset, ys = (double)vf * ratio + offset;
      const double rx = rint(xs), ry = rint(ys);
      int flag = 0;
      if (isfinite(xs) && isfinite(ys)) flag |= 1;
      if (rx >= DM4D_SKEL_COORD_MIN && rx <= DM4D_SKEL_COORD_MAX && ry >= DM4D_SKEL_COORD_MIN && ry <= DM4D_SKEL_COORD_MAX) flag |= 2;
      s_x[i] = (flag & 2) ? (int)rx : 0;
      s_y[i] = (flag & 2) ? (int)ry : 0;
      s_score[i] = s;
      s_depth[i] = df;
      s_flag[i] = flag;
      any_depth |= df != 0.0f;
      any_score |= s != 1.0f;
    }
  }
  const bool by_depth = __ballot(any_depth) != 0;
  const bool by_score = !by_depth && __ballot(any_score) != 0;
  __syncthreads();

  int n_keep = 0, dropped = 0, first_nocolor = L;
  bool nonfinite = false;
  for (int base = 0; base < L; base += kPlanThreads) {
    const int l = base + lane;
    bool keep = false;
    if (l < L) {
      const int i1 = links[l * DM4D_SKEL_LINK_FIELDS], i2 = links[l * DM4D_SKEL_LINK_FIELDS + 1];
      const float line_score = min_nan(s_score[i1], s_score[i2]);
      keep = !(line_score < low);
      if (keep && !((s_flag[i1] & s_flag[i2]) & 1)) nonfinite = true;
      const bool inside = ((s_flag[i1] & s_flag[i2]) & 2) != 0;
      if (keep && !inside) ++dropped;
      keep = keep && inside;
      if (keep && (colors[i1 * 4 + 3] == 0.0f || colors[i2 * 4 + 3] == 0.0f) && l < first_nocolor) first_nocolor = l;
      s_key[l] = by_depth ? -(((double)s_depth[i1] + (double)s_depth[i2]) / 2) : by_score ? (double)line_score : 0.0;
      s_keep[l] = keep;
    }
    n_keep += __popcll(__ballot(keep));
  }
  __syncthreads();
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    dropped += __shfl_xor(dropped, off);
    first_nocolor = min(first_nocolor, __shfl_xor(first_nocolor, off));
  }
  const bool any_nonfinite = __ballot(nonfinite) != 0;

  int32_t* rec = records + (int64_t)map * 3 * L * DM4D_SKEL_FIELDS;
  for (int base = 0; base < L; base += kPlanThreads) {
    const int l = base + lane;
    if (l < L && s_keep[l]) {
      const double key = s_key[l];
      int rank = 0;
      for (int j = 0; j < L; ++j) {
        const double kj = s_key[j];
        if (s_keep[j] && (kj < key || (kj == key && j < l))) ++rank;
      }
      const int32_t* link = links + l * DM4D_SKEL_LINK_FIELDS;
      const int i1 = link[0], i2 = link[1];
      const float s1 = s_score[i1], s2 = s_score[i2];
      int32_t* dst = rec + (int64_t)rank * 3 * DM4D_SKEL_FIELDS;
      store_record(dst, DM4D_SKEL_LINE, s_x[i1], s_y[i1], s_x[i2], s_y[i2], thickness * link[4],
                   dimmed(colors + (int64_t)(k + l) * 4, min_nan(s1, s2), low, high, span));
      store_record(dst + DM4D_SKEL_FIELDS, DM4D_SKEL_CIRCLE, s_x[i1], s_y[i1], s_x[i1], s_y[i1], radius * link[3],
                   dimmed(colors + i1 * 4, s1, low, high, span));
      store_record(dst + 2 * DM4D_SKEL_FIELDS, DM4D_SKEL_CIRCLE, s_x[i2], s_y[i2], s_x[i2], s_y[i2], radius * link[3],
                   dimmed(colors + i2 * 4, s2, low, high, span));
    }
  }
  for (int slot = 3 * n_keep + lane; slot < 3 * L; slot += kPlanThreads) store_record(rec + (int64_t)slot * DM4D_SKEL_FIELDS, 0, 0, 0, 0, 0, 0, 0u);
  if (lane == 0) {
    counts[map] = 3 * n_keep;
    const int nocolor = first_nocolor < L;
    status[2 * map] = (any_nonfinite ? DM4D_SKEL_ST_NONFINITE : 0) | (nocolor ? DM4D_SKEL_ST_NOCOLOR | (first_nocolor << DM4D_SKEL_ST_LINK_SHIFT) : 0);
    status[2 * map + 1] = dropped;
  }
}

}  // namespace

extern "C" int dm4d_skeleton_plan_kp3d(void* stream, const double* kp3d, const double* K, const double* T, int F, int m, int k,
                                       const int32_t* jobs_host, const int32_t* jobs_dev, int n_maps, const float* scores,
                                       const double* scale_host, const double* scale_dev, const int32_t* sizes_host, const int32_t* sizes_dev,
                                       const int32_t* links_host, const int32_t* links_dev, int L, const float* colors_host,
                                       const float* colors_dev, float low_thr, float high_thr, float thr_span, int32_t* records,
                                       int32_t* counts, int32_t* status) {
  if (!kp3d || !K || !T || !jobs_host || !jobs_dev || !scale_host || !scale_dev || !sizes_host || !sizes_dev || !links_host || !links_dev ||
      !colors_host || !colors_dev || !records || !counts || !status)
    return dm4d_set_error(DM4D_ERR_ARG, "skeleton_plan_kp3d: null pointer");
  if (F <= 0 || m <= 0 || k <= 0 || L <= 0 || n_maps <= 0 || n_maps > 65535 || k > DM4D_SKEL_MAX_KPTS)
    return dm4d_set_error(DM4D_ERR_ARG, "skeleton_plan_kp3d: empty shape, more than 65535 maps or more than DM4D_SKEL_MAX_KPTS keypoints");
  if (3 * (int64_t)L > DM4D_SKEL_MAX_PRIMS)
    return dm4d_set_error(DM4D_ERR_ARG, "skeleton_plan_kp3d: 3 L records a map exceed DM4D_SKEL_MAX_PRIMS");
  if ((((uintptr_t)kp3d | (uintptr_t)K | (uintptr_t)T | (uintptr_t)scale_dev) & 7) || ((uintptr_t)records & 15) ||
      (((uintptr_t)jobs_dev | (uintptr_t)scores | (uintptr_t)sizes_dev | (uintptr_t)links_dev | (uintptr_t)colors_dev | (uintptr_t)counts |
        (uintptr_t)status) & 3))
    return dm4d_set_error(DM4D_ERR_ARG, "skeleton_plan_kp3d: misaligned pointer (fp64 tensors 8 bytes, records 16, the others 4)");
  if (!isfinite(low_thr) || !isfinite(high_thr) || !isfinite(thr_span) || !(thr_span > 0.0f))
    return dm4d_set_error(DM4D_ERR_ARG, "skeleton_plan_kp3d: the thresholds must be finite with high_thr above low_thr");
  for (int i = 0; i < n_maps; ++i) {
    if (jobs_host[2 * i] < 0 || jobs_host[2 * i] >= F || jobs_host[2 * i + 1] < 0 || jobs_host[2 * i + 1] >= m)
      return dm4d_set_error(DM4D_ERR_ARG, "skeleton_plan_kp3d: a job names a frame outside [0, F) or a camera outside [0, m)");
    if (!isfinite(scale_host[2 * i]) || !isfinite(scale_host[2 * i + 1]))
      return dm4d_set_error(DM4D_ERR_ARG, "skeleton_plan_kp3d: a map's scale ratio or offset is not finite");
    if (sizes_host[2 * i] < 0 || sizes_host[2 * i] > DM4D_SKEL_MAX_SIZE / 2 || sizes_host[2 * i + 1] < 1 || sizes_host[2 * i + 1] > DM4D_SKEL_MAX_SIZE / 2)
      return dm4d_set_error(DM4D_ERR_ARG, "skeleton_plan_kp3d: a thickness below 1, a negative radius, or a size above DM4D_SKEL_MAX_SIZE / 2");
  }
  for (int l = 0; l < L; ++l) {
    const int32_t* q = links_host + (int64_t)l * DM4D_SKEL_LINK_FIELDS;
    if (q[0] < 0 || q[0] >= k || q[1] < 0 || q[1] >= k) return dm4d_set_error(DM4D_ERR_ARG, "skeleton_plan_kp3d: a link joins a keypoint outside [0, k)");
    if (q[2] < 0 || q[2] >= L) return dm4d_set_error(DM4D_ERR_ARG, "skeleton_plan_kp3d: a link id lies outside [0, L)");
    if ((q[3] != 1 && q[3] != 2) || (q[4] != 1 && q[4] != 2))
      return dm4d_set_error(DM4D_ERR_ARG, "skeleton_plan_kp3d: a link's radius or thickness multiplier is neither 1 nor 2");
  }
  for (int64_t i = 0; i < (int64_t)k + L; ++i) {
    const float* c = colors_host + i * 4;
    for (int j = 0; j < 3; ++j)
      if (!(c[j] >= 0.0f && c[j] <= 255.0f)) return dm4d_set_error(DM4D_ERR_ARG, "skeleton_plan_kp3d: a colour channel lies outside [0, 255]");
    if (c[3] != 0.0f && c[3] != 1.0f) return dm4d_set_error(DM4D_ERR_ARG, "skeleton_plan_kp3d: a has-colour flag is neither 0 nor 1");
    if (i >= k && c[3] != 1.0f) return dm4d_set_error(DM4D_ERR_ARG, "skeleton_plan_kp3d: a link has no colour");
  }
  hipLaunchKernelGGL(skeleton_plan_kp3d_kernel, dim3((unsigned)n_maps), dim3(kPlanThreads), plan_lds_bytes(k, L), (hipStream_t)stream, kp3d, K, T,
                     jobs_dev, scores, scale_dev, sizes_dev, links_dev, colors_dev, k, L, low_thr, high_thr, thr_span, records, counts, status);
  return dm4d_check_launch("skeleton_plan_kp3d_kernel");
}
