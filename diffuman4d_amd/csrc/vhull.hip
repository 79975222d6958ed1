// Visual-hull carving (scripts/preprocess/carve_visual_hull.py:76-151): of a regular voxel grid keep the voxels whose projection
// falls on foreground in every view (or in at least min_views views), and write the kept centres in ascending voxel index.
//
// Per voxel idx (z fastest): X = (xs[ix], ys[iy], zs[iz]) widened to fp64; per view x_r = ((P[r][0] X0 + P[r][1] X1) + P[r][2] X2) +
// P[r][3] with every multiply and add rounded on its own; u = rint(x_0 / max(z, 1e-8)), v = rint(x_1 / max(z, 1e-8)) (ties to even);
// inside = z > 0 && 0 <= u < W && 0 <= v < H && mask[v][u].  The range is tested in floating point, so a huge or infinite quotient is
// never converted to an integer.
//
// One chunk of the grid = three launches on one stream, and the launch boundaries are the only ordering between blocks:
//   flags   one lane per voxel; one 64-bit ballot word per wave into a bit array, one count per block
//   scan    ONE block turns the block counts into exclusive offsets and advances the running total of the frame
//   gather  one lane per voxel again; a kept voxel goes to running total + block offset + popcount of the lower bits
// No atomic decides a position and no block waits for another one.  Every index that involves the voxel index or the number of
// kept points is 64-bit.
//
// Masks are read as bits (dm4d_vhull_pack_masks: rows of 32-bit words), 1/8 of the bytes of the bool masks: see DESIGN.md §4.
//
// Compiled with -ffp-contract=off (build.py EXTRA_FLAGS); the projection is written with the _rn intrinsics as well, so that no
// multiply-add is ever contracted.
#include <stdint.h>

#include "common.h"
#include "dm4d.h"
#include "errors.h"
#include "image_common.h"

namespace {

constexpr int kThreads = DM4D_VHULL_BLOCK;  // 4 waves
constexpr int kWaves = kThreads / 64;
constexpr int kScanThreads = 1024;
constexpr int64_t kHeaderBytes = 16;  // workspace: {int64 base of the chunk, spare} | bit words | block counts -> offsets

struct Grid {
  const float* xs;
  const float* ys;
  const float* zs;
  int64_t ny, nz;
};

__device__ __forceinline__ void voxel(const Grid& g, int64_t idx, float& x, float& y, float& z) {
  const int64_t q = idx / g.nz;
  z = g.zs[idx - q * g.nz];
  const int64_t ix = q / g.ny;
  y = g.ys[q - ix * g.ny];
  x = g.xs[ix];
}

// one row of P times (X, 1): ((p0 X0 + p1 X1) + p2 X2) + p3, five separately rounded operations
__device__ __forceinline__ double project_row(const double* p, double X0, double X1, double X2) {
  return __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(p[0], X0), __dmul_rn(p[1], X1)), __dmul_rn(p[2], X2)), p[3]);
}

// bits[b][y][w]: bit (x & 31) of word x >> 5 = masks[b][y][x] >= thr (1: nonzero); the tail bits of a row's last word are 0
__global__ void __launch_bounds__(kThreads) vhull_pack_kernel(const uint8_t* __restrict__ masks, uint32_t* __restrict__ bits, int64_t rows,
                                                              int W, int words, uint32_t thr) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= rows * words) return;
  const int64_t line = i / words;  // which (view, image row)
  const int x0 = (int)(i - line * words) * 32;
  const uint8_t* src = masks + line * W + x0;
  uint32_t v = 0;
  if ((W & 3) == 0 && x0 + 32 <= W) {  // rows start 4-byte aligned (the base is checked by the entry): eight 4-byte loads
    const uint32_t* src4 = reinterpret_cast<const uint32_t*>(src);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const uint32_t four = src4[q];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (((four >> (8 * j)) & 0xffu) >= thr) v |= 1u << (4 * q + j);
    }
  } else {
    for (int j = 0; j < 32 && x0 + j < W; ++j)
      if (src[j] >= thr) v |= 1u << j;
  }
  bits[i] = v;
}

__global__ void __launch_bounds__(kThreads) vhull_flags_kernel(Grid g, const double* __restrict__ P, const uint32_t* __restrict__ bits, int B,
                                                               int H, int W, int words, int need, int64_t first, int64_t n,
                                                               unsigned long long* __restrict__ keep_words, uint32_t* __restrict__ counts) {
  __shared__ uint32_t wave_count[kWaves];
  const int block = xcd_remap(blockIdx.x, gridDim.x);  // neighbouring voxels (= neighbouring mask pixels) share one XCD's L2
  const int64_t local = (int64_t)block * kThreads + threadIdx.x;
  const bool active = local < n;
  double X0 = 0.0, X1 = 0.0, X2 = 0.0;
  if (active) {
    float x, y, z;
    voxel(g, first + local, x, y, z);
    X0 = (double)x, X1 = (double)y, X2 = (double)z;
  }
  const double wd = (double)W, hd = (double)H;
  int count = 0;
  for (int b = 0; b < B; ++b) {
    // still open: `need` can be reached, and has not been reached yet (all-views mode is need = B: open while no view has missed)
    const bool open = active && count < need && count + (B - b) >= need;
    if (__ballot(open) == 0ull) break;
    // nested ifs only (no `continue`): every lane is back together at the ballot above
    if (open) {
      const double* p = P + (int64_t)b * 12;
      const double z = project_row(p + 8, X0, X1, X2);
      if (z > 0.0) {
        const double den = z < 1e-8 ? 1e-8 : z;
        const double u = rint(__ddiv_rn(project_row(p, X0, X1, X2), den));
        if (u >= 0.0 && u < wd) {
          const double v = rint(__ddiv_rn(project_row(p + 4, X0, X1, X2), den));
          if (v >= 0.0 && v < hd) {
            const int ui = (int)u, vi = (int)v;  // in [0, W) and [0, H) here
            const uint32_t word = bits[((int64_t)b * H + vi) * words + (ui >> 5)];
            count += (int)((word >> (ui & 31)) & 1u);
          }
        }
      }
    }
  }
  const unsigned long long kept = __ballot(active && count >= need);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    keep_words[(int64_t)block * kWaves + wave] = kept;
    wave_count[wave] = (uint32_t)__popcll(kept);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
    for (int w = 0; w < kWaves; ++w) s += wave_count[w];
    counts[block] = s;
  }
}

// ONE block: counts[i] -> sum of counts[0 .. i) in place; header[0] = points of the frame before this chunk, *total += the chunk's.
__global__ void __launch_bounds__(kScanThreads) vhull_scan_kernel(uint32_t* __restrict__ counts, int64_t nblocks, int64_t* __restrict__ header,
                                                                  int64_t* __restrict__ total) {
  const uint32_t sum = block_excl_scan_inplace<uint32_t, kScanThreads>(counts, nblocks);
  if (threadIdx.x == 0) {
    const int64_t base = *total;
    header[0] = base;
    *total = base + (int64_t)sum;
  }
}

__global__ void __launch_bounds__(kThreads) vhull_gather_kernel(Grid g, int64_t first, int64_t n, const unsigned long long* __restrict__ keep_words,
                                                                const uint32_t* __restrict__ offsets, const int64_t* __restrict__ header,
                                                                float* __restrict__ out, int64_t capacity) {
  const int64_t local = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long* words = keep_words + (int64_t)blockIdx.x * kWaves;
  const unsigned long long mine = words[wave];
  if (local >= n || !((mine >> lane) & 1ull)) return;
  int64_t pos = header[0] + (int64_t)offsets[blockIdx.x] + (int64_t)__popcll(mine & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) pos += (int64_t)__popcll(words[w]);
  if (pos >= capacity) return;  // the frame is carved again with room for *total points (host/vhull.py)
  float x, y, z;
  voxel(g, first + local, x, y, z);
  float* o = out + pos * 3;
  o[0] = x, o[1] = y, o[2] = z;
}

int64_t blocks_of(int64_t n) { return (n + kThreads - 1) / kThreads; }

}  // namespace

extern "C" int dm4d_vhull_pack_masks_u8(void* stream, const void* masks, void* bits, int B, int H, int W, int threshold) {
  if (threshold < 1 || threshold > 255) return dm4d_set_error(DM4D_ERR_ARG, "vhull_pack_masks: threshold outside 1..255");
  if (!masks || !bits) return dm4d_set_error(DM4D_ERR_ARG, "vhull_pack_masks: null pointer");
  if (B <= 0 || H <= 0 || W <= 0 || B > 65535 || H > (1 << 16) || W > (1 << 16))
    return dm4d_set_error(DM4D_ERR_ARG, "vhull_pack_masks: empty or oversized shape");
  if (((uintptr_t)masks | (uintptr_t)bits) & 3) return dm4d_set_error(DM4D_ERR_ARG, "vhull_pack_masks: masks and bits must be 4-byte aligned");
  const int words = (W + 31) / 32;
  const int64_t rows = (int64_t)B * H;
  const int64_t grid = (rows * words + kThreads - 1) / kThreads;
  if (grid > 0x7fffffffll) return dm4d_set_error(DM4D_ERR_ARG, "vhull_pack_masks: too many mask words for one launch");
  hipLaunchKernelGGL(vhull_pack_kernel, dim3((unsigned)grid), dim3(kThreads), 0, (hipStream_t)stream, (const uint8_t*)masks, (uint32_t*)bits,
                     rows, W, words, (uint32_t)threshold);
  return dm4d_check_launch("vhull_pack_kernel");
}

extern "C" int dm4d_vhull_pack_masks(void* stream, const void* masks, void* bits, int B, int H, int W) {
  return dm4d_vhull_pack_masks_u8(stream, masks, bits, B, H, W, 1);
}

extern "C" size_t dm4d_vhull_ws_bytes(int64_t n_voxels) {
  if (n_voxels <= 0 || n_voxels > DM4D_VHULL_MAX_CHUNK) return 0;
  return (size_t)(kHeaderBytes + blocks_of(n_voxels) * (kWaves * 8 + 4));
}

extern "C" int dm4d_vhull_carve_chunk(void* stream, const float* xs, const float* ys, const float* zs, int64_t nx, int64_t ny, int64_t nz,
                                      const double* P, const void* bits, int B, int H, int W, int min_views, int64_t first, int64_t n_voxels,
                                      void* workspace, int64_t workspace_bytes, int64_t* total, float* out, int64_t capacity) {
  if (!xs || !ys || !zs || !P || !bits || !workspace || !total || (!out && capacity > 0))
    return dm4d_set_error(DM4D_ERR_ARG, "vhull_carve_chunk: null pointer");
  if (nx <= 0 || ny <= 0 || nz <= 0 || nx > (1 << 20) || ny > (1 << 20) || nz > (1 << 20))
    return dm4d_set_error(DM4D_ERR_ARG, "vhull_carve_chunk: an axis is empty or longer than 2^20");
  if (B <= 0 || H <= 0 || W <= 0 || B > 65535 || H > (1 << 16) || W > (1 << 16))
    return dm4d_set_error(DM4D_ERR_ARG, "vhull_carve_chunk: empty or oversized mask shape");
  if (min_views < 0) return dm4d_set_error(DM4D_ERR_ARG, "vhull_carve_chunk: min_views must be 0 (all views) or positive");
  if (n_voxels <= 0 || n_voxels > DM4D_VHULL_MAX_CHUNK || first < 0 || first > nx * ny * nz - n_voxels)
    return dm4d_set_error(DM4D_ERR_ARG, "vhull_carve_chunk: the chunk is empty, too long or leaves the grid");
  if (capacity < 0 || workspace_bytes < (int64_t)dm4d_vhull_ws_bytes(n_voxels))
    return dm4d_set_error(DM4D_ERR_ARG, "vhull_carve_chunk: negative capacity or workspace too small");
  if (((uintptr_t)workspace | (uintptr_t)total | (uintptr_t)P) & 7)
    return dm4d_set_error(DM4D_ERR_ARG, "vhull_carve_chunk: workspace, total and P must be 8-byte aligned");
  const int64_t nb = blocks_of(n_voxels);
  int64_t* header = (int64_t*)workspace;
  unsigned long long* keep_words = (unsigned long long*)((char*)workspace + kHeaderBytes);
  uint32_t* counts = (uint32_t*)(keep_words + nb * kWaves);
  const Grid g{xs, ys, zs, ny, nz};
  const int need = min_views > 0 ? min_views : B;  // need > B keeps nothing, as the reference's count >= min_views
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(vhull_flags_kernel, dim3((unsigned)nb), dim3(kThreads), 0, st, g, P, (const uint32_t*)bits, B, H, W, (W + 31) / 32, need,
                     first, n_voxels, keep_words, counts);
  int rc = dm4d_check_launch("vhull_flags_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(vhull_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, counts, nb, header, total);
  rc = dm4d_check_launch("vhull_scan_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(vhull_gather_kernel, dim3((unsigned)nb), dim3(kThreads), 0, st, g, first, n_voxels, keep_words, counts, header, out, capacity);
  return dm4d_check_launch("vhull_gather_kernel");
}
