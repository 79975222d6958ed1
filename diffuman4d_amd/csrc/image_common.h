// The parts that the uint8 image kernels share (capture.hip, jpeg.hip, skeleton.hip, pose.hip, detect.hip, vhull.hip), each defined once:
//   Pillow resample   the fixed-point rule of libImaging/Resample.c and the host-side check of a coefficient table
//   pixel box         the bounding box of the set pixels of a uint8 plane: the walk, the wave reduction and the block fold; and the
//                     writing of a plane that is a filled rectangle
//   scan              the 64-lane inclusive scan and the one-block exclusive scan with a carry
//   composite         Pillow's MULDIV255, the per-byte rule of Image.composite over black (pose.hip, detect.hip)
// Integer code only, so -ffp-contract=off (build.py EXTRA_FLAGS gives it to some of the including files) cannot change what this
// header compiles to.  Everything assumes one-dimensional blocks (lane = threadIdx.x & 63).
#pragma once
#include <stdint.h>

#include "common.h"

// -- composite ------------------------------------------------------------------------------------------------------------------------------
// Image.composite(image, black, mask) for an L mask: Pillow's MULDIV255
__device__ __forceinline__ uint32_t muldiv255(uint32_t p, uint32_t m) {
  const uint32_t t = p * m + 128u;
  return ((t >> 8) + t) >> 8;
}

// -- Pillow resample --------------------------------------------------------------------------------------------------------------------
// int32 coefficients with 22 fractional bits; every output value is clip8((2^21 + sum u * k) >> 22)
constexpr int kPillowBits = 22;
constexpr int32_t kPillowHalf = 1 << (kPillowBits - 1);  // where every sum starts: the rounding

__device__ __forceinline__ uint32_t clip8(int32_t v) {
  if (v >= (1 << kPillowBits << 8)) return 255u;
  if (v <= 0) return 0u;
  return (uint32_t)(v >> kPillowBits);
}

// The two sources of a 3-channel window: tap t of packed words r | g << 8 | b << 16, `stride` words apart, ...
struct PackedRgb {
  const uint32_t* p;
  int stride;
  __device__ __forceinline__ void operator()(int t, uint32_t (&c)[3]) const {
    const uint32_t v = p[t * stride];
    c[0] = v & 0xffu, c[1] = (v >> 8) & 0xffu, c[2] = (v >> 16) & 0xffu;
  }
};
// ... or of byte triples, `stride` bytes apart
struct ByteRgb {
  const uint8_t* p;
  int64_t stride;
  __device__ __forceinline__ void operator()(int t, uint32_t (&c)[3]) const {
    const uint8_t* q = p + t * stride;
    c[0] = q[0], c[1] = q[1], c[2] = q[2];
  }
};

// one output pixel: the window's `cnt` taps weighted by k[0 .. cnt), rounded and clipped per channel
template <typename Src>
__device__ __forceinline__ void pillow_rgb(const Src& src, const int32_t* __restrict__ k, int cnt, uint32_t (&out)[3]) {
  int32_t a0 = kPillowHalf, a1 = kPillowHalf, a2 = kPillowHalf;
  for (int t = 0; t < cnt; ++t) {
    uint32_t c[3];
    src(t, c);
    const int32_t wt = k[t];
    a0 += (int32_t)c[0] * wt;
    a1 += (int32_t)c[1] * wt;
    a2 += (int32_t)c[2] * wt;
  }
  out[0] = clip8(a0), out[1] = clip8(a1), out[2] = clip8(a2);
}

// Host-side check of one coefficient table at tab[off ..): `n` windows {start, length} then n x ksize weights inside tab_len, every
// window inside [0, in_size) and at most ksize long; `ordered`: starts and ends do not decrease either
inline bool pillow_table_ok(const int32_t* tab, int64_t tab_len, int64_t off, int64_t ksize, int64_t ksize_max, int64_t n, int64_t in_size,
                            bool ordered) {
  if (off < 0 || ksize < 1 || ksize > ksize_max || off > tab_len || n * (2 + ksize) > tab_len - off) return false;
  int64_t prev_start = 0, prev_end = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t start = tab[off + 2 * i], cnt = tab[off + 2 * i + 1];
    if (start < 0 || cnt < 1 || cnt > ksize || start + cnt > in_size) return false;
    if (ordered && (start < prev_start || start + cnt < prev_end)) return false;
    prev_start = start;
    prev_end = start + cnt;
  }
  return true;
}

// -- pixel box ----------------------------------------------------------------------------------------------------------------------------
// {first column, first row, last column, last row}; empty = {w, h, -1, -1}.  min and max of integers: no atomics
struct Box {
  int fc, fr, lc, lr;
};

__device__ __forceinline__ void box_merge(Box& b, const Box& o) {
  b.fc = min(b.fc, o.fc);
  b.fr = min(b.fr, o.fr);
  b.lc = max(b.lc, o.lc);
  b.lr = max(b.lr, o.lr);
}

// the set bytes (byte & MASK) among the `count` bytes of `word` (little endian) that start at byte `at` of the plane
template <int BPP, uint32_t MASK>
__device__ __forceinline__ void box_scan_word(Box& b, uint32_t word, int count, int64_t at, int row_bytes) {
  if ((word & MASK) == 0) return;
  int row = (int)(at / row_bytes), cb = (int)(at % row_bytes);
  for (int j = 0; j < count; ++j) {
    if ((word >> (8 * j)) & (MASK & 0xffu)) box_merge(b, Box{cb / BPP, row, cb / BPP, row});
    if (++cb == row_bytes) {
      cb = 0;
      ++row;
    }
  }
}

// One thread's share of a plane of BPP bytes per pixel, a pixel being set when one of its bytes has a bit of MASK: the 16-byte vectors
// first_vec, first_vec + vec_stride, ... between a scalar head of up to 15 bytes before the first aligned address and a tail of up to
// 15 after the last vector (a byte per thread, where do_head_tail).  A vector with no set byte costs one load and one test.
template <int BPP, uint32_t MASK>
__device__ __forceinline__ void box_scan_plane(const uint8_t* __restrict__ src, int64_t total_bytes, int row_bytes, int64_t first_vec,
                                               int64_t vec_stride, bool do_head_tail, Box& b) {
  int64_t head = (16 - (int64_t)((uintptr_t)src & 15)) & 15;
  if (head > total_bytes) head = total_bytes;
  const int64_t nvec = (total_bytes - head) / 16;
  for (int64_t v = first_vec; v < nvec; v += vec_stride) {
    const int64_t at = head + v * 16;
    const U4 q = ldg16(src + at);
    if (((q.x | q.y | q.z | q.w) & MASK) == 0) continue;
    box_scan_word<BPP, MASK>(b, q.x, 4, at, row_bytes);
    box_scan_word<BPP, MASK>(b, q.y, 4, at + 4, row_bytes);
    box_scan_word<BPP, MASK>(b, q.z, 4, at + 8, row_bytes);
    box_scan_word<BPP, MASK>(b, q.w, 4, at + 12, row_bytes);
  }
  if (do_head_tail) {
    const int tid = threadIdx.x;
    if (tid < head) box_scan_word<BPP, MASK>(b, src[tid], 1, tid, row_bytes);
    const int64_t t = head + nvec * 16 + tid;
    if (t < total_bytes) box_scan_word<BPP, MASK>(b, src[t], 1, t, row_bytes);
  }
}

// every lane gets the box of its wave
__device__ __forceinline__ void box_wave_reduce(Box& b) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const Box o{__shfl_xor(b.fc, off), __shfl_xor(b.fr, off), __shfl_xor(b.lc, off), __shfl_xor(b.lr, off)};
    box_merge(b, o);
  }
}

// thread 0 gets the box of its block of THREADS: shuffles reduce a wave, LDS the block
template <int THREADS>
__device__ __forceinline__ void box_block_reduce(Box& b) {
  __shared__ int s_box[THREADS / 64][4];
  const int tid = threadIdx.x;
  box_wave_reduce(b);
  if ((tid & 63) == 0) {
    int* s = s_box[tid >> 6];
    s[0] = b.fc, s[1] = b.fr, s[2] = b.lc, s[3] = b.lr;
  }
  __syncthreads();
  if (tid == 0)
    for (int k = 1; k < THREADS / 64; ++k) box_merge(b, Box{s_box[k][0], s_box[k][1], s_box[k][2], s_box[k][3]});
}

// One thread's share of writing a [h, w] plane that is 255 on rows r0 .. r1 - 1 and columns c0 .. c1 - 1 and 0 elsewhere: the 16-byte
// vectors first_vec, first_vec + vec_stride, ... between a scalar head and tail as in box_scan_plane (a byte per thread, where
// do_head_tail).  Every byte of the plane is written, none outside it.
__device__ __forceinline__ void rect_fill_plane(uint8_t* __restrict__ dst, int h, int w, int c0, int r0, int c1, int r1, int64_t first_vec,
                                                int64_t vec_stride, bool do_head_tail) {
  const int64_t total = (int64_t)h * w;
  int64_t head = (16 - (int64_t)((uintptr_t)dst & 15)) & 15;
  if (head > total) head = total;
  const int64_t nvec = (total - head) / 16;
  const int64_t tail0 = head + nvec * 16;
  auto value = [&](int row, int col) -> uint32_t { return (row >= r0 && row < r1 && col >= c0 && col < c1) ? 255u : 0u; };
  for (int64_t v = first_vec; v < nvec; v += vec_stride) {
    const int64_t at = head + v * 16;
    int row = (int)(at / w), col = (int)(at % w);
    uint32_t q[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      uint32_t word = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        word |= value(row, col) << (8 * j);
        if (++col == w) {
          col = 0;
          ++row;
        }
      }
      q[k] = word;
    }
    stg16(dst + at, U4{q[0], q[1], q[2], q[3]});
  }
  if (do_head_tail) {
    const int tid = threadIdx.x;
    if (tid < head) dst[tid] = (uint8_t)value((int)(tid / w), (int)(tid % w));
    const int64_t t = tail0 + tid;
    if (t < total) dst[t] = (uint8_t)value((int)(t / w), (int)(t % w));
  }
}

// -- scan ---------------------------------------------------------------------------------------------------------------------------------
// inclusive prefix sum of v over the 64 lanes of a wave
template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const T o = __shfl_up(v, off);
    if (lane >= off) v += o;
  }
  return v;
}

// One block of THREADS: a[0 .. cnt) -> exclusive prefix sums in place, THREADS values a round with a carry between rounds; returns
// the total to every thread.
template <typename T, int THREADS>
__device__ T block_excl_scan_inplace(T* __restrict__ a, int64_t cnt) {
  __shared__ T wave_sum[THREADS / 64];
  __shared__ T carry_s;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  for (int64_t t0 = 0; t0 < cnt; t0 += THREADS) {
    const int64_t i = t0 + threadIdx.x;
    const T c = i < cnt ? a[i] : (T)0;
    const T s = wave_incl_scan(c);
    if (lane == 63) wave_sum[wave] = s;
    __syncthreads();
    T before = carry_s;
    for (int w = 0; w < wave; ++w) before += wave_sum[w];
    if (i < cnt) a[i] = before + s - c;
    __syncthreads();
    if (threadIdx.x == THREADS - 1) carry_s = before + s;
    __syncthreads();
  }
  return carry_s;
}
