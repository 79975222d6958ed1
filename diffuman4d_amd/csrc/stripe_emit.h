// What the device encoders that cut their stream into stripes share (png.hip, webp.hip; the offsets and the host section also
// jpeg.hip and pngdec.hip): the run finder of the tokenisers, the bit-window emitter, the files' offsets, and the host's size checks.
// Each is called by every lane of one workgroup of THREADS lanes.  jpeg_emit_kernel has an emitter of its own: one wave per MCU,
// left-aligned symbols, bytes most significant bit first, the trailing bits taken from the next MCU's head.
// Integer arithmetic only; the one atomic is an LDS-local integer OR whose result does not depend on its order.
#pragma once
#include <stdint.h>

#include "image_common.h"

// -- run finder ---------------------------------------------------------------------------------------------------------------------------
// A lane's segment [a, b) of the n positions of a stripe, and the runs that reach over its ends: the run that reaches into the segment
// started at s_in, the one that leaves it ends at e_out (only the segment's first position can lie inside a run begun before it).
struct LaneRuns {
  int a, b, s_in, e_out;
};

// value(i): what stands at position i (an int), read once per position.  starts(prev, v): a run starts where v follows prev (position 0
// always starts one).  visit(i, v): the caller's own work on position i, in the same pass.  sh_first, sh_last: THREADS ints of LDS each.
// Ends after the __syncthreads() that publishes them and the two neighbour searches.
template <int THREADS, typename Value, typename Starts, typename Visit>
__device__ __forceinline__ LaneRuns lane_runs(int n, int* sh_first, int* sh_last, Value value, Starts starts, Visit visit) {
  const int tid = threadIdx.x;
  const int L = (n + THREADS - 1) / THREADS;
  LaneRuns r;
  r.a = min(tid * L, n), r.b = min(r.a + L, n);
  int first = n, last = -1;  // the first and the last run start in the segment
  int prev = r.a > 0 && r.a < r.b ? value(r.a - 1) : 0;
  for (int i = r.a; i < r.b; ++i) {
    const int v = value(i);
    if (i == 0 || starts(prev, v)) {
      if (first == n) first = i;
      last = i;
    }
    visit(i, v);
    prev = v;
  }
  sh_first[tid] = first, sh_last[tid] = last;
  __syncthreads();
  r.s_in = 0, r.e_out = n;
  for (int u = tid - 1; u >= 0; --u)
    if (sh_last[u] >= 0) {
      r.s_in = sh_last[u];
      break;
    }
  for (int u = tid + 1; u < THREADS; ++u)
    if (sh_first[u] < n) {
      r.e_out = sh_first[u];
      break;
    }
  return r;
}

// -- bit-window emitter -------------------------------------------------------------------------------------------------------------------
// The `count` positions of a stripe to bits, least significant bit first, PER positions per lane and round: token(q, v, nb) gives the
// bits of position q (V v of nb bits; nb == 0, as on entry: none), and is called for every position of a round, so it must give none
// for q >= count (the callers read "no token" there: one chain of tests, no branch of its own); they are OR-ed into the LDS window win[WIN_WORDS] at positions from a
// prefix sum (wave_tot: THREADS / 64 words of LDS); store(i, byte) takes whole byte i of the stripe's output, and the unfinished byte is
// carried into the next round.  WIN_WORDS covers 7 + THREADS x PER tokens of the most bits, and two words of slack.
// On entry win[] is zero except for the carry_bits low bits of win[0], and all lanes have passed a __syncthreads() since it was written.
// On return win[0] holds the unfinished byte, carry_bits its bit count, done the bytes handed to store.
template <int THREADS, int PER, int WIN_WORDS, typename V, typename Token, typename Store>
__device__ __forceinline__ void emit_window(int count, uint32_t* win, uint32_t* wave_tot, int& carry_bits, uint64_t& done, Token token,
                                            Store store) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int base = 0; base < count; base += THREADS * PER) {
    V v[PER];
    int nb[PER];
    int tot = 0;
    const int q0 = base + tid * PER;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      v[k] = 0, nb[k] = 0;
      token(q0 + k, v[k], nb[k]);
      tot += nb[k];
    }
    const int incl = wave_incl_scan(tot);
    if (lane == 63) wave_tot[wave] = (uint32_t)incl;
    __syncthreads();
    int pos = carry_bits + incl - tot, T = carry_bits;
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) {
      if (w < wave) pos += (int)wave_tot[w];
      T += (int)wave_tot[w];
    }
#pragma unroll
    for (int k = 0; k < PER; ++k)
      if (nb[k]) {
        const int i = pos >> 5, sh = pos & 31;
        atomicOr(&win[i], (uint32_t)(v[k] << sh));
        if (sh + nb[k] > 32) atomicOr(&win[i + 1], (uint32_t)(v[k] >> (32 - sh)));
        if constexpr (sizeof(V) > 4)
          if (sh + nb[k] > 64) atomicOr(&win[i + 2], (uint32_t)(v[k] >> (64 - sh)));
        pos += nb[k];
      }
    __syncthreads();
    const uint32_t nbytes = (uint32_t)T >> 3;
    for (uint32_t i = tid; i < nbytes; i += THREADS) store(done + i, (win[i >> 2] >> (8 * (i & 3))) & 0xffu);
    const uint32_t carry = (T & 7) ? (win[nbytes >> 2] >> (8 * (nbytes & 3))) & 0xffu : 0u;
    __syncthreads();
    for (int i = tid; i < WIN_WORDS; i += THREADS) win[i] = i == 0 ? carry : 0u;
    __syncthreads();
    done += nbytes, carry_bits = T & 7;
  }
}

// -- the files' places in the blob ----------------------------------------------------------------------------------------------------------
// offs[i] = sum of lens[0 .. i), ONE block
template <int THREADS>
__device__ __forceinline__ void offsets_block(const int64_t* __restrict__ lens, int64_t* __restrict__ offs, int n) {
  for (int i = threadIdx.x; i < n; i += THREADS) offs[i] = lens[i];
  __syncthreads();
  block_excl_scan_inplace<int64_t, THREADS>(offs, n);
}

// -- host ---------------------------------------------------------------------------------------------------------------------------------
inline int64_t pad16(int64_t v) { return (v + 15) / 16 * 16; }

// the h rows of `row` bytes, `stride` apart, that start at `off` lie inside a buffer of `bytes`
inline bool plane_ok(int64_t off, int64_t stride, int64_t h, int64_t row, int64_t bytes) {
  return off >= 0 && stride >= row && stride <= (1ll << 32) && off <= bytes && (h - 1) * stride + row <= bytes - off;
}
