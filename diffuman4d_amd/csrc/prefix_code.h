// Length-limited canonical prefix codes built by one workgroup, and a one-lane bit writer: what the device encoders of deflate (png.hip)
// and of VP8L (webp.hip) share in building their codes.  The rule is tests/png_model.py's code_lengths / canonical.  Their run finder
// and the emitter that puts the codes into the stream are in stripe_emit.h.  Integer arithmetic; the one atomic is an LDS-local integer
// add whose result does not depend on its order.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

constexpr int kPrefixThreads = 256;  // lanes of the calling workgroup
constexpr int kPrefixMaxSyms = 288;  // the largest alphabet

struct HuffScratch {
  uint32_t w[kPrefixMaxSyms], nw[kPrefixMaxSyms];
  uint16_t order[kPrefixMaxSyms], pl[kPrefixMaxSyms], pn[kPrefixMaxSyms], dn[kPrefixMaxSyms];
  int n, maxd;
};

// Code lengths of the counts f[0 .. nsym) by the model's rule (png_model.code_lengths); f is halved where the limit asks for it.
// Called by every lane of the workgroup; lens[] is complete after the caller's next __syncthreads().
__device__ inline void build_lengths(uint32_t* f, int nsym, int limit, uint8_t* lens, HuffScratch& sc) {
  const int tid = threadIdx.x;
  for (;;) {
    if (tid == 0) sc.n = 0, sc.maxd = 0;
    __syncthreads();
    for (int sym = tid; sym < nsym; sym += kPrefixThreads) {
      const uint32_t fi = f[sym];
      lens[sym] = 0;
      if (fi) {  // rank among the used symbols by (count, symbol)
        int rank = 0;
        for (int j = 0; j < nsym; ++j) {
          const uint32_t fj = f[j];
          rank += (fj != 0 && (fj < fi || (fj == fi && j < sym))) ? 1 : 0;
        }
        sc.order[rank] = (uint16_t)sym, sc.w[rank] = fi;
        atomicAdd(&sc.n, 1);
      }
    }
    __syncthreads();
    if (tid == 0) {
      const int n = sc.n;
      int maxd = 0;
      if (n == 1) {
        lens[sc.order[0]] = 1, maxd = 1;
      } else if (n >= 2) {
        int li = 0, ni = 0;
        for (int k = 0; k < n - 1; ++k) {  // two queues: sorted leaves, nodes in order of creation; the leaf on a tie
          uint32_t wt = 0;
          for (int c = 0; c < 2; ++c) {
            if (li < n && (ni >= k || sc.w[li] <= sc.nw[ni])) {
              sc.pl[li] = (uint16_t)k, wt += sc.w[li], ++li;
            } else {
              sc.pn[ni] = (uint16_t)k, wt += sc.nw[ni], ++ni;
            }
          }
          sc.nw[k] = wt;
        }
        sc.dn[n - 2] = 0;
        for (int k = n - 3; k >= 0; --k) sc.dn[k] = (uint16_t)(sc.dn[sc.pn[k]] + 1);
        for (int i = 0; i < n; ++i) {
          const int d = sc.dn[sc.pl[i]] + 1;
          lens[sc.order[i]] = (uint8_t)d;
          maxd = max(maxd, d);
        }
      }
      sc.maxd = maxd;
    }
    __syncthreads();
    const bool done = sc.maxd <= limit;
    __syncthreads();
    if (done) return;
    for (int sym = tid; sym < nsym; sym += kPrefixThreads) {
      const uint32_t v = f[sym];
      f[sym] = v ? (v + 1) >> 1 : 0;
    }
  }
}

// canonical codes of lens[0 .. nsym) as they enter the stream: out[sym] = length << 16 | bit-reversed code (0 = unused).  One lane.
__device__ inline void canonical_codes(const uint8_t* lens, int nsym, uint32_t* out) {
  uint32_t count[17], next[17];
  for (int b = 0; b < 17; ++b) count[b] = 0;
  for (int s = 0; s < nsym; ++s) ++count[lens[s]];
  count[0] = 0;
  uint32_t code = 0;
  next[0] = 0;
  for (int b = 1; b < 17; ++b) {
    code = (code + count[b - 1]) << 1;
    next[b] = code;
  }
  for (int s = 0; s < nsym; ++s) {
    const int l = lens[s];
    out[s] = l ? ((uint32_t)l << 16) | (__brev(next[l]++) >> (32 - l)) : 0u;
  }
}

struct BitOut {  // one lane appends to zeroed words, least significant bit first
  uint32_t* w;
  int pos;
  __device__ __forceinline__ void put(uint32_t v, int nb) {
    const int i = pos >> 5, sh = pos & 31;
    w[i] |= v << sh;
    if (sh + nb > 32) w[i + 1] |= v >> (32 - sh);
    pos += nb;
  }
};
