// HBM-bound normalisation kernels for gfx950: GroupNorm(+SiLU) over NHWC (two-source channel concat fused in), LayerNorm, and the
// row softmaxes, in all three precisions.
//   * fast kernels (gn_stats / gn_apply / gn_resident, ln_kernel, softmax_rows*): statistics in fp32, all global traffic in vectors
//     of eight channels; bf16 in and out (fast precision), or fp32 / fp16 in and one fp16 plane out (precision "fp16")
//   * general kernels (gn32_*, ln32_kernel, softmax32_split_kernel): fp32 in, any channel count, GroupNorm statistics in fp64; the
//     two-term operand out (precision "parity") or one fp16 plane (what the fp16 entries fall back to).  None of these is tuned.
#include "common.h"
#include "dm4d.h"
#include "errors.h"

namespace {

constexpr int GN_THREADS = 256;
constexpr int GN_MAXC = 4096;

__host__ __device__ inline int gn_nchunk(int B, int HW) {
  int n = (2048 + B - 1) / B;
  int cap = (HW + 15) / 16;
  if (n > cap) n = cap;
  if (n < 1) n = 1;
  return n;
}

// What a tensor element is on the way in: eight channels ("a vector") as they sit in memory, as eight floats, and one channel alone.
struct In16 {
  typedef u16 in_t;
  typedef U4 raw_t;  // 16 bytes
  static __device__ __forceinline__ raw_t ldraw(const u16* p) { return ldg16(p); }
};
struct InBF16 : In16 {
  static __device__ __forceinline__ void unpack(const raw_t& r, float* v) { unpack8(r, v); }
  static __device__ __forceinline__ float ld1(const u16* p) { return bf2f(*p); }
};
struct InF16 : In16 {  // an activation a convolution left in fp16: conv1 of a resnet, whose only reader is norm2
  static __device__ __forceinline__ void unpack(const raw_t& r, float* v) { unpack8h(r, v); }
  static __device__ __forceinline__ float ld1(const u16* p) { return h2f(*p); }
};
struct InF32 {
  typedef float in_t;
  struct raw_t {  // 32 bytes
    f32x4_t a, b;
  };
  static __device__ __forceinline__ raw_t ldraw(const float* p) {
    raw_t r;
    r.a = *reinterpret_cast<const f32x4_t*>(p);
    r.b = *reinterpret_cast<const f32x4_t*>(p + 4);
    return r;
  }
  static __device__ __forceinline__ void unpack(const raw_t& r, float* v) {
    v[0] = r.a[0]; v[1] = r.a[1]; v[2] = r.a[2]; v[3] = r.a[3];
    v[4] = r.b[0]; v[5] = r.b[1]; v[6] = r.b[2]; v[7] = r.b[3];
  }
  static __device__ __forceinline__ float ld1(const float* p) { return *p; }
};

// What the result is on the way out, W = 1, 4 or 8 consecutive channels per store: st<W>(p, lo, v) writes v[0..W-1] at p (a second
// plane, where there is one, `lo` elements behind it).  gamma / beta come in the output's 16-bit format: par() one, par8() eight.
struct OutBF16 {  // one bf16 plane
  static constexpr int PLANES = 1;
  static __device__ __forceinline__ void par8(const u16* p, float* v) { unpack8(ldg16(p), v); }
  template <int W>
  static __device__ __forceinline__ void st(u16* p, int64_t, const float* v) {
    static_assert(W == 8, "whole vectors only");
    stg16(p, pack8(v));
  }
};
struct OutF16 {  // one fp16 plane, saturating
  static constexpr int PLANES = 1;
  static __device__ __forceinline__ float par(u16 v) { return h2f(v); }
  static __device__ __forceinline__ void par8(const u16* p, float* v) { unpack8h(ldg16(p), v); }
  template <int W>
  static __device__ __forceinline__ void st(u16* p, int64_t, const float* v) {
    if constexpr (W == 8) {
      stg16(p, pack8h_sat(v));
    } else if constexpr (W == 4) {
      uint2 ph;
      ph.x = pack_h2(sat_h(v[0]), sat_h(v[1])), ph.y = pack_h2(sat_h(v[2]), sat_h(v[3]));
      *reinterpret_cast<uint2*>(p) = ph;
    } else {
      *p = f2h_sat(v[0]);
    }
  }
};
struct OutSplit {  // the two-term bf16 operand [hi | lo]
  static constexpr int PLANES = 2;
  static __device__ __forceinline__ float par(u16 v) { return bf2f(v); }
  template <int W>
  static __device__ __forceinline__ void st(u16* p, int64_t lo_off, const float* v) {
    static_assert(W == 1 || W == 4, "one or four channels");
    u16 hi[W], lo[W];
#pragma unroll
    for (int e = 0; e < W; ++e) split2(v[e], hi[e], lo[e]);
    if constexpr (W == 4) {
      uint2 ph, pl;
      ph.x = (uint32_t)hi[0] | ((uint32_t)hi[1] << 16), ph.y = (uint32_t)hi[2] | ((uint32_t)hi[3] << 16);
      pl.x = (uint32_t)lo[0] | ((uint32_t)lo[1] << 16), pl.y = (uint32_t)lo[2] | ((uint32_t)lo[3] << 16);
      *reinterpret_cast<uint2*>(p) = ph;
      *reinterpret_cast<uint2*>(p + lo_off) = pl;
    } else {
      p[0] = hi[0];
      p[lo_off] = lo[0];
    }
  }
};

// IO (template parameter of the fast GroupNorm / LayerNorm kernels): the three combinations of the traits above that they are built for
//   0  bf16 in, bf16 out, bf16 gamma / beta                    (fast precision)
//   2  fp32 in, ONE fp16 plane out, fp16 gamma / beta          (precision "fp16": dm4d_groupnorm_nhwc_f32_f16 / dm4d_layernorm_f32_f16)
//   3  fp16 in, ONE fp16 plane out, fp16 gamma / beta          (precision "fp16": dm4d_groupnorm_nhwc_f16_f16, GroupNorm only)
template <class In, class Out>
struct NormPair {
  typedef In in;
  typedef Out out;
  typedef typename In::in_t in_t;
};
template <int IO>
struct NormIO;
template <>
struct NormIO<0> : NormPair<InBF16, OutBF16> {};
template <>
struct NormIO<2> : NormPair<InF32, OutF16> {};
template <>
struct NormIO<3> : NormPair<InF16, OutF16> {};

struct GNParams {
  const void* X1;  // the input trait's in_t
  const void* X2;
  int C1, C2, B, HW, groups, nchunk;
  float eps;
  const u16* gamma;
  const u16* beta;
  u16* Y;  // [B*HW, PLANES * C]
  int silu;
  void* ws;  // [B][nchunk][groups][2], float (fast kernels) or double (gn32_*)
  // IO = 2 only: a second output, the UN-normalised input rounded to fp16 ([B*HW, C], the channel concat of X1 | X2) -- the operand of a
  // resnet's 1x1 shortcut convolution, which reads the same tensor as its first GroupNorm (unet_multiview_blocks.py:667, resnet.py)
  u16* Yraw;
};

// the workgroup's sample and chunk of the two-launch kernels, and the chunk's pixels [p0, p1)
struct GNSpan {
  int b, chunk, p0, p1;
};
__device__ __forceinline__ GNSpan gn_span(const GNParams& p) {
  const int b = blockIdx.x / p.nchunk, chunk = blockIdx.x % p.nchunk;
  const int per = (p.HW + p.nchunk - 1) / p.nchunk;
  const int p0 = chunk * per;
  return {b, chunk, p0, min(p0 + per, p.HW)};
}

// channel c of the concat [X1 | X2] in sample b: where it sits at pixel 0, and the pixel stride of its source
template <class T>
struct GNSrc {
  const T* src;
  int ld;
};
template <class T>
__device__ __forceinline__ GNSrc<T> gn_src(const GNParams& p, int b, int c) {
  if (c < p.C1) return {static_cast<const T*>(p.X1) + (int64_t)b * p.HW * p.C1 + c, p.C1};
  return {static_cast<const T*>(p.X2) + (int64_t)b * p.HW * p.C2 + (c - p.C1), p.C2};
}

// the partial sums of (sample b, chunk k, group g)
template <class Acc>
__device__ __forceinline__ Acc* gn_ws(const GNParams& p, int b, int k, int g) {
  return static_cast<Acc*>(p.ws) + (((int64_t)b * p.nchunk + k) * p.groups + g) * 2;
}

// end of a statistics pass: sm [PPB][C][2] holds every thread's sum / sum of squares; one thread per group adds them up in a fixed order
template <class Acc>
__device__ __forceinline__ void gn_store_partials(const Acc* sm, const GNParams& p, const GNSpan& sp, int C, int PPB) {
  const int gs = C / p.groups;
  for (int g = threadIdx.x; g < p.groups; g += GN_THREADS) {
    Acc s = 0, q = 0;
    for (int r = 0; r < PPB; ++r)
      for (int c = g * gs; c < (g + 1) * gs; ++c) {
        s += sm[(r * C + c) * 2 + 0];
        q += sm[(r * C + c) * 2 + 1];
      }
    Acc* w = gn_ws<Acc>(p, sp.b, sp.chunk, g);
    w[0] = s;
    w[1] = q;
  }
}

// (sum, sum of squares, count) of a group -> its mean and 1 / sqrt(variance + eps), the variance clamped at zero.  Acc = float: the
// sums are of shifted values (below) and the caller adds the shift to the mean.
template <class Acc>
__device__ __forceinline__ void gn_finish(Acc s, Acc q, Acc n, float eps, float& mean, float& rstd) {
  const Acc m = s / n;
  Acc var = q / n - m * m;
  var = var < (Acc)0 ? (Acc)0 : var;
  mean = (float)m;
  if constexpr (sizeof(Acc) == sizeof(float)) rstd = rsqrtf(var + eps);
  else rstd = (float)(1.0 / sqrt(var + (double)eps));
}

// Shifted statistics.  Sum / sum of squares are taken of (x - s_g), s_g = the sample's value at pixel 0 in the first channel
// of group g (any value near the group's data would do; this one costs one 2-byte load): mean = s_g + S / n and
// var = Q / n - (S / n)^2 then cancel at the scale of the group's SPREAD, not of its mean -- with raw sums a group whose mean
// is 200 standard deviations loses 15 of fp32's 24 bits (1e-2 relative error on the output; 3e-4 at 50).  All channels of a
// group share the shift, so partial sums of different threads, chunks and kernels add up exactly as before.
template <class In>
__device__ __forceinline__ float gn_shift(const GNParams& p, int b, int g, int gs) {
  return In::ld1(gn_src<typename In::in_t>(p, b, g * gs).src);  // first channel of the group, in the concatenated channel axis
}
// the shifts of the eight channels of vector cv: groups of eight or more channels put at most two groups in a vector
template <class In>
__device__ __forceinline__ void gn_shift8(const GNParams& p, int b, int cv, int gs, float (&sh)[8]) {
  const int g0 = (cv * 8) / gs, g1 = (cv * 8 + 7) / gs;
  if (g1 - g0 <= 1) {
    const float s0 = gn_shift<In>(p, b, g0, gs), s1 = g1 != g0 ? gn_shift<In>(p, b, g1, gs) : s0;
#pragma unroll
    for (int e = 0; e < 8; ++e) sh[e] = (cv * 8 + e) / gs == g0 ? s0 : s1;
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) sh[e] = gn_shift<In>(p, b, (cv * 8 + e) / gs, gs);
  }
}

// One loaded vector into the sums of its eight channels.  FMA: q += d * d with one rounding (fmaf), or with two (contraction off).
// Spelled out because every output bit depends on it and the compiler, left to choose, chose by the code around it: two roundings in
// gn_stats_kernel, one in gn_resident_kernel -- except fp32 in at 16 pixels per thread, two again.  tests/test_norm_bits_gpu.py holds
// those bits, so the three choices are written down where they are made.  (The two-rounding form is called through a lambda at both
// places, as the parent wrote its loop body: profiles/norm_family_codegen.md has the register counts of either way.)
template <class In, bool FMA>
__device__ __forceinline__ void gn_add8(const typename In::raw_t& r, const float (&sh)[8], float (&s)[8], float (&q)[8]) {
#pragma clang fp contract(off)
  float v[8];
  In::unpack(r, v);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float d = v[e] - sh[e];
    s[e] += d;
    q[e] = FMA ? fmaf(d, d, q[e]) : q[e] + d * d;
  }
}

// one loaded vector out, at pixel px of rows of C channels behind dst: y = x * a + sft, optional SiLU (and, IO = 2 with dst_raw, x itself in fp16)
template <int IO>
__device__ __forceinline__ void gn_put8(const typename NormIO<IO>::in::raw_t& r, const float (&a)[8], const float (&sft)[8], int silu, u16* dst,
                                        u16* dst_raw, int px, int C) {
  const int64_t off = (int64_t)px * C;
  typedef typename NormIO<IO>::out out;
  float v[8];
  NormIO<IO>::in::unpack(r, v);
  if constexpr (IO == 2) {
    if (dst_raw) out::template st<8>(dst_raw + off, 0, v);
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float y = v[e] * a[e] + sft[e];
    v[e] = silu ? silu_f(y) : y;
  }
  out::template st<8>(dst + off, 0, v);
}

// pass 1: per (batch, pixel chunk) partial sum / sum of squares of every group, fixed summation order
template <int IO = 0>
__global__ __launch_bounds__(GN_THREADS) void gn_stats_kernel(GNParams p) {
  typedef typename NormIO<IO>::in in;
  typedef typename in::in_t in_t;
  typedef typename in::raw_t raw_t;
  extern __shared__ __attribute__((aligned(16))) float sm[];  // [PPB][C][2]
  const int C = p.C1 + p.C2, CV = C / 8;
  const GNSpan sp = gn_span(p);
  const int PPB = CV >= GN_THREADS ? 1 : GN_THREADS / CV;  // pixels processed per pass
  const int tid = threadIdx.x;

  for (int slot = tid; slot < CV * PPB; slot += GN_THREADS) {
    const int cv = slot % CV, prow = slot / CV;
    float s[8], q[8], sh[8];
    gn_shift8<in>(p, sp.b, cv, C / p.groups, sh);
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] = q[e] = 0.f;
    const GNSrc<in_t> x = gn_src<in_t>(p, sp.b, cv * 8);
    // two loads in flight per thread (a chunk is only a few passes long: one load per pass leaves the kernel waiting on a
    // memory round trip per pass; four cost 92 registers and three of the eight resident workgroups); the sums still run
    // pixel by pixel in ascending order
    auto add = [&](const raw_t& r) { gn_add8<in, false>(r, sh, s, q); };
    int px = sp.p0 + prow;
#pragma nounroll
    for (; px + PPB < sp.p1; px += 2 * PPB) {
      const in_t* a = x.src + (int64_t)px * x.ld;
      const raw_t r0 = in::ldraw(a), r1 = in::ldraw(a + (int64_t)PPB * x.ld);
      add(r0);
      add(r1);
    }
    for (; px < sp.p1; px += PPB) add(in::ldraw(x.src + (int64_t)px * x.ld));
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      sm[(prow * C + cv * 8 + e) * 2 + 0] = s[e];
      sm[(prow * C + cv * 8 + e) * 2 + 1] = q[e];
    }
  }
  __syncthreads();
  gn_store_partials<float>(sm, p, sp, C, PPB);
}

// pass 2: y = (x - mean) * rstd * gamma + beta, optional SiLU; writes the concatenated tensor
template <int IO = 0>
__global__ __launch_bounds__(GN_THREADS) void gn_apply_kernel(GNParams p) {
  typedef typename NormIO<IO>::in in;
  typedef typename in::in_t in_t;
  typedef typename in::raw_t raw_t;
  extern __shared__ __attribute__((aligned(16))) float sm[];  // reduction scratch, then mean[g], rstd[g]
  const int C = p.C1 + p.C2, CV = C / 8;
  float* sc = sm;  // reduction scratch
  float* mean = sm + (2 * C > 2 * GN_THREADS ? 2 * C : 2 * GN_THREADS);  // first part: reduction scratch
  float* rstd = mean + p.groups;
  const GNSpan sp = gn_span(p);
  const int b = sp.b, tid = threadIdx.x;
  const int gs = C / p.groups;
  // reduce the per-chunk partials: all 256 threads fetch (fixed association order => deterministic), then one
  // thread per group combines the GN_THREADS/groups slices -- the serial 64-deep loop this replaces was the
  // latency floor of the kernel
  const int slices = GN_THREADS / p.groups > 0 ? GN_THREADS / p.groups : 1;
  {
    const int g = tid % p.groups, sl = tid / p.groups;
    float s = 0.f, q = 0.f;
    if (sl < slices) {
      for (int k = sl; k < p.nchunk; k += slices) {
        const float* w = gn_ws<float>(p, b, k, g);
        s += w[0];
        q += w[1];
      }
      sc[(sl * p.groups + g) * 2 + 0] = s;  // 2*slices*groups <= 2*GN_THREADS floats
      sc[(sl * p.groups + g) * 2 + 1] = q;
    }
    __syncthreads();
  }
  for (int g = tid; g < p.groups; g += GN_THREADS) {
    float s = 0.f, q = 0.f;
    for (int sl = 0; sl < slices; ++sl) {
      s += sc[(sl * p.groups + g) * 2 + 0];
      q += sc[(sl * p.groups + g) * 2 + 1];
    }
    float dm;  // mean of (x - shift)
    gn_finish<float>(s, q, (float)gs * (float)p.HW, p.eps, dm, rstd[g]);
    mean[g] = gn_shift<in>(p, b, g, gs) + dm;
  }
  __syncthreads();
  // A thread keeps one 8-channel vector (its scale / shift in registers) and walks the chunk's pixels: no index
  // division and no LDS traffic in the streaming loop; 256 threads cover GN_THREADS / CV consecutive pixels per pass.
  const int PPB = CV >= GN_THREADS ? 1 : GN_THREADS / CV;
  for (int slot = tid; slot < CV * PPB; slot += GN_THREADS) {
    const int cv = slot % CV, prow = slot / CV;
    float a[8], sft[8];
    {
      float gm[8], bt[8];
      NormIO<IO>::out::par8(p.gamma + cv * 8, gm);
      NormIO<IO>::out::par8(p.beta + cv * 8, bt);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int g = (cv * 8 + e) / gs;
        a[e] = gm[e] * rstd[g];
        sft[e] = bt[e] - mean[g] * a[e];
      }
    }
    const GNSrc<in_t> x = gn_src<in_t>(p, b, cv * 8);
    u16* dst = p.Y + (int64_t)b * p.HW * C + cv * 8;
    u16* dst_raw = (IO == 2 && p.Yraw) ? p.Yraw + (int64_t)b * p.HW * C + cv * 8 : nullptr;
    auto put = [&](const raw_t& r, int px) { gn_put8<IO>(r, a, sft, p.silu, dst, dst_raw, px, C); };
    int px = sp.p0 + prow;
#pragma nounroll
    for (; px + 3 * PPB < sp.p1; px += 4 * PPB) {  // four loads in flight per thread, as in the statistics pass
      const in_t* s0 = x.src + (int64_t)px * x.ld;
      const raw_t r0 = in::ldraw(s0), r1 = in::ldraw(s0 + (int64_t)PPB * x.ld), r2 = in::ldraw(s0 + (int64_t)2 * PPB * x.ld), r3 = in::ldraw(s0 + (int64_t)3 * PPB * x.ld);
      put(r0, px);
      put(r1, px + PPB);
      put(r2, px + 2 * PPB);
      put(r3, px + 3 * PPB);
    }
    for (; px < sp.p1; px += PPB) put(in::ldraw(x.src + (int64_t)px * x.ld), px);
  }
}

// Single-launch GroupNorm for feature maps small enough to stay in registers between the statistics and the apply step
// (levels 1-3 of the UNet at 72x40 latents): one workgroup owns (sample, slab of `gps` whole groups), every thread
// keeps one 16-byte channel vector of up to NV pixels in VGPRs, so X is read from HBM exactly once and the second
// launch (with its dependent-launch gap) disappears.  Same fp32 sum / sum-of-squares formulas as the two-pass kernels;
// the summation order is fixed by (HW, C, groups) only, never by the batch.
constexpr int GN_RES_MAXGPS = 8;

template <int NV, int IO = 0>
__global__ __launch_bounds__(GN_THREADS) void gn_resident_kernel(GNParams p, int gps, int SV, int PPB, int NS, int xcd_map) {
  typedef typename NormIO<IO>::in in;
  typedef typename in::in_t in_t;
  typedef typename in::raw_t raw_t;
  __shared__ float sm[2 * 8 * GN_THREADS];  // [PPB][SC][2]
  __shared__ float sm2[2 * GN_THREADS];     // [PARTS][SC][2]
  __shared__ float stat[2 * GN_RES_MAXGPS];
  const int C = p.C1 + p.C2, gs = C / p.groups, SC = SV * 8;
  int b, slab;
  if (xcd_map) {  // workgroup i runs on XCD i % 8: keep all slabs of a sample on one XCD so that the 128-byte lines
    const int x = blockIdx.x & 7, j = blockIdx.x >> 3;  // two slabs share are fetched into ONE L2
    b = x + 8 * (j / NS);
    slab = j % NS;
  } else {
    b = blockIdx.x / NS;
    slab = blockIdx.x % NS;
  }
  const int tid = threadIdx.x, sv = tid % SV, prow = tid / SV;
  const bool active = prow < PPB;
  const int cv = slab * gps * gs / 8 + sv;  // vector index in the concatenated channel axis
  const GNSrc<in_t> x = gn_src<in_t>(p, b, cv * 8);
  raw_t r[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int px = prow + k * PPB;
    if (active && px < p.HW) r[k] = in::ldraw(x.src + (int64_t)px * x.ld);
  }
  {
    float s[8], q[8], sh[8];
    gn_shift8<in>(p, b, cv, gs, sh);
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] = q[e] = 0.f;
    auto add2 = [&](const raw_t& rr) { gn_add8<in, false>(rr, sh, s, q); };
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int px = prow + k * PPB;
      if (active && px < p.HW) {
        if constexpr (NV == 16 && IO == 2) add2(r[k]);  // (see gn_add8)
        else gn_add8<in, true>(r[k], sh, s, q);
      }
    }
    if (active) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        sm[(prow * SC + sv * 8 + e) * 2 + 0] = s[e];
        sm[(prow * SC + sv * 8 + e) * 2 + 1] = q[e];
      }
    }
  }
  __syncthreads();
  {
    const int PARTS = GN_THREADS / SC, c = tid % SC, part = tid / SC;
    if (part < PARTS) {
      float s = 0.f, q = 0.f;
      for (int rr = part; rr < PPB; rr += PARTS) {
        s += sm[(rr * SC + c) * 2 + 0];
        q += sm[(rr * SC + c) * 2 + 1];
      }
      sm2[(part * SC + c) * 2 + 0] = s;
      sm2[(part * SC + c) * 2 + 1] = q;
    }
    __syncthreads();
    // one WAVE per group: the PARTS x gs partials of a group are summed 64 at a time and folded with a butterfly.  (This
    // was one THREAD per group walking up to 6 x 80 LDS entries serially -- ~10 us of latency in a kernel that moves a few
    // KB at the 18x10 and 9x5 levels.)  The order depends on (HW, C, groups) only, never on the batch.
    const int wv = tid >> 6, ln = tid & 63;
    for (int g = wv; g < gps; g += GN_THREADS / 64) {
      float s = 0.f, q = 0.f;
      for (int e = ln; e < PARTS * gs; e += 64) {
        const int pt = e / gs, cc = g * gs + (e - pt * gs);
        s += sm2[(pt * SC + cc) * 2 + 0];
        q += sm2[(pt * SC + cc) * 2 + 1];
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        s += __shfl_xor(s, off);
        q += __shfl_xor(q, off);
      }
      if (ln == 0) {
        float dm;  // mean of (x - shift)
        gn_finish<float>(s, q, (float)gs * (float)p.HW, p.eps, dm, stat[g * 2 + 1]);
        stat[g * 2 + 0] = gn_shift<in>(p, b, slab * gps + g, gs) + dm;
      }
    }
  }
  __syncthreads();
  if (!active) return;
  float a[8], sft[8];
  {
    float gm[8], bt[8];
    NormIO<IO>::out::par8(p.gamma + cv * 8, gm);
    NormIO<IO>::out::par8(p.beta + cv * 8, bt);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int g = (sv * 8 + e) / gs;
      a[e] = gm[e] * stat[g * 2 + 1];
      sft[e] = bt[e] - stat[g * 2 + 0] * a[e];
    }
  }
  u16* dst = p.Y + (int64_t)b * p.HW * C + cv * 8;
  u16* dst_raw = (IO == 2 && p.Yraw) ? p.Yraw + (int64_t)b * p.HW * C + cv * 8 : nullptr;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int px = prow + k * PPB;
    if (px < p.HW) gn_put8<IO>(r[k], a, sft, p.silu, dst, dst_raw, px, C);
  }
}

int g_gn_resident = 1;  // tuning hook (dm4d_tune_set_groupnorm_resident)

// slab geometry of the single-launch kernel, or false when the map does not fit in registers (two-pass path then)
bool gn_resident_plan(int C, int HW, int groups, int* gps, int* SV, int* PPB, int* NV) {
  const int gs = C / groups;
  for (int g = 1; g <= GN_RES_MAXGPS && g <= groups; g *= 2) {
    if (groups % g || (g * gs) % 8 || g * gs * 2 < 64) continue;
    const int sv = g * gs / 8;
    if (sv > 32) return false;
    const int ppb = GN_THREADS / sv, nv = (HW + ppb - 1) / ppb;
    if (nv > 16) return false;
    *gps = g, *SV = sv, *PPB = ppb, *NV = nv;
    return true;
  }
  return false;
}

// The general GroupNorm (+SiLU): fp32 NHWC in, any channel count, W = 1 or 4 channels per thread (4: 16-byte loads, 8-byte stores of
// each plane -- what every layer of the UNet and the VAE runs in the parity precision, C1 and C2 multiples of 4; with one channel per
// thread a C = 320 layer kept a quarter of the block idle in its second sweep and moved 2 bytes per store instruction: 1.15 TB/s
// over a step, round 4 bench).  The same two passes as above with the sums in fp64: no shift trick needed.  PPB comes from C / W, so
// the two widths sum in different orders: their statistics differ by fp64 rounding.
template <int W>
__device__ __forceinline__ void ld_f32(const float* p, float (&v)[W]) {
  if constexpr (W == 4) {
    const f32x4_t r = *reinterpret_cast<const f32x4_t*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = r[e];
  } else {
    static_assert(W == 1, "one or four channels");
    v[0] = *p;
  }
}

template <int W>
__global__ __launch_bounds__(GN_THREADS) void gn32_stats_kernel(GNParams p) {
  extern __shared__ __attribute__((aligned(16))) double smd[];  // [PPB][C][2]
  const int C = p.C1 + p.C2, Q = C / W;
  const GNSpan sp = gn_span(p);
  const int PPB = Q >= GN_THREADS ? 1 : GN_THREADS / Q;
  for (int slot = threadIdx.x; slot < Q * PPB; slot += GN_THREADS) {
    const int c = (slot % Q) * W, prow = slot / Q;
    const GNSrc<float> x = gn_src<float>(p, sp.b, c);
    double s[W], q[W];
#pragma unroll
    for (int e = 0; e < W; ++e) s[e] = q[e] = 0.0;
    for (int px = sp.p0 + prow; px < sp.p1; px += PPB) {
      float v[W];
      ld_f32<W>(x.src + (int64_t)px * x.ld, v);
#pragma unroll
      for (int e = 0; e < W; ++e) {
        const double d = (double)v[e];
        s[e] += d;
        q[e] += d * d;
      }
    }
#pragma unroll
    for (int e = 0; e < W; ++e) {
      smd[(prow * C + c + e) * 2 + 0] = s[e];
      smd[(prow * C + c + e) * 2 + 1] = q[e];
    }
  }
  __syncthreads();
  gn_store_partials<double>(smd, p, sp, C, PPB);
}

template <int W, class Out>
__global__ __launch_bounds__(GN_THREADS) void gn32_apply_kernel(GNParams p) {
  extern __shared__ __attribute__((aligned(16))) float smf[];  // mean[groups], rstd[groups]
  const int C = p.C1 + p.C2, Q = C / W;
  float* mean = smf;
  float* rstd = smf + p.groups;
  const GNSpan sp = gn_span(p);
  const int tid = threadIdx.x;
  const int gs = C / p.groups;
  for (int g = tid; g < p.groups; g += GN_THREADS) {
    double s = 0.0, q = 0.0;
    for (int k = 0; k < p.nchunk; ++k) {
      const double* w = gn_ws<double>(p, sp.b, k, g);
      s += w[0];
      q += w[1];
    }
    gn_finish<double>(s, q, (double)gs * (double)p.HW, p.eps, mean[g], rstd[g]);
  }
  __syncthreads();
  const int PPB = Q >= GN_THREADS ? 1 : GN_THREADS / Q;
  constexpr int PL = Out::PLANES;
  for (int slot = tid; slot < Q * PPB; slot += GN_THREADS) {
    const int c = (slot % Q) * W, prow = slot / Q;
    float mu[W], a[W], bt[W];
#pragma unroll
    for (int e = 0; e < W; ++e) {
      const int g = (c + e) / gs;
      mu[e] = mean[g];
      a[e] = rstd[g] * Out::par(p.gamma[c + e]);
      bt[e] = Out::par(p.beta[c + e]);
    }
    const GNSrc<float> x = gn_src<float>(p, sp.b, c);
    u16* dst = p.Y + (int64_t)sp.b * p.HW * (PL * C) + c;
    for (int px = sp.p0 + prow; px < sp.p1; px += PPB) {
      float v[W], y[W];
      ld_f32<W>(x.src + (int64_t)px * x.ld, v);
#pragma unroll
      for (int e = 0; e < W; ++e) {
        float t = (v[e] - mu[e]) * a[e] + bt[e];
        if (p.silu) t = silu_f(t);
        y[e] = t;
      }
      Out::template st<W>(dst + (int64_t)px * (PL * C), C, y);
    }
  }
}

// LayerNorm: one wave per row, row kept in registers (two-pass mean / variance)
template <int NV, int IO = 0>  // eight-channel vectors per lane
__global__ __launch_bounds__(256) void ln_kernel(const typename NormIO<IO>::in_t* X, int64_t ldx, const u16* gamma, const u16* beta, u16* Y,
                                                 int64_t ldy, int M, int C, float eps) {
  typedef typename NormIO<IO>::in in;
  typedef typename NormIO<IO>::out out;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + wave;
  if (row >= M) return;
  const int CV = C / 8;
  float v[NV][8];
  bool on[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int cv = lane + 64 * i;
    on[i] = cv < CV;
    if (on[i]) {
      in::unpack(in::ldraw(X + (int64_t)row * ldx + cv * 8), v[i]);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[i][e] = 0.f;
    }
  }
  float mu, rs;
  ln_row_stats<NV>(v, on, C, eps, mu, rs);
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int cv = lane + 64 * i;
    if (on[i]) {
      float g[8], bt[8], y[8];
      out::par8(gamma + cv * 8, g);
      out::par8(beta + cv * 8, bt);
      ln_row_apply(v[i], mu, rs, g, bt, y);
      out::template st<8>(Y + (int64_t)row * ldy + cv * 8, 0, y);
    }
  }
}

// The general LayerNorm: fp32 rows of any length in, one wave per row, two-pass statistics in fp32, one channel per lane and step
template <class Out>
__global__ __launch_bounds__(256) void ln32_kernel(const float* X, int64_t ldx, const u16* gamma, const u16* beta, u16* Y, int64_t ldy,
                                                   int M, int C, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const float* x = X + (int64_t)row * ldx;
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += x[c];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  const float mu = s / (float)C;
  float q = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float d = x[c] - mu;
    q += d * d;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) q += __shfl_xor(q, off);
  const float rs = rsqrtf(q / (float)C + eps);
  u16* y = Y + (int64_t)row * ldy;
  for (int c = lane; c < C; c += 64) {
    const float v = (x[c] - mu) * rs * Out::par(gamma[c]) + Out::par(beta[c]);
    Out::template st<1>(y + c, C, &v);
  }
}

// Row softmax, one workgroup of four waves per row.  A value per thread -> the four waves' maxima / sums, through red[4], in wave
// order on every thread.  The maximum of four is the same however it is associated; the SUMS are handed back one by one because the
// kernels below do not add them alike (softmax_rows_kernel left to right, the fp32-logit kernels pairwise) and their bits are kept.
struct Wave4 {
  float w[4];
};
template <bool MAX>
__device__ __forceinline__ Wave4 block_reduce4(float v, float* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = MAX ? fmaxf(v, __shfl_xor(v, off)) : v + __shfl_xor(v, off);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return {red[0], red[1], red[2], red[3]};
}
__device__ __forceinline__ float block_max(float v, float* red) {
  const Wave4 m = block_reduce4<true>(v, red);
  return fmaxf(fmaxf(m.w[0], m.w[1]), fmaxf(m.w[2], m.w[3]));
}

// row softmax over N columns: P = softmax(S * scale); one workgroup per row
__global__ __launch_bounds__(256) void softmax_rows_kernel(const u16* S, int64_t lds, u16* P, int64_t ldp, int N,
                                                           float scale) {
  __shared__ float red[8];
  const int row = blockIdx.x, tid = threadIdx.x;
  const u16* s = S + (int64_t)row * lds;
  u16* o = P + (int64_t)row * ldp;
  float mx = -1e30f;
  for (int i = tid; i < N; i += 256) mx = fmaxf(mx, bf2f(s[i]));
  mx = block_max(mx, red);
  float sum = 0.f;
  const float c = scale * 1.4426950408889634f;
  for (int i = tid; i < N; i += 256) sum += __builtin_amdgcn_exp2f((bf2f(s[i]) - mx) * c);
  const Wave4 t = block_reduce4<false>(sum, red + 4);
  sum = t.w[0] + t.w[1] + t.w[2] + t.w[3];
  const float inv = 1.0f / sum;
  for (int i = tid; i < N; i += 256) o[i] = f2bf(__builtin_amdgcn_exp2f((bf2f(s[i]) - mx) * c) * inv);
}

// the same for fp32 logits (VAE mid-block attention, d = 512: SDPA keeps its logits in fp32; rounding them to bf16 first
// costs up to 2^-9 * |logit| in the exponent).  Rows are read as float4 (16-byte aligned rows: lds % 4 == 0) with a scalar
// tail of N % 4 columns (threads 0..2), so a row may be LONGER than N: the caller pads the key axis to the GEMM's K
// granularity and the columns behind N are neither read nor written.  The second and third pass of a row hit L2.
__global__ __launch_bounds__(256) void softmax_rows_f32_kernel(const float* S, int64_t lds, u16* P, int64_t ldp, int N,
                                                               float scale) {
  __shared__ float red[8];
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* srow = S + (int64_t)row * lds;
  u16* prow = P + (int64_t)row * ldp;
  const f32x4_t* s = reinterpret_cast<const f32x4_t*>(srow);
  uint2* o = reinterpret_cast<uint2*>(prow);
  const int n4 = N >> 2;
  const bool tail = tid < (N & 3);  // this thread also owns column 4 n4 + tid
  const float st = tail ? srow[4 * n4 + tid] : 0.f;
  float mx = tail ? st : -3.0e38f;
  for (int i = tid; i < n4; i += 256) {
    const f32x4_t v = s[i];
    mx = fmaxf(fmaxf(mx, fmaxf(v[0], v[1])), fmaxf(v[2], v[3]));
  }
  mx = block_max(mx, red);
  const float c = scale * 1.4426950408889634f;
  const float mc = mx * c;
  const float et = tail ? __builtin_amdgcn_exp2f(fmaf(st, c, -mc)) : 0.f;
  float sum = 0.f;
  for (int i = tid; i < n4; i += 256) {
    const f32x4_t v = s[i];
    sum += (__builtin_amdgcn_exp2f(fmaf(v[0], c, -mc)) + __builtin_amdgcn_exp2f(fmaf(v[1], c, -mc))) +
           (__builtin_amdgcn_exp2f(fmaf(v[2], c, -mc)) + __builtin_amdgcn_exp2f(fmaf(v[3], c, -mc)));
  }
  sum += et;  // (after the vector part: rows with N % 4 == 0 sum exactly as before)
  const Wave4 t = block_reduce4<false>(sum, red + 4);
  sum = (t.w[0] + t.w[1]) + (t.w[2] + t.w[3]);
  const float inv = 1.0f / sum;
  for (int i = tid; i < n4; i += 256) {
    const f32x4_t v = s[i];
    uint2 w;
    w.x = pack_bf2(__builtin_amdgcn_exp2f(fmaf(v[0], c, -mc)) * inv, __builtin_amdgcn_exp2f(fmaf(v[1], c, -mc)) * inv);
    w.y = pack_bf2(__builtin_amdgcn_exp2f(fmaf(v[2], c, -mc)) * inv, __builtin_amdgcn_exp2f(fmaf(v[3], c, -mc)) * inv);
    o[i] = w;
  }
  if (tail) prow[4 * n4 + tid] = f2bf(et * inv);
}

// P = softmax(S * scale) per row of fp32 logits -> [p_hi | p_lo | p_hi], each plane Np wide (columns N..Np-1 zero): the three-plane
// operand of the VAE mid block, where both factors of q k^T and of p v are activations, so each product takes three terms
// hi hi + lo hi + hi lo.  H16: one fp16 plane [M, Np] (plain rounding: a probability cannot overflow).
template <bool H16>
__global__ __launch_bounds__(256) void softmax32_split_kernel(const float* S, int64_t lds, u16* P, int64_t ldp, int M, int N, int Np,
                                                              float scale) {
  __shared__ float red[8];
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* s = S + (int64_t)row * lds;
  float mx = -3.0e38f;
  for (int c = tid; c < N; c += 256) mx = fmaxf(mx, s[c]);
  mx = block_max(mx, red);
  float sum = 0.f;
  for (int c = tid; c < N; c += 256) sum += expf((s[c] - mx) * scale);
  const Wave4 t = block_reduce4<false>(sum, red + 4);
  sum = (t.w[0] + t.w[1]) + (t.w[2] + t.w[3]);
  const float inv = 1.0f / sum;
  u16* y = P + (int64_t)row * ldp;
  for (int c = tid; c < Np; c += 256) {
    if constexpr (H16) {
      y[c] = c < N ? f2h(expf((s[c] - mx) * scale) * inv) : (u16)0;
    } else {
      u16 hi = 0, lo = 0;
      if (c < N) split2(expf((s[c] - mx) * scale) * inv, hi, lo);
      y[c] = hi;
      y[Np + c] = lo;
      y[2 * Np + c] = hi;
    }
  }
}

// dm4d_groupnorm_plan_batch: the batch this thread's GroupNorm launches plan their statistics chunks for (0 = each launch's own)
thread_local int t_gn_plan_batch = 0;
inline int gn_plan_nchunk(int B, int HW) { return gn_nchunk(t_gn_plan_batch > B ? t_gn_plan_batch : B, HW); }

}  // namespace

extern "C" int dm4d_groupnorm_plan_batch(int B) {
  if (B < 0) return dm4d_set_error(DM4D_ERR_ARG, "groupnorm_plan_batch: negative batch");
  t_gn_plan_batch = B;
  return DM4D_OK;
}

extern "C" size_t dm4d_groupnorm_ws_bytes(int B, int HW, int groups) {
  return (size_t)B * gn_nchunk(B, HW) * groups * 2 * sizeof(float);
}

extern "C" size_t dm4d_groupnorm_f32_ws_bytes(int B, int HW, int groups) {
  return (size_t)B * gn_nchunk(B, HW) * groups * 2 * sizeof(double);
}

template <int IO>
static int groupnorm_impl(void* stream, const void* X1, int C1, const void* X2, int C2, int B, int HW, int groups, float eps,
                          const void* gamma, const void* beta, void* Y, int apply_silu, void* ws, void* Yraw = nullptr) {
  if (!X1 || !gamma || !beta || !Y || !ws || B <= 0 || HW <= 0 || groups <= 0)
    return dm4d_set_error(DM4D_ERR_ARG, "groupnorm: null pointer or empty shape");
  if (!X2) C2 = 0;
  const int C = C1 + C2;
  if ((C1 & 7) || (C2 & 7) || C % groups != 0 || C > GN_MAXC)
    return dm4d_set_error(DM4D_ERR_ARG, "groupnorm: channels must be multiples of 8, divisible by groups, <= 4096");
  GNParams p{X1, X2, C1, C2, B, HW, groups, gn_plan_nchunk(B, HW), eps, (const u16*)gamma, (const u16*)beta, (u16*)Y, apply_silu, ws, (u16*)Yraw};
  hipStream_t st = (hipStream_t)stream;
  {
    int gps, SV, RPB, NV;
    if (g_gn_resident && gn_resident_plan(C, HW, groups, &gps, &SV, &RPB, &NV)) {
      const int NS = groups / gps, xcd = (B % 8 == 0);
      const dim3 grid(B * NS), blk(GN_THREADS);
      if (NV <= 2) hipLaunchKernelGGL((gn_resident_kernel<2, IO>), grid, blk, 0, st, p, gps, SV, RPB, NS, xcd);
      else if (NV <= 4) hipLaunchKernelGGL((gn_resident_kernel<4, IO>), grid, blk, 0, st, p, gps, SV, RPB, NS, xcd);
      else if (NV <= 8) hipLaunchKernelGGL((gn_resident_kernel<8, IO>), grid, blk, 0, st, p, gps, SV, RPB, NS, xcd);
      else hipLaunchKernelGGL((gn_resident_kernel<16, IO>), grid, blk, 0, st, p, gps, SV, RPB, NS, xcd);
      return dm4d_check_launch("gn_resident_kernel");
    }
  }
  const int CV = C / 8;
  const int PPB = CV >= GN_THREADS ? 1 : GN_THREADS / CV;
  const size_t sm1 = (size_t)PPB * C * 2 * sizeof(float);
  const size_t sm2 = ((size_t)(2 * C > 2 * GN_THREADS ? 2 * C : 2 * GN_THREADS) + 2 * groups) * sizeof(float);
  hipLaunchKernelGGL(gn_stats_kernel<IO>, dim3(B * p.nchunk), dim3(GN_THREADS), sm1, st, p);
  int rc = dm4d_check_launch("gn_stats_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(gn_apply_kernel<IO>, dim3(B * p.nchunk), dim3(GN_THREADS), sm2, st, p);
  return dm4d_check_launch("gn_apply_kernel");
}

// The statistics pass keeps PPB * C pairs of doubles in LDS, PPB = pixels per pass.  With C <= GN_MAXC = 4096 that always fits in 64 KiB:
//   Q = C / W >= 256 gives PPB = 1 and 16 C <= 65536 bytes;  Q < 256 gives PPB * Q <= 256, so PPB * C <= 1024 pairs = 16 KiB.
template <int W, class Out>
static int gn32_launch(const GNParams& p, hipStream_t st) {
  const int C = p.C1 + p.C2, Q = C / W, PPB = Q >= GN_THREADS ? 1 : GN_THREADS / Q;
  const size_t sm1 = (size_t)PPB * C * 2 * sizeof(double);
  hipLaunchKernelGGL(gn32_stats_kernel<W>, dim3(p.B * p.nchunk), dim3(GN_THREADS), sm1, st, p);
  // (the four-wide pair keeps the labels its launches had as kernels of their own: error messages are part of the ABI's behaviour)
  int rc = dm4d_check_launch(W == 4 ? "gn32_stats4_kernel" : "gn32_stats_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL((gn32_apply_kernel<W, Out>), dim3(p.B * p.nchunk), dim3(GN_THREADS), 2 * p.groups * sizeof(float), st, p);
  return dm4d_check_launch(W == 4 ? "gn32_apply4_kernel" : "gn32_apply_kernel");
}

template <class Out>
static int groupnorm_f32_impl(void* stream, const float* X1, int C1, const float* X2, int C2, int B, int HW, int groups, float eps,
                              const void* gamma, const void* beta, void* Y, int apply_silu, void* ws) {
  if (!X1 || !gamma || !beta || !Y || !ws || B <= 0 || HW <= 0 || groups <= 0 || C1 <= 0 || C2 < 0 || (C2 > 0 && !X2))
    return dm4d_set_error(DM4D_ERR_ARG, "groupnorm_f32: bad arguments");
  const int C = C1 + C2;
  if (C % groups != 0 || C > GN_MAXC) return dm4d_set_error(DM4D_ERR_ARG, "groupnorm_f32: channels must divide into groups and be <= 4096");
  GNParams p{X1, X2, C1, C2, B, HW, groups, gn_plan_nchunk(B, HW), eps, (const u16*)gamma, (const u16*)beta, (u16*)Y, apply_silu, ws, nullptr};
  const bool vec4 = C1 % 4 == 0 && C2 % 4 == 0 && ((uintptr_t)X1 & 15) == 0 && (C2 == 0 || ((uintptr_t)X2 & 15) == 0) && ((uintptr_t)Y & 7) == 0;
  return vec4 ? gn32_launch<4, Out>(p, (hipStream_t)stream) : gn32_launch<1, Out>(p, (hipStream_t)stream);
}

extern "C" int dm4d_groupnorm_nhwc_bf16(void* stream, const void* X1, int C1, const void* X2, int C2, int B, int HW,
                                        int groups, float eps, const void* gamma, const void* beta, void* Y,
                                        int apply_silu, void* ws) {
  return groupnorm_impl<0>(stream, X1, C1, X2, C2, B, HW, groups, eps, gamma, beta, Y, apply_silu, ws);
}

// precision "parity": fp32 NHWC in, fp64 statistics, the two-term operand [B*HW, 2 C] out
extern "C" int dm4d_groupnorm_nhwc_f32_split(void* stream, const float* X1, int C1, const float* X2, int C2, int B, int HW,
                                             int groups, float eps, const void* gamma, const void* beta, void* Y, int apply_silu,
                                             void* ws) {
  return groupnorm_f32_impl<OutSplit>(stream, X1, C1, X2, C2, B, HW, groups, eps, gamma, beta, Y, apply_silu, ws);
}

extern "C" int dm4d_groupnorm_f32_f16_general(void* stream, const float* X1, int C1, const float* X2, int C2, int B, int HW, int groups,
                                              float eps, const void* gamma, const void* beta, void* Y, int apply_silu, void* ws) {
  return groupnorm_f32_impl<OutF16>(stream, X1, C1, X2, C2, B, HW, groups, eps, gamma, beta, Y, apply_silu, ws);
}

// precision "fp16": fp32 NHWC in (shifted fp32 statistics as above), one fp16 plane out.  Channel counts that are not multiples
// of 8 take the general kernels (fp64 statistics, one / four channels per thread).
extern "C" int dm4d_groupnorm_nhwc_f32_f16(void* stream, const float* X1, int C1, const float* X2, int C2, int B, int HW, int groups,
                                           float eps, const void* gamma, const void* beta, void* Y, int apply_silu, void* ws) {
  if (!X2) C2 = 0;
  if ((C1 & 7) || (C2 & 7) || (((uintptr_t)X1) & 15) || (X2 && (((uintptr_t)X2) & 15)) || (((uintptr_t)Y) & 15))
    return dm4d_groupnorm_f32_f16_general(stream, X1, C1, X2, C2, B, HW, groups, eps, gamma, beta, Y, apply_silu, ws);
  return groupnorm_impl<2>(stream, X1, C1, X2, C2, B, HW, groups, eps, gamma, beta, Y, apply_silu, ws);
}

// precision "fp16", fp16 in: the input is an activation its producer already rounded to fp16 (same statistics, same output rounding;
// half the bytes of the fp32 form on the way in).  Channel counts must be multiples of 8, tensors 16-byte aligned.
extern "C" int dm4d_groupnorm_nhwc_f16_f16(void* stream, const void* X1, int C1, const void* X2, int C2, int B, int HW, int groups,
                                           float eps, const void* gamma, const void* beta, void* Y, int apply_silu, void* ws) {
  if (!X2) C2 = 0;
  if ((C1 & 7) || (C2 & 7) || (((uintptr_t)X1) & 15) || (X2 && (((uintptr_t)X2) & 15)) || (((uintptr_t)Y) & 15))
    return dm4d_set_error(DM4D_ERR_ARG, "groupnorm_f16_f16: channel counts must be multiples of 8, tensors 16-byte aligned");
  return groupnorm_impl<3>(stream, X1, C1, X2, C2, B, HW, groups, eps, gamma, beta, Y, apply_silu, ws);
}

extern "C" int dm4d_groupnorm_nhwc_f32_f16_raw(void* stream, const float* X1, int C1, const float* X2, int C2, int B, int HW, int groups,
                                               float eps, const void* gamma, const void* beta, void* Y, void* Yraw, int apply_silu,
                                               void* ws) {
  if (!X2) C2 = 0;
  if (!Yraw || (C1 & 7) || (C2 & 7) || (((uintptr_t)X1) & 15) || (X2 && (((uintptr_t)X2) & 15)) || ((((uintptr_t)Y) | ((uintptr_t)Yraw)) & 15))
    return dm4d_set_error(DM4D_ERR_ARG, "groupnorm_f32_f16_raw: needs Yraw, channel counts that are multiples of 8 and 16-byte aligned tensors");
  return groupnorm_impl<2>(stream, X1, C1, X2, C2, B, HW, groups, eps, gamma, beta, Y, apply_silu, ws, Yraw);
}

template <int IO>
static int layernorm_impl(void* stream, const void* X, int64_t ldx, const void* gamma, const void* beta, void* Y, int64_t ldy, int M,
                          int C, float eps) {
  typedef typename NormIO<IO>::in_t in_t;
  hipStream_t st = (hipStream_t)stream;
  const int nv = (C / 8 + 63) / 64;
  dim3 grid((M + 3) / 4), block(256);
#define LN_LAUNCH(NV) \
  hipLaunchKernelGGL((ln_kernel<NV, IO>), grid, block, 0, st, (const in_t*)X, ldx, (const u16*)gamma, (const u16*)beta, (u16*)Y, ldy, M, C, eps)
  if (nv <= 1) LN_LAUNCH(1);
  else if (nv <= 2) LN_LAUNCH(2);
  else if (nv <= 3) LN_LAUNCH(3);
  else if (nv <= 4) LN_LAUNCH(4);
  else LN_LAUNCH(8);
#undef LN_LAUNCH
  return dm4d_check_launch("ln_kernel");
}

template <class Out>
static int layernorm_f32_impl(void* stream, const float* X, int64_t ldx, const void* gamma, const void* beta, void* Y, int64_t ldy, int M,
                              int C, float eps) {
  hipLaunchKernelGGL(ln32_kernel<Out>, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, X, ldx, (const u16*)gamma, (const u16*)beta,
                     (u16*)Y, ldy, M, C, eps);
  return dm4d_check_launch("ln32_kernel");
}

extern "C" int dm4d_layernorm_bf16(void* stream, const void* X, int64_t ldx, const void* gamma, const void* beta,
                                   void* Y, int64_t ldy, int M, int C, float eps) {
  if (!X || !gamma || !beta || !Y || M <= 0 || C <= 0)
    return dm4d_set_error(DM4D_ERR_ARG, "layernorm: null pointer or empty shape");
  if ((C & 7) || (ldx & 7) || (ldy & 7) || C > 64 * 8 * 8)
    return dm4d_set_error(DM4D_ERR_ARG, "layernorm: C must be a multiple of 8 and <= 4096");
  return layernorm_impl<0>(stream, X, ldx, gamma, beta, Y, ldy, M, C, eps);
}

extern "C" int dm4d_layernorm_f32_split(void* stream, const float* X, int64_t ldx, const void* gamma, const void* beta, void* Y,
                                        int64_t ldy, int M, int C, float eps) {
  if (!X || !gamma || !beta || !Y || M <= 0 || C <= 0 || ldx < C || ldy < 2 * (int64_t)C)
    return dm4d_set_error(DM4D_ERR_ARG, "layernorm_f32: bad arguments");
  return layernorm_f32_impl<OutSplit>(stream, X, ldx, gamma, beta, Y, ldy, M, C, eps);
}

extern "C" int dm4d_layernorm_f32_f16_general(void* stream, const float* X, int64_t ldx, const void* gamma, const void* beta, void* Y,
                                              int64_t ldy, int M, int C, float eps) {
  if (!X || !gamma || !beta || !Y || M <= 0 || C <= 0 || ldx < C || ldy < (int64_t)C)
    return dm4d_set_error(DM4D_ERR_ARG, "layernorm_f32_f16: bad arguments");
  return layernorm_f32_impl<OutF16>(stream, X, ldx, gamma, beta, Y, ldy, M, C, eps);
}

// precision "fp16": fp32 rows in (kept in registers: read once), one fp16 plane out.  Rows that are not 16-byte vectors of eight
// channels take the general kernel.
extern "C" int dm4d_layernorm_f32_f16(void* stream, const float* X, int64_t ldx, const void* gamma, const void* beta, void* Y,
                                      int64_t ldy, int M, int C, float eps) {
  if (!X || !gamma || !beta || !Y || M <= 0 || C <= 0 || ldx < C || ldy < (int64_t)C)
    return dm4d_set_error(DM4D_ERR_ARG, "layernorm_f32_f16: bad arguments");
  if ((C & 7) || (ldx & 3) || (ldy & 7) || C > 64 * 8 * 8 || (((uintptr_t)X) & 15) || (((uintptr_t)Y) & 15) || (((uintptr_t)gamma) & 15) ||
      (((uintptr_t)beta) & 15))
    return dm4d_layernorm_f32_f16_general(stream, X, ldx, gamma, beta, Y, ldy, M, C, eps);
  return layernorm_impl<2>(stream, X, ldx, gamma, beta, Y, ldy, M, C, eps);
}

extern "C" int dm4d_softmax_rows_bf16(void* stream, const void* S, int64_t lds, void* P, int64_t ldp, int M, int N,
                                      float scale) {
  if (!S || !P || M <= 0 || N <= 0) return dm4d_set_error(DM4D_ERR_ARG, "softmax: null pointer or empty shape");
  hipLaunchKernelGGL(softmax_rows_kernel, dim3(M), dim3(256), 0, (hipStream_t)stream, (const u16*)S, lds, (u16*)P, ldp,
                     N, scale);
  return dm4d_check_launch("softmax_rows_kernel");
}

extern "C" int dm4d_softmax_rows_f32in_bf16(void* stream, const float* S, int64_t lds, void* P, int64_t ldp, int M, int N,
                                            float scale) {
  if (!S || !P || M <= 0 || N <= 0) return dm4d_set_error(DM4D_ERR_ARG, "softmax: null pointer or empty shape");
  if ((lds & 3) || (ldp & 3) || lds < N || ldp < N || (((uintptr_t)S) & 15) || (((uintptr_t)P) & 7))
    return dm4d_set_error(DM4D_ERR_ARG, "softmax (fp32 logits): row strides must be multiples of 4 and >= N, rows 16-byte aligned");
  hipLaunchKernelGGL(softmax_rows_f32_kernel, dim3(M), dim3(256), 0, (hipStream_t)stream, S, lds, (u16*)P, ldp, N, scale);
  return dm4d_check_launch("softmax_rows_f32_kernel");
}

extern "C" int dm4d_softmax_rows_f32_f16(void* stream, const float* S, int64_t lds, void* P, int64_t ldp, int M, int N, int Np,
                                         float scale) {
  if (!S || !P || M <= 0 || N <= 0 || Np < N || lds < N || ldp < (int64_t)Np)
    return dm4d_set_error(DM4D_ERR_ARG, "softmax_rows_f32_f16: bad arguments");
  hipLaunchKernelGGL(softmax32_split_kernel<true>, dim3(M), dim3(256), 0, (hipStream_t)stream, S, lds, (u16*)P, ldp, M, N, Np, scale);
  return dm4d_check_launch("softmax32_split_kernel");
}

extern "C" int dm4d_softmax_rows_f32_split(void* stream, const float* S, int64_t lds, void* P, int64_t ldp, int M, int N, int Np,
                                           float scale) {
  if (!S || !P || M <= 0 || N <= 0 || Np < N || lds < N || ldp < 3 * (int64_t)Np)
    return dm4d_set_error(DM4D_ERR_ARG, "softmax_rows_f32_split: bad arguments");
  hipLaunchKernelGGL(softmax32_split_kernel<false>, dim3(M), dim3(256), 0, (hipStream_t)stream, S, lds, (u16*)P, ldp, M, N, Np, scale);
  return dm4d_check_launch("softmax32_split_kernel");
}

extern "C" int dm4d_tune_set_groupnorm_resident(int on) {
  g_gn_resident = on;
  return DM4D_OK;
}
