// Parity-precision kernels for gfx950 (host/ops.py, precision = "parity"): the same path with fp32 tensors between kernels and
// TWO-TERM bf16 operands on the matrix unit.
//
// Why: BASELINE.json's north_star asks for decoded RGB within 1e-3 rel-L2 of the reference's fp32 CPU path.  The fast path cannot
// get there -- rounding the MFMA operands to bf16 alone costs 7e-3 on the judged UNet call (profiles/r03_error_budget.log) -- and
// gfx950 has neither an xf32 mode nor a fast fp32 MFMA.  A bf16/fp16 checkpoint's WEIGHTS are exact in bf16, so only the
// activations need more bits: x = hi + lo with hi = bf16(x), lo = bf16(x - hi) carries 16 mantissa bits (|x - hi - lo| <= 2^-17 |x|),
// and  x W^T = [hi | lo] [W | W]^T  is one more pass of the SAME kernels over a K axis twice as long (dm4d_gemm_bf16 /
// dm4d_conv3x3_nhwc_bf16_flags with DM4D_EPI_F32OUT / F32SIDE / SPLITOUT).  This file holds what sits between those launches:
//   * split_kernel            fp32 [M, C] (one or two sources = the up-block channel concat) -> operand [M, hi(Cp) | lo(Cp)]
//   * to_f16_vec8_kernel      the same tensor as ONE fp16 plane, eight channels per thread (precision "fp16")
//   * attn_split_kernel       the d = 64 flash attention with three MFMAs per product (Kh Qh + Kh Ql + Kl Qh; Vh Ph + Vl Ph + Vh Pl),
//                             exact running-max softmax in fp32, operand out
// The normalisations and the row softmax of this precision (gn32_*, ln32_kernel, softmax32_split_kernel) live in norm.hip with the
// fast ones.
// None of these is tuned: the parity mode exists to PROVE the arithmetic of the path (tests/modelcheck.py --precision parity), its
// cost is reported beside the fast mode's (bench.py `parity`).
#include "common.h"
#include "dm4d.h"
#include "errors.h"

namespace {

// ------------------------------------------------------------------------------------------------
// fp32 -> two-term operand
// ------------------------------------------------------------------------------------------------
struct SplitParams {
  const float* X1;
  int64_t rs1, cs1;  // row / column stride of X1 in floats (cs1 != 1: a transposed read, V^T of the VAE mid block)
  const float* X2;
  int64_t rs2;
  int C1, C2, Cp;
  int64_t M;
  u16* Y;
  int64_t ldy;
  int act;      // 1 = SiLU
  float scale;  // applied after the activation
  int pattern;  // 0: [hi | lo]   1: [hi | lo | hi]   2: [hi | hi | lo]   3: one fp16 plane (precision "fp16")
};

__global__ __launch_bounds__(256) void split_kernel(SplitParams p) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.M * p.Cp) return;
  const int64_t m = i / p.Cp;
  const int c = (int)(i - m * p.Cp);
  float x = 0.f;
  if (c < p.C1) x = p.X1[m * p.rs1 + (int64_t)c * p.cs1];
  else if (c < p.C1 + p.C2) x = p.X2[m * p.rs2 + (c - p.C1)];
  if (p.act == 1) x = silu_f(x);
  x *= p.scale;
  u16* y = p.Y + m * p.ldy + c;
  if (p.pattern == 3) {
    y[0] = f2h_sat(x);
    return;
  }
  u16 hi, lo;
  split2(x, hi, lo);
  y[0] = hi;
  if (p.pattern == 0) {
    y[p.Cp] = lo;
  } else if (p.pattern == 1) {
    y[p.Cp] = lo;
    y[2 * p.Cp] = hi;
  } else {
    y[p.Cp] = hi;
    y[2 * p.Cp] = lo;
  }
}

// precision "fp16", the plain case (round 6): contiguous channels, every count a multiple of 8, 16-byte aligned rows -- eight channels per
// thread, 2 x 16 bytes in, 16 bytes out (the per-element kernel above moved 1.6 TB/s on the 72 x 40 level's tensors; same values:
// act, scale, one saturating rounding)
__global__ __launch_bounds__(256) void to_f16_vec8_kernel(SplitParams p) {
  const int CV = p.Cp >> 3;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.M * CV) return;
  const int64_t m = i / CV;
  const int c = (int)(i - m * CV) << 3;
  float v[8];
  if (c < p.C1 + p.C2) {
    const float* src = c < p.C1 ? p.X1 + m * p.rs1 + c : p.X2 + m * p.rs2 + (c - p.C1);
    const f32x4_t a = *reinterpret_cast<const f32x4_t*>(src), b = *reinterpret_cast<const f32x4_t*>(src + 4);
    v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
    v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = 0.f;
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float x = v[e];
    if (p.act == 1) x = silu_f(x);
    v[e] = x * p.scale;
  }
  stg16(p.Y + m * p.ldy + c, pack8h_sat(v));
}

// ------------------------------------------------------------------------------------------------
// Self-attention, head_dim 64, two-term Q / K / V (hi plane at the pointer, lo plane `*_lo` elements behind it), exact
// running-max softmax in fp32, two-term P, operand out.  Loop structure, LDS layouts and the register <-> key mapping are those
// of attention.hip's exact loop (kv_loop<SAFE>): S^T = K Q^T with lane (q = lane & 31) holding 16 of a 32-key block's scores,
// O^T = V^T P^T with V delivered by transposing LDS reads in the accumulator's key order.
// ------------------------------------------------------------------------------------------------
struct AttnSplitParams {
  const u16 *Q, *K, *V;
  u16* O;
  int64_t ldq, ldk, ldv, ldo;
  int64_t q_lo, k_lo, v_lo, o_lo;
  int L, Lk, heads, nqt;
  float c;  // scale * log2(e)
};


constexpr int KV = 64;
constexpr int LDK = 72;  // K rows: 64 + 8 pad bf16
constexpr int LDV = 96;  // V rows: 64 + 32 pad bf16
constexpr int LDO = 72;
constexpr float RESCALE_THR = 8.0f;

__device__ __forceinline__ bf16x8_t pack_frag(const float* v) {
  U4 w = pack8(v);
  return *reinterpret_cast<bf16x8_t*>(&w);
}

template <int NW>
__global__ __launch_bounds__(NW * 64) void attn_split_kernel(AttnSplitParams p) {
  constexpr int KS = 2 * KV * LDK, VS = 2 * KV * LDV;  // elements of one double-buffered plane
  __shared__ __attribute__((aligned(16))) u16 smem[2 * KS + 2 * VS];
  u16* Ks[2] = {smem, smem + KS};                    // [plane][buf][64][LDK]
  u16* Vs[2] = {smem + 2 * KS, smem + 2 * KS + VS};  // [plane][buf][64][LDV]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, lh = lane >> 5;
  const int L = p.L, Lk = p.Lk;
  const int lid = xcd_remap(blockIdx.x, gridDim.x);
  const int qt = lid % p.nqt, bh = lid / p.nqt;
  const int head = bh % p.heads, batch = bh / p.heads;
  const int q_tile0 = qt * (NW * 32) + wave * 32;
  const u16* Qb = p.Q + (int64_t)batch * L * p.ldq + head * 64;
  const u16* Kb = p.K + (int64_t)batch * Lk * p.ldk + head * 64;
  const u16* Vb = p.V + (int64_t)batch * Lk * p.ldv + head * 64;
  u16* Ob = p.O + (int64_t)batch * L * p.ldo + head * 64;

  bf16x8_t qf[2][4];
  {
    int q = q_tile0 + l31;
    if (q > L - 1) q = L - 1;
    const u16* qp = Qb + (int64_t)q * p.ldq + lh * 8;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      U4 v = ldg16(qp + j * 16);
      qf[0][j] = *reinterpret_cast<bf16x8_t*>(&v);
      U4 w = ldg16(qp + p.q_lo + j * 16);
      qf[1][j] = *reinterpret_cast<bf16x8_t*>(&w);
    }
  }
  f32x16_t o[2];
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[db][r] = 0.f;
  float m_run = -1e30f, l_run = 0.f;
  const float cs = p.c;

  constexpr int RPT = 8 / NW;  // key rows per thread and tile
  static_assert(RPT >= 1, "at most 8 waves");
  U4 rk[2][RPT], rv[2][RPT];
  const int s_key = tid >> 3, s_c = tid & 7;
  auto load_tile = [&](int t) {
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      int key = t * KV + s_key + i * (NW * 8);
      if (key > Lk - 1) key = Lk - 1;
      const u16* kp = Kb + (int64_t)key * p.ldk + s_c * 8;
      const u16* vp = Vb + (int64_t)key * p.ldv + s_c * 8;
      rk[0][i] = ldg16(kp);
      rk[1][i] = ldg16(kp + p.k_lo);
      rv[0][i] = ldg16(vp);
      rv[1][i] = ldg16(vp + p.v_lo);
    }
  };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int pl = 0; pl < 2; ++pl)
#pragma unroll
      for (int i = 0; i < RPT; ++i) {
        *reinterpret_cast<U4*>(Ks[pl] + (buf * KV + s_key + i * (NW * 8)) * LDK + s_c * 8) = rk[pl][i];
        *reinterpret_cast<U4*>(Vs[pl] + (buf * KV + s_key + i * (NW * 8)) * LDV + s_c * 8) = rv[pl][i];
      }
  };
  // V fragment base (elements inside a plane): row 4 lh + ((lane & 15) >> 2), column 16 ((lane >> 4) & 1) + 4 (lane & 3)
  const int v_lane = (4 * lh + ((lane & 15) >> 2)) * LDV + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);

  const int nt = (Lk + KV - 1) / KV;
  load_tile(0);
  store_tile(0);
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    const int buf = t & 1;
    if (t + 1 < nt) load_tile(t + 1);
    f32x16_t s[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) s[kb][r] = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        const int off = (buf * KV + kb * 32 + l31) * LDK + j * 16 + lh * 8;
        const bf16x8_t kh = *reinterpret_cast<const bf16x8_t*>(Ks[0] + off);
        const bf16x8_t kl = *reinterpret_cast<const bf16x8_t*>(Ks[1] + off);
        s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kl, qf[0][j], s[kb], 0, 0, 0);
        s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kh, qf[1][j], s[kb], 0, 0, 0);
        s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kh, qf[0][j], s[kb], 0, 0, 0);
      }
    if ((t == nt - 1) && (Lk % KV) != 0) {
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        const int key0 = t * KV + kb * 32 + 4 * lh;
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (key0 + (r & 3) + 8 * (r >> 2) >= Lk) s[kb][r] = -1e30f;
      }
    }
    {
      float mx = fmaxf(s[0][0], s[1][0]);
#pragma unroll
      for (int r = 1; r < 16; ++r) mx = fmaxf(mx, fmaxf(s[0][r], s[1][r]));
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      if (__any((mx - m_run) * cs > RESCALE_THR)) {
        const float m_new = fmaxf(m_run, mx);
        const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * cs);
        m_run = m_new;
        l_run *= alpha;
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
          for (int r = 0; r < 16; ++r) o[db][r] *= alpha;
      }
    }
    const float mc = m_run * cs;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      float ph[16], pl[16];
      float sum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float pv = s[kb][r] <= -1e29f ? 0.f : __builtin_amdgcn_exp2f(s[kb][r] * cs - mc);
        sum += pv;
        ph[r] = bf2f(f2bf(pv));
        pl[r] = pv - ph[r];
      }
      l_run += sum;
      bf16x8_t pfh[2], pfl[2];
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        pfh[jj] = pack_frag(ph + jj * 8);
        pfl[jj] = pack_frag(pl + jj * 8);
      }
#pragma unroll
      for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
          const int off = v_lane + (buf * KV + kb * 32 + jj * 16) * LDV + db * 32;
          bf16x8_t vf[2];
#pragma unroll
          for (int pln = 0; pln < 2; ++pln) {
            const u16* vp = Vs[pln] + off;
            s16x4_t v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_p)vp);
            s16x4_t v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_p)(vp + 8 * LDV));
            s16x8_t v01 = __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7);
            vf[pln] = *reinterpret_cast<bf16x8_t*>(&v01);
          }
          o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[1], pfh[jj], o[db], 0, 0, 0);
          o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[0], pfl[jj], o[db], 0, 0, 0);
          o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[0], pfh[jj], o[db], 0, 0, 0);
        }
    }
    if (t + 1 < nt) store_tile(buf ^ 1);
    __syncthreads();
  }
  const float l_tot = l_run + __shfl_xor(l_run, 32);
  const float inv = 1.0f / l_tot;
  // O through two wave-private LDS tiles (hi, lo), then whole 128-byte rows out; the loop ended with a workgroup barrier
  u16* Oh = smem + wave * (32 * LDO);
  u16* Ol = smem + (NW + wave) * (32 * LDO);
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float v[4], h[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] = o[db][4 * g + e] * inv;
        h[e] = bf2f(f2bf(v[e]));
      }
      uint2 wh, wl;
      wh.x = pack_bf2(h[0], h[1]);
      wh.y = pack_bf2(h[2], h[3]);
      wl.x = pack_bf2(v[0] - h[0], v[1] - h[1]);
      wl.y = pack_bf2(v[2] - h[2], v[3] - h[3]);
      *reinterpret_cast<uint2*>(Oh + l31 * LDO + db * 32 + 8 * g + 4 * lh) = wh;
      *reinterpret_cast<uint2*>(Ol + l31 * LDO + db * 32 + 8 * g + 4 * lh) = wl;
    }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int row = 8 * k + (lane >> 3), ch = lane & 7;
    const u32x4_t vh = *reinterpret_cast<const u32x4_t*>(Oh + row * LDO + ch * 8);
    const u32x4_t vl = *reinterpret_cast<const u32x4_t*>(Ol + row * LDO + ch * 8);
    const int q = q_tile0 + row;
    if (q < L) {
      *reinterpret_cast<u32x4_t*>(Ob + (int64_t)q * p.ldo + ch * 8) = vh;
      *reinterpret_cast<u32x4_t*>(Ob + (int64_t)q * p.ldo + p.o_lo + ch * 8) = vl;
    }
  }
}

}  // namespace

extern "C" int dm4d_split_f32(void* stream, const float* X1, int64_t row_stride1, int64_t col_stride1, int C1, const float* X2,
                              int64_t row_stride2, int C2, void* Y, int64_t ldy, int64_t M, int Cp, int act_silu, float scale,
                              int pattern) {
  if (!X1 || !Y || M <= 0 || C1 <= 0 || C2 < 0 || (C2 > 0 && !X2) || Cp < C1 + C2 || pattern < 0 || pattern > 2)
    return dm4d_set_error(DM4D_ERR_ARG, "split_f32: bad arguments");
  if (ldy < (int64_t)(pattern == 0 ? 2 : 3) * Cp) return dm4d_set_error(DM4D_ERR_ARG, "split_f32: ldy too small for the planes");
  SplitParams p{X1, row_stride1, col_stride1, X2, row_stride2, C1, C2, Cp, M, (u16*)Y, ldy, act_silu, scale, pattern};
  hipLaunchKernelGGL(split_kernel, grid1d(M * Cp, 256), dim3(256), 0, (hipStream_t)stream, p);
  return dm4d_check_launch("split_kernel");
}

extern "C" int dm4d_to_f16_f32(void* stream, const float* X1, int64_t row_stride1, int64_t col_stride1, int C1, const float* X2,
                               int64_t row_stride2, int C2, void* Y, int64_t ldy, int64_t M, int Cp, int act_silu, float scale) {
  if (!X1 || !Y || M <= 0 || C1 <= 0 || C2 < 0 || (C2 > 0 && !X2) || Cp < C1 + C2 || ldy < Cp)
    return dm4d_set_error(DM4D_ERR_ARG, "to_f16_f32: bad arguments");
  SplitParams p{X1, row_stride1, col_stride1, X2, row_stride2, C1, C2, Cp, M, (u16*)Y, ldy, act_silu, scale, 3};
  const bool vec8 = col_stride1 == 1 && ((C1 | C2 | Cp) & 7) == 0 && (row_stride1 & 3) == 0 && (C2 == 0 || (row_stride2 & 3) == 0) && (ldy & 7) == 0 &&
                    (((uintptr_t)X1) & 15) == 0 && (C2 == 0 || (((uintptr_t)X2) & 15) == 0) && (((uintptr_t)Y) & 15) == 0;
  if (vec8) {
    hipLaunchKernelGGL(to_f16_vec8_kernel, grid1d(M * (Cp >> 3), 256), dim3(256), 0, (hipStream_t)stream, p);
    return dm4d_check_launch("to_f16_vec8_kernel");
  }
  hipLaunchKernelGGL(split_kernel, grid1d(M * Cp, 256), dim3(256), 0, (hipStream_t)stream, p);
  return dm4d_check_launch("split_kernel");
}

extern "C" int dm4d_attention_split_bf16(void* stream, const void* Q, const void* K, const void* V, void* O, int64_t ldq, int64_t ldk,
                                         int64_t ldv, int64_t ldo, int64_t q_lo, int64_t k_lo, int64_t v_lo, int64_t o_lo, int batch,
                                         int heads, int Lq, int Lk, float scale) {
  if (!Q || !K || !V || !O || batch <= 0 || heads <= 0 || Lq <= 0 || Lk <= 0)
    return dm4d_set_error(DM4D_ERR_ARG, "attention_split: null pointer or empty shape");
  if ((ldq & 7) || (ldk & 7) || (ldv & 7) || (ldo & 7) || (q_lo & 7) || (k_lo & 7) || (v_lo & 7) || (o_lo & 7))
    return dm4d_set_error(DM4D_ERR_ARG, "attention_split: strides and plane offsets must be multiples of 8 elements");
  if ((((uintptr_t)Q) | ((uintptr_t)K) | ((uintptr_t)V) | ((uintptr_t)O)) & 15)
    return dm4d_set_error(DM4D_ERR_ARG, "attention_split: Q, K, V and O must be 16-byte aligned");
  AttnSplitParams p{(const u16*)Q, (const u16*)K, (const u16*)V, (u16*)O, ldq, ldk, ldv, ldo, q_lo, k_lo, v_lo, o_lo,
                    Lq, Lk, heads, 0, scale * 1.4426950408889634f};
  constexpr int nw = 8;
  p.nqt = (Lq + nw * 32 - 1) / (nw * 32);
  const long nwg = (long)p.nqt * heads * batch;
  if (nwg > 0x7fffffffL) return dm4d_set_error(DM4D_ERR_ARG, "attention_split: grid too large");
  hipLaunchKernelGGL((attn_split_kernel<nw>), dim3((unsigned)nwg), dim3(nw * 64), 0, (hipStream_t)stream, p);
  return dm4d_check_launch("attn_split_kernel");
}
