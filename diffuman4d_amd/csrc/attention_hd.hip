// Flash-style self-attention for gfx950 at the head dimensions of the SD-1.x UNet layout: D = 40, 80, 160 (8 heads over
// 320 / 640 / 1280 channels).  The D = 64 kernels of attention.hip are untouched; host/ops.py picks the entry from the operand widths.
//
// One kernel template, three operand forms (MODE):
//   BF16  dm4d_attention_hd_qscaled_kv_bf16  bf16 Q (carrying scale * log2 e) / K / V -> bf16 O, one MFMA per product;
//   F16   dm4d_attention_hd_qscaled_kv_f16   the same on fp16 operands (precision "fp16");
//   SPLIT dm4d_attention_hd_split_bf16       two-term Q / K / V / O (hi plane at the pointer, lo plane `*_lo` elements behind it),
//                                            three MFMAs per product (Kh Qh + Kh Ql + Kl Qh; Vh Ph + Vl Ph + Vh Pl), unscaled Q
//                                            (scores times scale * log2 e in fp32) -- the parity precision.
// Work decomposition and register <-> key mapping are those of attention.hip's exact loop (kv_loop<SAFE>): a workgroup = 8 waves,
// each wave owns 32 query rows; K/V tiles of KT keys are staged through registers into double-buffered LDS.  Per 32-key block,
// on v_mfma_f32_32x32x16_{bf16,f16}:
//   S^T = K Q^T over the head dimension padded to DP = 16 ceil(D / 16) (48 / 80 / 160): NJ = DP / 16 MFMAs;
//   O^T = V^T P^T with P^T packed straight from the S^T accumulator and V^T from transposing LDS reads (ds_read_b64_tr_b16); O^T rows
//         are d, padded to DO = 32 ceil(D / 32) (64 / 96 / 160): NDB = DO / 32 accumulator blocks.
// Padding: only whole 8-element chunks below D are ever read from memory (D is a multiple of 8, so a chunk is all in or all out);
// the padding chunks of Q (registers) and K / V (LDS) are written as zeros, never filled from the neighbouring head or from past the
// end of the row.  O stores write exactly the head's D columns.
// LDS rows (u16 elements): K rows LDK = DP + 8 (56 / 88 / 168: 28 / 44 / 84 dwords, an odd number of 16-byte groups, so the 16 rows
// of a ds_read_b128 phase land in 16 distinct bank quads); V rows LDV = 96 / 96 / 160 (48 / 48 / 80 dwords = 48 / 48 / 16 mod 64: the
// four rows of one transposing read phase tile the 64 banks, as attention.hip's 96-element exact-loop rows do).
// Softmax: exact running maximum, fp32, per ROW (no wave vote: a row's arithmetic does not depend on which rows share its wave or
// workgroup, so a rank's slice of the queries reproduces the unsharded rows bit for bit); every tile rescales by
// alpha = exp2(m_old - m_new), which is exactly 1 when the maximum did not move.  All probabilities are <= 1, so fp16 holds them.
// Lq, Lk >= 1 independently (frame-sharded 3-D attention: Lk = world * Lq); ragged tails are clamped on load and masked on scores.
#include "common.h"
#include "dm4d.h"
#include "errors.h"
#include <stdio.h>

namespace {

enum { MODE_BF16 = 0, MODE_F16 = 1, MODE_SPLIT = 2 };

struct AttnHdParams {
  const u16 *Q, *K, *V;
  u16* O;
  int64_t ldq, ldk, ldv, ldo;
  int64_t q_lo, k_lo, v_lo, o_lo;  // SPLIT: element offset of the lo plane
  int L, Lk, heads, nqt;
  float c;  // SPLIT: scale * log2(e); the pre-scaled forms ignore it
};

constexpr int NW = 8;  // waves per workgroup, 32 query rows each

template <int D>
struct HdGeom {
  static_assert(D % 8 == 0, "whole 16-byte chunks");
  static constexpr int DP = (D + 15) / 16 * 16;  // QK^T contraction
  static constexpr int DO = (D + 31) / 32 * 32;  // O^T rows
  static constexpr int NJ = DP / 16, NDB = DO / 32;
  static constexpr int LDK = DP + 8;
  static constexpr int LDV = DO == 160 ? 160 : 96;
  static_assert((LDK / 8) % 2 == 1, "K rows: odd number of 16-byte groups");
  static_assert(LDV >= DO && ((LDV / 2) % 64 == 16 || (LDV / 2) % 64 == 48), "V rows: four rows tile the banks");
};

__device__ __forceinline__ bf16x8_t as_frag(const U4& v) { return __builtin_bit_cast(bf16x8_t, v); }

template <int D, int MODE>
__global__ __launch_bounds__(NW * 64) void attn_hd_kernel(AttnHdParams p) {
  using G = HdGeom<D>;
  constexpr bool SPLIT = MODE == MODE_SPLIT, H16 = MODE == MODE_F16;
  constexpr int NP = SPLIT ? 2 : 1;                 // operand planes
  constexpr int KT = (SPLIT && D > 128) ? 32 : 64;  // keys per tile (two-plane D = 160 rings at 64 keys exceed the 160 KiB of LDS)
  constexpr int NKB = KT / 32;
  constexpr int KCH = G::DP / 8, VCH = G::DO / 8;   // 16-byte chunks per staged row
  constexpr int KIT = (KT * KCH + NW * 64 - 1) / (NW * 64), VIT = (KT * VCH + NW * 64 - 1) / (NW * 64);
  constexpr int KS = 2 * KT * G::LDK, VS = 2 * KT * G::LDV;  // elements of one double-buffered plane
  __shared__ __attribute__((aligned(16))) u16 smem[NP * (KS + VS)];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, lh = lane >> 5;
  const int L = p.L, Lk = p.Lk;
  const int lid = xcd_remap(blockIdx.x, gridDim.x);
  const int qt = lid % p.nqt, bh = lid / p.nqt;
  const int head = bh % p.heads, batch = bh / p.heads;
  const int q_tile0 = qt * (NW * 32) + wave * 32;
  const u16* Qb = p.Q + (int64_t)batch * L * p.ldq + head * D;
  const u16* Kb = p.K + (int64_t)batch * Lk * p.ldk + head * D;
  const u16* Vb = p.V + (int64_t)batch * Lk * p.ldv + head * D;
  u16* Ob = p.O + (int64_t)batch * L * p.ldo + head * D;
  const U4 zero = {0u, 0u, 0u, 0u};

  // Q fragments: lane (q = l31) holds d = 16 j + 8 lh .. + 7 of its row; chunks at or past D are zero
  bf16x8_t qf[NP][G::NJ];
  {
    int q = q_tile0 + l31;
    if (q > L - 1) q = L - 1;
    const u16* qp = Qb + (int64_t)q * p.ldq + lh * 8;
#pragma unroll
    for (int j = 0; j < G::NJ; ++j) {
      const bool in = 16 * j + 8 * lh < D;
#pragma unroll
      for (int pl = 0; pl < NP; ++pl) qf[pl][j] = as_frag(in ? ldg16(qp + (pl ? p.q_lo : 0) + j * 16) : zero);
    }
  }
  f32x16_t o[G::NDB];
#pragma unroll
  for (int db = 0; db < G::NDB; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[db][r] = 0.f;
  float m_run = -1e30f, l_run = 0.f;
  const float cs = SPLIT ? p.c : 1.0f;

  // staging: chunk c of a tile = row c / CH, 16-byte chunk c % CH; source rows clamped to Lk - 1, padding chunks zero
  U4 rk[NP][KIT], rv[NP][VIT];
  auto load_tile = [&](int t) {
#pragma unroll
    for (int i = 0; i < KIT; ++i) {
      const int c = tid + i * NW * 64, row = c / KCH, ch = c % KCH;
      int key = t * KT + row;
      if (key > Lk - 1) key = Lk - 1;
      const bool in = c < KT * KCH && ch * 8 < D;
#pragma unroll
      for (int pl = 0; pl < NP; ++pl) rk[pl][i] = in ? ldg16(Kb + (int64_t)key * p.ldk + (pl ? p.k_lo : 0) + ch * 8) : zero;
    }
#pragma unroll
    for (int i = 0; i < VIT; ++i) {
      const int c = tid + i * NW * 64, row = c / VCH, ch = c % VCH;
      int key = t * KT + row;
      if (key > Lk - 1) key = Lk - 1;
      const bool in = c < KT * VCH && ch * 8 < D;
#pragma unroll
      for (int pl = 0; pl < NP; ++pl) rv[pl][i] = in ? ldg16(Vb + (int64_t)key * p.ldv + (pl ? p.v_lo : 0) + ch * 8) : zero;
    }
  };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int i = 0; i < KIT; ++i) {
      const int c = tid + i * NW * 64, row = c / KCH, ch = c % KCH;
      if (c < KT * KCH)
#pragma unroll
        for (int pl = 0; pl < NP; ++pl) *reinterpret_cast<U4*>(smem + pl * KS + (buf * KT + row) * G::LDK + ch * 8) = rk[pl][i];
    }
#pragma unroll
    for (int i = 0; i < VIT; ++i) {
      const int c = tid + i * NW * 64, row = c / VCH, ch = c % VCH;
      if (c < KT * VCH)
#pragma unroll
        for (int pl = 0; pl < NP; ++pl)
          *reinterpret_cast<U4*>(smem + NP * KS + pl * VS + (buf * KT + row) * G::LDV + ch * 8) = rv[pl][i];
    }
  };
  // V fragment base (elements inside a plane): row 4 lh + ((lane & 15) >> 2), column 16 ((lane >> 4) & 1) + 4 (lane & 3)
  const int v_lane = (4 * lh + ((lane & 15) >> 2)) * G::LDV + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);

  const int nt = (Lk + KT - 1) / KT;
  load_tile(0);
  store_tile(0);
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    const int buf = t & 1;
    if (t + 1 < nt) load_tile(t + 1);
    f32x16_t s[NKB];
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) s[kb][r] = 0.f;
#pragma unroll
    for (int j = 0; j < G::NJ; ++j)
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb) {
        const int off = (buf * KT + kb * 32 + l31) * G::LDK + j * 16 + lh * 8;
        const bf16x8_t kh = *reinterpret_cast<const bf16x8_t*>(smem + off);
        if constexpr (SPLIT) {
          const bf16x8_t kl = *reinterpret_cast<const bf16x8_t*>(smem + KS + off);
          s[kb] = mfma32<false>(kl, qf[0][j], s[kb]);
          s[kb] = mfma32<false>(kh, qf[NP - 1][j], s[kb]);
        }
        s[kb] = mfma32<H16>(kh, qf[0][j], s[kb]);
      }
    if ((t == nt - 1) && (Lk % KT) != 0) {
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb) {
        const int key0 = t * KT + kb * 32 + 4 * lh;
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (key0 + (r & 3) + 8 * (r >> 2) >= Lk) s[kb][r] = -1e30f;
      }
    }
    // exact running maximum of this lane's row (the two lane halves hold the two halves of the row's scores)
    {
      float mx = s[0][0];
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[kb][r]);
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      const float m_new = fmaxf(m_run, mx);
      const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * cs);
      m_run = m_new;
      l_run *= alpha;
#pragma unroll
      for (int db = 0; db < G::NDB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[db][r] *= alpha;
    }
    const float mc = m_run * cs;
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
      float pv[16];
      float sum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        pv[r] = s[kb][r] <= -1e29f ? 0.f : __builtin_amdgcn_exp2f(s[kb][r] * cs - mc);
        sum += pv[r];
      }
      l_run += sum;
      bf16x8_t pf[NP][2];  // SPLIT: [hi, lo] of P
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        U4 w;
        w.x = pack2<H16>(pv[jj * 8 + 0], pv[jj * 8 + 1]);
        w.y = pack2<H16>(pv[jj * 8 + 2], pv[jj * 8 + 3]);
        w.z = pack2<H16>(pv[jj * 8 + 4], pv[jj * 8 + 5]);
        w.w = pack2<H16>(pv[jj * 8 + 6], pv[jj * 8 + 7]);
        pf[0][jj] = as_frag(w);
        if constexpr (SPLIT) {
          float lo[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) lo[e] = pv[jj * 8 + e] - bf2f(f2bf(pv[jj * 8 + e]));
          pf[NP - 1][jj] = as_frag(pack8(lo));
        }
      }
#pragma unroll
      for (int db = 0; db < G::NDB; ++db)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
          const int off = v_lane + (buf * KT + kb * 32 + jj * 16) * G::LDV + db * 32;
          bf16x8_t vf[NP];
#pragma unroll
          for (int pl = 0; pl < NP; ++pl) {
            const u16* vp = smem + NP * KS + pl * VS + off;
            s16x4_t v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_p)vp);
            s16x4_t v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_p)(vp + 8 * G::LDV));
            s16x8_t v01 = __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7);
            vf[pl] = __builtin_bit_cast(bf16x8_t, v01);
          }
          if constexpr (SPLIT) {
            o[db] = mfma32<false>(vf[1], pf[0][jj], o[db]);
            o[db] = mfma32<false>(vf[0], pf[1][jj], o[db]);
          }
          o[db] = mfma32<H16>(vf[0], pf[0][jj], o[db]);
        }
    }
    if (t + 1 < nt) store_tile(buf ^ 1);
    __syncthreads();
  }
  // O^T block db: lane (q = l31) holds d = 32 db + 8 g + 4 lh + (0..3) in o[db][4 g ..]; 8-byte stores of exactly the head's D columns
  const float inv = 1.0f / (l_run + __shfl_xor(l_run, 32));
  const int q = q_tile0 + l31;
  if (q < L) {
    u16* orow = Ob + (int64_t)q * p.ldo;
#pragma unroll
    for (int db = 0; db < G::NDB; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d0 = 32 * db + 8 * g + 4 * lh;
        if (d0 < D) {
          float v[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = o[db][4 * g + e] * inv;
          uint2 w;
          w.x = pack2<H16>(v[0], v[1]);
          w.y = pack2<H16>(v[2], v[3]);
          *reinterpret_cast<uint2*>(orow + d0) = w;
          if constexpr (SPLIT) {
            float lo[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) lo[e] = v[e] - bf2f(f2bf(v[e]));
            uint2 wl;
            wl.x = pack_bf2(lo[0], lo[1]);
            wl.y = pack_bf2(lo[2], lo[3]);
            *reinterpret_cast<uint2*>(orow + p.o_lo + d0) = wl;
          }
        }
      }
  }
}

template <int MODE>
int attention_hd_launch(const char* what, void* stream, const void* Q, const void* K, const void* V, void* O, int64_t ldq, int64_t ldk,
                        int64_t ldv, int64_t ldo, int64_t q_lo, int64_t k_lo, int64_t v_lo, int64_t o_lo, int batch, int heads,
                        int head_dim, int Lq, int Lk, float scale) {
  char msg[256];
  if (head_dim != 40 && head_dim != 80 && head_dim != 160) {
    snprintf(msg, sizeof(msg), "%s: head_dim %d not supported (40, 80 or 160; head_dim 64 has its own entry points)", what, head_dim);
    return dm4d_set_error(DM4D_ERR_ARG, msg);
  }
  if (!Q || !K || !V || !O || batch <= 0 || heads <= 0 || Lq <= 0 || Lk <= 0) {
    snprintf(msg, sizeof(msg), "%s: null pointer or empty shape", what);
    return dm4d_set_error(DM4D_ERR_ARG, msg);
  }
  const int64_t C = (int64_t)heads * head_dim;
  if (ldq < C || ldk < C || ldv < C || ldo < C || (ldq & 7) || (ldk & 7) || (ldv & 7) || (ldo & 7)) {
    snprintf(msg, sizeof(msg), "%s: row strides must be >= heads * head_dim = %lld and multiples of 8 elements", what, (long long)C);
    return dm4d_set_error(DM4D_ERR_ARG, msg);
  }
  if ((q_lo & 7) || (k_lo & 7) || (v_lo & 7) || (o_lo & 7)) {
    snprintf(msg, sizeof(msg), "%s: plane offsets must be multiples of 8 elements", what);
    return dm4d_set_error(DM4D_ERR_ARG, msg);
  }
  if ((((uintptr_t)Q) | ((uintptr_t)K) | ((uintptr_t)V) | ((uintptr_t)O)) & 15) {
    snprintf(msg, sizeof(msg), "%s: Q, K, V and O must be 16-byte aligned", what);
    return dm4d_set_error(DM4D_ERR_ARG, msg);
  }
  AttnHdParams p{(const u16*)Q, (const u16*)K, (const u16*)V, (u16*)O, ldq, ldk, ldv, ldo, q_lo, k_lo, v_lo, o_lo,
                 Lq, Lk, heads, (Lq + NW * 32 - 1) / (NW * 32), scale * 1.4426950408889634f};
  const long nwg = (long)p.nqt * heads * batch;
  if (nwg > 0x7fffffffL) {
    snprintf(msg, sizeof(msg), "%s: grid too large", what);
    return dm4d_set_error(DM4D_ERR_ARG, msg);
  }
  const dim3 grid((unsigned)nwg), block(NW * 64);
  hipStream_t st = (hipStream_t)stream;
  if (head_dim == 40) hipLaunchKernelGGL((attn_hd_kernel<40, MODE>), grid, block, 0, st, p);
  else if (head_dim == 80) hipLaunchKernelGGL((attn_hd_kernel<80, MODE>), grid, block, 0, st, p);
  else hipLaunchKernelGGL((attn_hd_kernel<160, MODE>), grid, block, 0, st, p);
  return dm4d_check_launch("attn_hd_kernel");
}

}  // namespace

extern "C" int dm4d_attention_hd_qscaled_kv_bf16(void* stream, const void* Q, const void* K, const void* V, void* O, int64_t ldq,
                                                 int64_t ldk, int64_t ldv, int64_t ldo, int batch, int heads, int head_dim, int Lq,
                                                 int Lk) {
  return attention_hd_launch<MODE_BF16>("attention_hd_qscaled_kv_bf16", stream, Q, K, V, O, ldq, ldk, ldv, ldo, 0, 0, 0, 0, batch,
                                        heads, head_dim, Lq, Lk, 1.0f);
}

extern "C" int dm4d_attention_hd_qscaled_kv_f16(void* stream, const void* Q, const void* K, const void* V, void* O, int64_t ldq,
                                                int64_t ldk, int64_t ldv, int64_t ldo, int batch, int heads, int head_dim, int Lq,
                                                int Lk) {
  return attention_hd_launch<MODE_F16>("attention_hd_qscaled_kv_f16", stream, Q, K, V, O, ldq, ldk, ldv, ldo, 0, 0, 0, 0, batch,
                                       heads, head_dim, Lq, Lk, 1.0f);
}

extern "C" int dm4d_attention_hd_split_bf16(void* stream, const void* Q, const void* K, const void* V, void* O, int64_t ldq,
                                            int64_t ldk, int64_t ldv, int64_t ldo, int64_t q_lo, int64_t k_lo, int64_t v_lo,
                                            int64_t o_lo, int batch, int heads, int Lq, int Lk, float scale, int head_dim) {
  return attention_hd_launch<MODE_SPLIT>("attention_hd_split_bf16", stream, Q, K, V, O, ldq, ldk, ldv, ldo, q_lo, k_lo, v_lo, o_lo,
                                         batch, heads, head_dim, Lq, Lk, scale);
}
