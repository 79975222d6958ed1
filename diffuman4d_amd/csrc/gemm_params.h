// Launch parameters of the MFMA GEMM / convolution kernels (gemm.hip, ff_fused.hip): a kernel argument, so fields, order and types
// are ABI between host and device code.  Plain C++ (no HIP): csrc/gemm_select.h reads it on the host alone.
#pragma once
#include <stdint.h>

typedef unsigned short u16;

namespace {

struct GemmParams {
  const u16* A;
  int64_t lda;
  const u16* A2;
  int64_t lda2;
  int K1;
  // conv geometry (CONV only)
  int H, W, Cin, Ho, Wo, stride, pad, upsample;
  const u16* Wt;
  int64_t ldw;
  u16* C;
  int64_t ldc;
  int M, N, K;
  const u16* bias;
  const u16* rowbias;
  int64_t ld_rb;
  int rows_per_rb;
  const u16* res;
  int64_t ld_res;
  unsigned flags;
  float out_scale;
  int tiles_n;
  // split-K of the strip convolution over the 3 kernel rows (small images): partial sums go to ws[split][M][N] fp32
  int splits;
  float* ws;
  // phase-decomposed x2 upsampling convolution (conv_strip2_kernel<.., KT = 2>): rows m of the GEMM are LOW-resolution
  // pixels (b, y, x) of width up_w, output row = 2 m + 2 up_w (m / up_w) from a C pointer moved to the phase's first pixel
  int up_w;
  // precision "fp16" (PAR = 2 kernels): output columns [0, scale_cols) are multiplied by col_scale in fp32 before the one rounding
  // (the to_q third of a fused QKV projection takes scale * log2 e for dm4d_attention_qscaled_kv_f16); 0 = none
  int scale_cols;
  float col_scale;
};

}  // namespace
