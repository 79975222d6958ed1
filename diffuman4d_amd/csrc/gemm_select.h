// Which kernel configuration a GEMM / 3x3-convolution launch of gemm.hip takes: predicates, workspace rule, tile heuristic and the choice
// per precision, each written once.  Host-only, plain C++17 (no HIP), pure functions of the launch parameters: tests/gemm_select_probe.cpp
// compiles this header with the host compiler and tests/test_gemm_select_cpu.py pins what it returns (every kernel walks K in the same
// order, so a wrong choice never changes a result and no other test would notice).  launch_by_id of gemm.hip turns an id into a kernel.
#pragma once
#include "dm4d.h"
#include "gemm_params.h"
#include <stddef.h>
#include <type_traits>
#include <utility>

namespace {

enum { PREC_FAST = 0, PREC_PAR = 1, PREC_H16 = 2 };  // precision of a launch = the PAR argument of the kernel templates
// id: configuration id of launch_by_id, 0 = the precision has no kernel for this shape; splits: 3 = strip convolution split over its
// kernel rows (needs GemmParams::ws), else 1
struct GemmChoice { int id, splits; };

inline bool is_geglu(const GemmParams& p) { return (p.flags & DM4D_EPI_GEGLU) != 0; }

// the geometry the strip kernels (conv_strip2_kernel) serve: stride 1, pad 1, same-size output, K-slab of 64 inside one tap
inline bool strip_conv(const GemmParams& p) {
  return p.stride == 1 && p.pad == 1 && !p.upsample && p.Ho == p.H && p.Wo == p.W && p.Cin % 64 == 0;
}

// K-slab 64 (direct-to-LDS DMA); otherwise the K-slab 32 register-staged kernels
template <bool CONV>
inline bool k64(const GemmParams& p) { return CONV ? (p.Cin % 64 == 0) : (p.K % 64 == 0 && (!p.A2 || p.K1 % 64 == 0)); }
// 128-wide B tiles leave no (or few) padded columns
inline bool n128(const GemmParams& p) { return is_geglu(p) || (p.N % 128 == 0) || (p.N > 1024); }

// the second form addresses A, A2 and W with 32-bit byte offsets from a uniform base and walks K in slabs of 64
inline bool lin2_ok(const GemmParams& p) {
  return p.K % 64 == 0 && (!p.A2 || p.K1 % 64 == 0) && (uint64_t)p.M * (uint64_t)p.lda * 2u < (1ull << 32) &&
         (!p.A2 || (uint64_t)p.M * (uint64_t)p.lda2 * 2u < (1ull << 32)) &&
         (uint64_t)(2 * (uint64_t)p.N) * (uint64_t)p.ldw * 2u < (1ull << 32);
}

// the strip kernel addresses A and W with 32-bit byte offsets from a uniform base
inline bool strip2_ok(const GemmParams& p) {
  return (uint64_t)p.M * (uint64_t)p.Cin * 2u < (1ull << 32) && (uint64_t)p.N * (uint64_t)p.ldw * 2u < (1ull << 32);
}

// Split-K applies to stride-1 convolutions on small images (the 9x5 level of the UNet: M = B*45 rows against a
// 11520- or 23040-deep K).  The rule looks at the per-image geometry only, never at the batch, so a frame-sharded
// run (fewer frames per rank) sums in the same order as the unsharded one.
inline bool strip_split_ok(const GemmParams& p) {
  return p.H * p.W <= 64 && p.Cin >= 512 && (p.N & 7) == 0 && (p.ldc & 7) == 0 && (!p.res || (p.ld_res & 7) == 0) &&
         (!p.rowbias || (p.ld_rb & 7) == 0) && (p.flags & ~(DM4D_EPI_F32OUT | DM4D_EPI_F32SIDE | DM4D_EPI_H16)) == 0 &&
         ((p.flags & DM4D_EPI_H16) || p.flags == 0);  // the parity precision (F32OUT / F32SIDE without H16) never splits
}

// Workspace of the split strip convolution on a batch of B images: 3 fp32 planes [M][N], 0 where the launch never splits
// (dm4d_conv3x3_ws_bytes; p.flags as the kernels see them: the fp16 precision with DM4D_EPI_H16)
inline size_t strip_ws_bytes(const GemmParams& p, int B) {
  return strip_conv(p) && strip_split_ok(p) ? (size_t)3 * B * p.Ho * p.Wo * p.N * sizeof(float) : 0;
}

// Heuristic (tuned on the UNet shapes at 72x40 latents, profiles/r01_gemm_tune.log)
template <bool CONV>
int choose_cfg(const GemmParams& p) {
  const bool geglu = is_geglu(p);
  if (!k64<CONV>(p)) {  // K-slab 32 register-staged fallback
    const long tiles_big = (long)((p.M + 255) / 256) * ((p.N + (geglu ? 63 : 127)) / (geglu ? 64 : 128));
    if (n128(p)) return tiles_big >= 384 ? 21 : 22;
    return (long)((p.M + 255) / 256) * ((p.N + 63) / 64) >= 384 ? 23 : 24;
  }
  const int bn = geglu ? 64 : 128;  // output columns of a 128-wide B tile
  const long tm256 = (p.M + 255) / 256, tm128 = (p.M + 127) / 128, tn = (p.N + bn - 1) / bn;
  if (!CONV) {
    // N = 320 on a tall problem (level 0: proj_in, attention output projection, proj_out; the feed-forward's output projection when
    // the fused kernel is off): two 160-wide column tiles, no padded third tile -- cold-cache sweep profiles/r03_lin_160_tiles.log:
    // 59.2 vs 70.0 us at K = 320 and CFG batch 32, 85.6 vs 92.8 at 48; 126 vs 141 / 197 vs 200 at K = 1280 (where the 320-wide
    // tiles, ids 46 / 62 of round 2, used to be ahead; 46 stays for inputs the second form's 32-bit offsets cannot address)
    if (!geglu && p.N == 320 && tm256 >= 256) {
      if (lin2_ok(p)) return 69;
      if (p.K >= 1024) return 46;
    }
    // Round 6: the launches of a 2-task stack (CFG batch 64 / 96: 720 / 1080 row tiles of 256 at level 0) -- sweep of every id on those
    // shapes, profiles/r06_gemm_tune_stacks.log: the level-0 QKV projection (N = 960, K = 320) on the 320-wide tile (three column tiles,
    // no padded fourth: 209 -> 181 us, 301 -> 262 us), level 1's feed-forward output projection on the 160-wide one (197 -> 181, 288 -> 276)
    if (!geglu && p.K == 320 && p.N == 960 && tm256 >= 700) return 46;
    if (!geglu && p.N == 640 && p.K >= 2560 && tm256 >= 180 && lin2_ok(p)) return 69;
    // deep-K layers (K >= 1280): the second form (gemm_lin2_kernel), bit-identical, -4..-17 % per launch
    // (profiles/r02_lin2_ab.log): 128x128 tiles with two workgroups per CU wherever they fill the chip, the 8-wave
    // 3-stage 128x128 tile for the few-row, very deep output projections of the deepest level, and the 256x128 K-slab-64
    // tile for that level's GEGLU projection.  Shorter K needs two resident workgroups (a tile is mostly prologue and
    // epilogue): see id 65 below.
    if (lin2_ok(p)) {
      // 256x256 tiles on 8 waves (128x64 per wave: 6 fragment reads feed 8 MFMAs instead of 4 feeding 4), one workgroup per
      // CU.  Chosen from TWO sweeps of every id (all bit-identical): the usual timing loop (profiles/r02_lin_tiles_256.log) and
      // single launches after a cache flush with only the activations re-touched (profiles/r02_lin_cold.log) -- the state a
      // layer meets inside a UNet pass, where this tile's exposed prologue costs more.  It wins both ways on the deep-K wide
      // layers (K >= 1280: GEGLU projection of level 2 182 -> 156 us hot, 176 -> 156 cold; QKV of level 2 at CFG batch 48
      // 95 -> 80 / 98 -> 82) and on the K = 640 ones only when the rounds of 256 tiles are nearly full; at K = 320 the
      // two-workgroup 74 KB tile (id 65) is 8 % ahead cold and stays.
      {
        const long nw = geglu ? 2L * p.N : p.N, tn256 = (nw + 255) / 256, t = tm256 * tn256;
        const double fill = (double)t / (double)(((t + 255) / 256) * 256) * (double)nw / (double)(tn256 * 256);
        if (geglu && ((p.K >= 1280 && fill >= 0.85) || (p.K >= 640 && fill >= 0.95))) return 67;
        // (round 6, second sweep of the stacked launches: id 67 for level 1's GEGLU projection at fill 0.94 and id 61 for level 2's K = 5120
        // output projection were 6-8 % ahead per launch in the timing loop and 0.15 ms BEHIND over the Linear family of a bench step:
        // profiles/r06_stackcfg2.log; not taken)
        if (!geglu && p.K >= 640 && p.N >= 1280 && fill >= 0.85) return 67;
        // one partial round (160-256 tiles) of the N = 1280 projections of level 2 at CFG batch 48: 42 vs 45 us, 122 vs 135 us
        if (!geglu && p.K >= 1280 && p.N == 1280 && t >= 160 && t <= 256) return 67;
      }
      if (geglu) {
        if (tm256 <= 12 && p.K >= 1280) return 61;
      } else if (p.K >= 1280 && p.N >= 640) {
        if (tm128 * ((p.N + 127) / 128) >= 256) return 63;
        if (p.K >= 2560) return 64;
      }
    }
    // Linear layers stream A once with little reuse (K = C or 4C): they are bound by L2->LDS bytes and DMA latency,
    // so the 8-wave 256x128 tile with 2 slabs of DMA in flight wins whenever it still fills the chip (1.2-1.35x)
    const long t = tm256 * tn;  // one 8-wave workgroup per CU => 256 slots per round; avoid a mostly empty last round
    if (t >= 256 && 5 * t >= 4 * ((t + 255) / 256) * 256) {
      // the same 74 KB geometry (two workgroups per CU) in the second form: -2..-9 % on the GEGLU projections of levels 0-2,
      // -9..-16 % on the K = 640 layers of level 1, +-1 % on the narrow K = 320 layers; the wide K = 320 QKV projection
      // (N = 960) is the one shape where it is not ahead at both batch sizes (profiles/r02_lin2_ab.log, id 65 vs auto)
      // (id 61, the 147 KB three-stage tile, for the residual layers with K <= 640 -- ahead in the cold sweep, behind in the timing
      // loop -- measured in a bench step: Linear family 27.6 -> 27.8 ms, profiles/r02_lin_heuristic_cold_ab.log; not taken)
      if (lin2_ok(p) && (geglu || p.K >= 640 || p.N <= 640)) return 65;
      return 14;
    }
  } else {
    // stride-1 convs: the strip kernels stage A once per kernel row (profiles/r01_conv_strip.log)
    if (strip_conv(p) && strip2_ok(p)) {
      if (!n128(p)) {
        // N = 320 on a tall problem (level 0 of the UNet): two 160-wide column tiles, no padded columns and a third of the A re-reads
        // of the 64-wide tile -- 8 waves on 256 rows when the last round of 256 workgroups is at least half full, else 4 waves on
        // 128 rows with two workgroups per CU (-6..-12 % per launch against ids 33 / 35 at CFG batch 32 and 48, cold-cache sweep
        // profiles/r03_strip_160_tiles.log); same K order as every strip kernel, so the choice never changes a result
        if (p.N == 320 && tm256 >= 256) {
          // round 6, stacked launches (profiles/r06_gemm_tune_stacks.log): with 720 / 1080 row tiles the 320-wide tile -- the A strip staged
          // once per kernel row for all of N -- is ahead of the 160-wide ones: 320 -> 320 292 -> 269 us, 960 -> 320 845 -> 758 / 1298 -> 1196,
          // 640 -> 320 570 -> 510 / 874 -> 817 (at CFG batch 32 / 48 the 160-wide tiles stay: r03_strip_160_tiles.log)
          if (tm256 >= 700) return 35;
          const long t2 = tm256 * 2, last = t2 % 256;
          return (last == 0 || last >= 128) ? 37 : 36;
        }
        if (tm128 * ((p.N + 63) / 64) >= 256) return 33;
      } else {
        const long t = tm256 * tn;
        // (round 6, second sweep of the stacked launches, two passes of 12 launches, profiles/r06_gemm_tune_stacks_p1.log / _p2.log: the
        // 160-wide tiles for level 1 (N = 640) and 256x128 for level 2 at CFG batch 96 are 4-7 % ahead per launch and take 0.7 ms off the
        // convolution family of a one-stack-at-a-time pass -- and ADD 0.2-0.3 ms to the bench step with three stacks in flight
        // (profiles/r06_stackcfg3.log): not taken)
        // N = 640 (level 1) when two 320-wide column tiles make ONE nearly full round of 256 workgroups (CFG batch 32: 180): the A strip
        // is read twice instead of five times, -3..-9 % per launch in both cold sweeps (r02_strip_cold.log, r03_strip_160_tiles.log);
        // at batch 48 the same tile needs a second, nearly empty round and loses 20 %
        if (p.N == 640 && p.Cin >= 640 && tm256 * 2 >= 160 && tm256 * 2 <= 256) return 35;
        if (p.N % 256 == 0 && tm256 * (p.N / 256) >= 160) return 34;
        // one partial round of 256x128 tiles against a nearly full round of 128x128 tiles at two workgroups per CU (level 2 at CFG
        // batch 32: 230 vs 450 of 512): the small tile is 4-6 % ahead in both cold-cache sweeps (r02_strip_cold.log, r03_strip_160_tiles.log)
        if (t <= 256 && tm128 * tn >= 384 && tm128 * tn <= 512) return 31;
        if (t >= 200 && 5 * t >= 4 * ((t + 255) / 256) * 256) return 32;
        if (tm128 * tn >= 256) return 31;
      }
    }
    // upsample-fused convs (Upsample2D): the gather reads every input pixel four times, so tiles that cut the A traffic
    // win: 320-wide for N = 640 (578 vs 698-760 us), 16-wave 256x256 for N = 1280 (634 vs 685-740 us); all of these walk K
    // in the same (ky, kx, ci) order as the other gather kernels
    if (p.upsample) {
      if (p.N % 320 == 0 && p.N <= 640 && tm256 >= 64) return 46;
      if (p.N % 256 == 0 && tm256 * (p.N / 256) >= 256) return 20;
    }
    // other convs: 128x128 / 2 workgroups per CU is best except for wide, tall problems
    if (!geglu && p.N % 256 == 0 && tm256 * (p.N / 256) >= 384) return 13;
  }
  if (n128(p)) {
    if (tm128 * tn >= 256) return 1;
    if (geglu) return 3;
    return tm128 * tn >= 200 ? 3 : 4;  // deepest UNet level: shrink the tile until the grid covers the 256 CUs
  }
  return tm256 * ((p.N + 63) / 64) >= 384 ? 2 : 3;
}

// Configuration ids.  AllIds: the fast and the fp16 precision.  ParIds: the parity precision = the PAR = 1 instantiations of gemm.hip, a
// few tile geometries only, since the fast kernels do not carry that epilogue code (22, 24: K-slab 32, register staged, for P V of the
// VAE mid block: K = 3 Lp with Lp a multiple of 32).  launch_by_id walks these lists and instantiates nothing else, in list order.
template <int... I>
using IdList = std::integer_sequence<int, I...>;
using AllIds = IdList<1, 2, 3, 4, 13, 14, 20, 46, 31, 32, 33, 35, 36, 37, 34, 67, 65, 61, 69, 63, 64, 21, 22, 23, 24>;
template <bool CONV>
using ParIds = std::conditional_t<CONV, IdList<33, 32, 31, 1, 3, 4>, IdList<22, 24, 67, 65, 61, 69, 63, 64, 1, 3, 4>>;

template <int... I>
constexpr bool has_id(IdList<I...>, int id) { return ((id == I) || ...); }
constexpr bool par_has_id(bool conv, int id) { return conv ? has_id(ParIds<true>{}, id) : has_id(ParIds<false>{}, id); }

// Parity-precision launches (DM4D_EPI_F32SIDE / DM4D_EPI_SPLITOUT: fp32 side inputs, two-term output): the Linear tiles the fast
// precision picks for this shape (K here is the doubled K of the two-term operand) where PAR = 1 has them, else the tail of the
// heuristic above.  0 = no kernel: a convolution whose Cin is no multiple of 64 (a two-term operand of Cin / 2 channels).
template <bool CONV>
int choose_par(const GemmParams& p) {
  const bool geglu = is_geglu(p);
  const long tm128 = (p.M + 127) / 128, tm256 = (p.M + 255) / 256, tn = (p.N + (geglu ? 63 : 127)) / (geglu ? 64 : 128);
  if (CONV) {
    if (!k64<CONV>(p)) return 0;
    if (strip_conv(p) && strip2_ok(p)) {
      if (!n128(p)) return 33;
      return tm256 * tn >= 200 ? 32 : 31;
    }
  } else {
    if (!k64<CONV>(p)) return n128(p) ? 22 : 24;
    if (lin2_ok(p)) {
      const int id = choose_cfg<false>(p);
      if (id >= 61 && par_has_id(false, id)) return id;
    }
  }
  if (n128(p)) {
    if (tm128 * tn >= 256 || geglu) return 1;
    return tm128 * tn >= 200 ? 3 : 4;
  }
  return 3;
}

// (launch parameters, precision) -> (id, splits).  The strip convolution on small images splits over its 3 kernel rows on 128x128
// tiles (id 31) when the caller brought the workspace; the parity precision never splits.
template <bool CONV>
GemmChoice select_cfg(const GemmParams& p, int prec) {
  if (prec == PREC_PAR) return {choose_par<CONV>(p), 1};
  if (CONV && p.ws && strip_conv(p) && strip_split_ok(p) && strip2_ok(p)) return {31, 3};
  return {choose_cfg<CONV>(p), 1};
}

// Phase-decomposed x2 upsampling convolution, tile as for the stride-1 strips, named by the strip id of the same geometry:
// 32 = 256x128 where a phase alone fills the chip's 256 CUs, 31 = 128x128, 33 = 128x64 for the other channel counts
inline int choose_up2x(const GemmParams& p) {
  const long tm256 = (p.M + 255) / 256;
  if (p.N % 128 == 0) return tm256 * (p.N / 128) >= 200 ? 32 : 31;
  return 33;
}

}  // namespace
