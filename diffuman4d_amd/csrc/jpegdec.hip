// Baseline JPEG files decoded on the device: what libjpeg's default decompression (Pillow's Image.open) gives for a file of the
// supported set (host/jpegdec.py::probe: SOF0, 8 bits, one interleaved Huffman scan without restart markers, grayscale or YCbCr at
// 4:4:4 / 4:2:2 / 4:2:0), for a batch of files of different sizes, samplings and tables.  All of it is integer arithmetic, so the bytes
// are defined exactly (DESIGN.md "Device JPEG decode"; tests/jpegdec_model.py is the same definition in numpy).
//
// Decoder = a fill of the coefficient buffer with zeros and two launches on one stream; launch boundaries are the only ordering
// between workgroups, there are no atomics, and an image's bytes depend on its file alone:
//   entropy  one workgroup per image.  The unstuffed scan has no restart markers, so where a symbol starts is known only by decoding
//            everything before it.  The scan is cut into subsequences of DM4D_JPEGDEC_SUB_BITS bits; DM4D_JPEGDEC_TILE_LANES of them
//            make a tile that is staged in LDS.  Every lane decodes its subsequence from a GUESSED state (bit position = its first bit,
//            block slot 0 of the MCU, DC symbol next) and records the state it leaves with; rounds then re-decode every lane whose
//            predecessor's exit state differs from the state it started from, until a round changes nothing (closed with
//            __syncthreads_or).  Lane 0 starts from the true state carried over from the tile before, so after r rounds lanes 0 .. r
//            are right: a tile needs at most as many rounds as it has lanes, and Huffman codes resynchronise long before that.  A scan of
//            the lanes' finished-block counts gives every lane its first block, and a last pass stores the values as int16 at their
//            natural positions.  When the scan is through, a prefix sum per component turns the DC differences into DC values.
//   pixel    one workgroup per 64 x 64 output tile: dequantisation and jidctint "islow" of the blocks the tile needs (one lane per
//            block; with down-sampled chroma one ring of blocks around the tile is inverted too), samples to LDS, then per pixel the
//            "fancy" triangle up-sampling of the chroma, the 16-bit fixed-point YCbCr -> RGB tables and the store.
// Every loop is bounded by a constant or by the scan's length, never by what the scan's bits say; every read of the scan is masked by
// its length and every coefficient store is below the image's block count.  A file the decoder cannot finish gets a nonzero status.
#include <stdint.h>

#include "common.h"
#include "dm4d.h"
#include "errors.h"
#include "image_common.h"

namespace {

constexpr int kLanes = DM4D_JPEGDEC_TILE_LANES;
constexpr int kSubBits = DM4D_JPEGDEC_SUB_BITS;
constexpr int kSubWords = kSubBits / 32;
constexpr int kTileWords = kLanes * kSubWords;
constexpr int kTileBytes = kTileWords * 4;
// a lane's words are kSubWords + 1 apart in LDS, so lanes that read the same word of their subsequences hit different banks; two more
// words follow the tile, for the window of a symbol that starts in its last bits
constexpr int kTileLds = kTileWords + 2 + (kTileWords + 2) / kSubWords + 1;
constexpr int kPixTile = 64;
constexpr int kPixThreads = 256;
constexpr int64_t kMaxBlocks = 1ll << 25;
static_assert(kLanes == 256 && kSubWords == 32, "the entropy kernel's LDS layout and scans are written for 256 lanes of 32 words");

enum { D_SCAN = 0, D_BYTES, D_H, D_W, D_NCOMP, D_HS, D_VS, D_OUT, D_CHANNELS, D_BLOCK0 };
constexpr int kHuffRec = 304;  // DC bits[16] values[16], AC bits[16] values[256]
constexpr int kQuantAt = 3 * kHuffRec;
static_assert(kQuantAt + 192 == DM4D_JPEGDEC_TABLE_BYTES, "table record");

__device__ const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                        41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                        30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Image {
  int64_t scan, out, block0;
  uint32_t nbytes;
  int h, w, ncomp, hs, vs, channels;
  int nb, mcux, mcus;
};

__host__ __device__ inline Image image_of(const int64_t* desc, int i) {
  const int64_t* d = desc + (int64_t)i * DM4D_JPEGDEC_FIELDS;
  Image im;
  im.scan = d[D_SCAN], im.nbytes = (uint32_t)d[D_BYTES], im.out = d[D_OUT], im.block0 = d[D_BLOCK0];
  im.h = (int)d[D_H], im.w = (int)d[D_W], im.ncomp = (int)d[D_NCOMP], im.hs = (int)d[D_HS], im.vs = (int)d[D_VS];
  im.channels = (int)d[D_CHANNELS];
  im.nb = im.ncomp == 1 ? 1 : im.hs * im.vs + 2;
  im.mcux = (im.w + 8 * im.hs - 1) / (8 * im.hs);
  im.mcus = im.mcux * ((im.h + 8 * im.vs - 1) / (8 * im.vs));
  return im;
}

// -- entropy stage -----------------------------------------------------------------------------------------------------------------------
struct HuffLut {
  uint16_t look[256];   // the next 8 bits -> (length << 8) | symbol of the code they start with; 0 = a longer code or none
  int32_t maxcode[17];  // [l] = the largest code of length l, -1 when there is none
  int32_t valoff[17];   // code c of length l is symbol vals[valoff[l] + c]
  uint8_t vals[256];
};

// Annex C / jdhuff.c: codes in order of length, then of value.  One lane builds one table.
__device__ void build_lut(HuffLut& t, const uint8_t* __restrict__ bits, const uint8_t* __restrict__ vals, int room) {
  for (int i = 0; i < 256; ++i) t.look[i] = 0, t.vals[i] = 0;
  int code = 0, k = 0;
  for (int l = 1; l <= 16; ++l) {
    const int n = bits[l - 1];
    t.maxcode[l] = n ? code + n - 1 : -1;
    t.valoff[l] = k - code;
    for (int i = 0; i < n; ++i) {
      const uint8_t v = k < room ? vals[k] : (uint8_t)0;
      t.vals[k & 255] = v;
      if (l <= 8) {
        const int first = (code << (8 - l)) & 255, cnt = 1 << (8 - l);
        for (int j = 0; j < cnt; ++j) t.look[(first + j) & 255] = (uint16_t)((l << 8) | v);
      }
      ++code, ++k;
    }
    code <<= 1;
  }
}

// the state between two symbols: bit position | block slot in the MCU << 32 | zig-zag index << 40 (0 = the DC symbol is next)
__device__ __forceinline__ uint64_t pack_state(uint32_t p, int b, int k) { return (uint64_t)p | ((uint64_t)b << 32) | ((uint64_t)k << 40); }

__device__ __forceinline__ int tile_at(int w) { return w + (w >> 5); }

struct Writer {
  int16_t* coef;      // the image's blocks
  int64_t block;      // index of the block the entry state is in
  int64_t total;      // blocks of the image
  int status;         // DM4D_JPEGDEC_ST_* seen
  uint32_t done_at;   // bit position at which the image's last block ended
  bool done;
};

// Symbols from (p, b, k) while p < end.  n = blocks finished.  WRITE: the values are stored, errors are recorded and decoding ends
// with the image's last block; otherwise nothing is stored and whatever the bits say is followed (a guessed state decodes garbage).
template <bool WRITE>
__device__ __forceinline__ void run(const uint32_t* __restrict__ tile, uint32_t tile_bit0, const HuffLut* __restrict__ lut, int ncomp, int ny,
                                    int nb, uint32_t& p, int& b, int& k, uint32_t end, int& n, Writer* wr) {
  n = 0;
  for (int it = 0; it < kSubBits; ++it) {  // a symbol is at least one bit
    if (p >= end) break;
    if (WRITE && wr->block + n >= wr->total) break;
    const uint32_t rel = p - tile_bit0;
    const int w = min((int)(rel >> 5), kTileWords), sh = (int)(rel & 31u);
    const uint32_t w0 = tile[tile_at(w)], w1 = tile[tile_at(w + 1)];
    const uint32_t win = sh ? (w0 << sh) | (w1 >> (32 - sh)) : w0;
    const int c = (ncomp == 1 || b < ny) ? 0 : b - ny + 1;
    const HuffLut& t = lut[2 * c + (k != 0)];
    int len = 16, sym = 0;
    bool found = false;
    const uint32_t e = t.look[win >> 24];
    if (e) {
      len = (int)(e >> 8), sym = (int)(e & 255u), found = true;
    } else {
#pragma unroll
      for (int l = 9; l <= 16; ++l) {
        const int code = (int)(win >> (32 - l));
        if (!found && code <= t.maxcode[l]) {
          len = l, sym = t.vals[(t.valoff[l] + code) & 255], found = true;
        }
      }
    }
    if (!found) {
      len = 16, sym = 0;  // a window no code starts: 16 bits are dropped
      if (WRITE) wr->status |= DM4D_JPEGDEC_ST_BAD_CODE;
    }
    const int s = sym & 15;
    int32_t val = 0;
    if (s) {
      const uint32_t v = (win << len) >> (32 - s);  // len + s <= 31
      val = v < (1u << (s - 1)) ? (int32_t)v - (1 << s) + 1 : (int32_t)v;
    }
    if (k == 0) {
      if (WRITE && s) wr->coef[(wr->block + n) * 64] = (int16_t)val;
      k = 1;
    } else {
      const int r = sym >> 4;
      if (s) {
        k += r;
        if (k > 63) {
          if (WRITE) wr->status |= DM4D_JPEGDEC_ST_ZIGZAG;
          k = 64;
        } else {
          if (WRITE) wr->coef[(wr->block + n) * 64 + kZigzag[k]] = (int16_t)val;
          ++k;
        }
      } else if (r == 15) {
        k += 16;
      } else {
        k = 64;  // EOB (libjpeg ends the block at any other run with size 0 too)
      }
    }
    p += (uint32_t)(len + s);
    if (k >= 64) {
      k = 0;
      b = b + 1 < nb ? b + 1 : 0;
      ++n;
      if (WRITE && wr->block + n == wr->total) wr->done_at = p, wr->done = true;
    }
  }
}

// exclusive prefix sum of v over the 256 lanes of the block; total = the block's sum.  Two barriers.
__device__ __forceinline__ int block_excl(int v, int* wave_sum, int& total) {
  const int incl = wave_incl_scan(v);
  if ((threadIdx.x & 63) == 63) wave_sum[threadIdx.x >> 6] = incl;
  __syncthreads();
  int before = 0;
  total = 0;
  for (int w = 0; w < kLanes / 64; ++w) {
    if (w < (int)(threadIdx.x >> 6)) before += wave_sum[w];
    total += wave_sum[w];
  }
  __syncthreads();
  return before + incl - v;
}

__global__ void __launch_bounds__(kLanes) jpegdec_entropy_kernel(const int64_t* __restrict__ desc, const uint8_t* __restrict__ scans,
                                                                 const uint8_t* __restrict__ tabs, int16_t* __restrict__ coef_all,
                                                                 int32_t* __restrict__ status) {
  __shared__ uint32_t tile[kTileLds];
  __shared__ HuffLut lut[6];  // [2 c] the DC table of component c, [2 c + 1] its AC table
  __shared__ uint64_t exit_s[kLanes];
  __shared__ int wave_sum[kLanes / 64];
  __shared__ uint64_t carried_s;
  __shared__ uint32_t done_at_s;
  __shared__ int done_s;
  const Image im = image_of(desc, blockIdx.x);
  const int lane = threadIdx.x;
  const uint8_t* src = scans + im.scan;
  const uint8_t* tab = tabs + (int64_t)blockIdx.x * DM4D_JPEGDEC_TABLE_BYTES;
  int16_t* coef = coef_all + im.block0 * 64;
  const int64_t total_blocks = (int64_t)im.mcus * im.nb;
  const int ny = im.hs * im.vs;
  if (lane < 6) {
    const uint8_t* rec = tab + (lane >> 1) * kHuffRec + ((lane & 1) ? 32 : 0);
    build_lut(lut[lane], rec, rec + 16, (lane & 1) ? 256 : 16);
  }
  if (lane == 0) carried_s = 0, done_s = 0, done_at_s = 0;
  __syncthreads();
  const uint32_t total_bits = im.nbytes * 8u;  // nbytes < 2^28
  const int ntiles = (int)((im.nbytes + (uint32_t)kTileBytes - 1u) / (uint32_t)kTileBytes);
  int64_t carried_blocks = 0;  // the same in every lane
  int st_bits = 0;
  for (int t = 0; t < ntiles; ++t) {
    const uint32_t byte0 = (uint32_t)t * (uint32_t)kTileBytes;
    for (int j = lane; j < kTileWords + 2; j += kLanes) {
      const uint32_t off = byte0 + 4u * (uint32_t)j;
      uint32_t v = 0;
      if (off + 4u <= im.nbytes) {
        v = __builtin_bswap32(*reinterpret_cast<const uint32_t*>(src + off));  // the scan starts on a multiple of 4
      } else if (off < im.nbytes) {
        for (uint32_t i = 0; i < 4u; ++i) v |= off + i < im.nbytes ? (uint32_t)src[off + i] << (24 - 8 * i) : 0u;
      }
      tile[tile_at(j)] = v;  // bits beyond the scan read as zeros
    }
    __syncthreads();
    const uint32_t tile_bit0 = byte0 * 8u;
    const uint32_t start = tile_bit0 + (uint32_t)lane * (uint32_t)kSubBits;
    const bool live = start < total_bits;
    const uint32_t end = min(start + (uint32_t)kSubBits, total_bits);
    const int nlive = (int)min((uint32_t)kLanes, (total_bits - tile_bit0 + (uint32_t)kSubBits - 1u) / (uint32_t)kSubBits);
    uint64_t entry = lane == 0 ? carried_s : pack_state(start, 0, 0);
    int n = 0;
    if (live) {
      uint32_t p = (uint32_t)entry;
      int b = (int)((entry >> 32) & 255u), k = (int)(entry >> 40);
      run<false>(tile, tile_bit0, lut, im.ncomp, ny, im.nb, p, b, k, end, n, nullptr);
      exit_s[lane] = pack_state(p, b, k);
    }
    __syncthreads();
    for (int r = 0; r < kLanes; ++r) {  // round r makes lane r right at the latest
      const uint64_t ne = lane == 0 ? carried_s : exit_s[lane - 1];
      __syncthreads();
      const bool changed = live && ne != entry;
      if (changed) {
        entry = ne;
        uint32_t p = (uint32_t)entry;
        int b = (int)((entry >> 32) & 255u), k = (int)(entry >> 40);
        run<false>(tile, tile_bit0, lut, im.ncomp, ny, im.nb, p, b, k, end, n, nullptr);
        exit_s[lane] = pack_state(p, b, k);
      }
      if (!__syncthreads_or(changed ? 1 : 0)) break;
    }
    int tile_blocks;
    const int before = block_excl(live ? n : 0, wave_sum, tile_blocks);
    if (live) {
      Writer wr{coef, carried_blocks + before, total_blocks, 0, 0u, false};
      uint32_t p = (uint32_t)entry;
      int b = (int)((entry >> 32) & 255u), k = (int)(entry >> 40), n2;
      run<true>(tile, tile_bit0, lut, im.ncomp, ny, im.nb, p, b, k, end, n2, &wr);
      st_bits |= wr.status;
      if (wr.done) done_at_s = wr.done_at, done_s = 1;  // one lane of one tile
    }
    carried_blocks += tile_blocks;
    if (lane == nlive - 1) carried_s = exit_s[lane];
    __syncthreads();  // the tile and the exit states are rewritten next
  }
  // DC differences -> DC values: a prefix sum per component over the blocks in scan order (wrapping int32, truncated to int16 as
  // libjpeg's JCOEF is)
  __threadfence_block();
  __syncthreads();
  int carry[3] = {0, 0, 0};
  for (int m0 = 0; m0 < im.mcus; m0 += kLanes) {
    const int m = m0 + lane;
    int sum[3] = {0, 0, 0};
    int16_t* mcu = coef + (int64_t)m * im.nb * 64;
    if (m < im.mcus)
      for (int s = 0; s < im.nb; ++s) sum[(im.ncomp == 1 || s < ny) ? 0 : s - ny + 1] += mcu[s * 64];
    int before[3];
    for (int c = 0; c < im.ncomp; ++c) {
      int total;
      before[c] = carry[c] + block_excl(sum[c], wave_sum, total);
      carry[c] += total;
    }
    if (m < im.mcus)
      for (int s = 0; s < im.nb; ++s) {
        const int c = (im.ncomp == 1 || s < ny) ? 0 : s - ny + 1;
        before[c] += mcu[s * 64];
        mcu[s * 64] = (int16_t)before[c];
      }
  }
  int st = 0;
  for (int bit = 1; bit <= DM4D_JPEGDEC_ST_ZIGZAG; bit <<= 1)
    if (__syncthreads_or(st_bits & bit)) st |= bit;
  if (lane == 0) {
    // the scan ends early (not every block was reached) or has data left over (the last block does not end in the last byte)
    if (!done_s || ((done_at_s + 7u) >> 3) != im.nbytes) st |= DM4D_JPEGDEC_ST_END;
    status[blockIdx.x] = st;
  }
}

// -- pixel stage -------------------------------------------------------------------------------------------------------------------------
// jidctint.c jpeg_idct_islow, one pass over eight values, CONST_BITS 13.  Unsigned arithmetic wraps: pass 1 (SHIFT 11) is exact in 32
// bits for inputs in [-8192, 8191], and of pass 2 (SHIFT 18) only bits 18 .. 27 of each sum are used (DESIGN.md "Device JPEG decode").
template <int SHIFT>
__device__ __forceinline__ void idct8(uint32_t (&d)[8]) {
  uint32_t z2 = d[2], z3 = d[6];
  uint32_t z1 = (z2 + z3) * 4433u;
  uint32_t tmp2 = z1 - z3 * 15137u;
  uint32_t tmp3 = z1 + z2 * 6270u;
  uint32_t tmp0 = (d[0] + d[4]) << 13, tmp1 = (d[0] - d[4]) << 13;
  const uint32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = d[7], tmp1 = d[5], tmp2 = d[3], tmp3 = d[1];
  z1 = tmp0 + tmp3, z2 = tmp1 + tmp2, z3 = tmp0 + tmp2;
  uint32_t z4 = tmp1 + tmp3;
  const uint32_t z5 = (z3 + z4) * 9633u;
  tmp0 *= 2446u, tmp1 *= 16819u, tmp2 *= 25172u, tmp3 *= 12299u;
  z1 = 0u - z1 * 7373u, z2 = 0u - z2 * 20995u, z3 = z5 - z3 * 16069u, z4 = z5 - z4 * 3196u;
  tmp0 += z1 + z3, tmp1 += z2 + z4, tmp2 += z2 + z3, tmp3 += z1 + z4;
  constexpr uint32_t half = 1u << (SHIFT - 1);
  const uint32_t o[8] = {tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3};
#pragma unroll
  for (int i = 0; i < 8; ++i) d[i] = (uint32_t)((int32_t)(o[i] + half) >> SHIFT);
}

// libjpeg's IDCT range-limit table on v & 1023
__device__ __forceinline__ uint32_t range_limit(uint32_t v) {
  v &= 1023u;
  return v < 128u ? v + 128u : v < 512u ? 255u : v < 896u ? 0u : v - 896u;
}

struct Comp {
  int fx, fy;    // the component is down-sampled by these
  int dw, dh;    // its plane, cut to the down-sampled image
  int bx0, by0;  // the first block column / row of the tile's region of it (may be -1)
  int nbx, nby;  // blocks of the region
  int slot0;     // its first block slot in an MCU
};

__device__ __forceinline__ Comp comp_of(const Image& im, int c, int x0, int y0) {
  Comp cp;
  cp.fx = c == 0 ? 1 : im.hs, cp.fy = c == 0 ? 1 : im.vs;
  cp.dw = (im.w + cp.fx - 1) / cp.fx, cp.dh = (im.h + cp.fy - 1) / cp.fy;
  cp.bx0 = x0 / (8 * cp.fx) - (cp.fx == 2), cp.by0 = y0 / (8 * cp.fy) - (cp.fy == 2);
  cp.nbx = cp.fx == 2 ? 6 : 8, cp.nby = cp.fy == 2 ? 6 : 8;
  cp.slot0 = c == 0 ? 0 : im.hs * im.vs + c - 1;
  return cp;
}

__global__ void __launch_bounds__(kPixThreads) jpegdec_pixel_kernel(const int64_t* __restrict__ desc, const uint8_t* __restrict__ tabs,
                                                                    const int16_t* __restrict__ coef_all, uint8_t* __restrict__ out_all,
                                                                    int32_t* __restrict__ status) {
  __shared__ uint8_t plane[3][kPixTile * kPixTile];  // a component's region of samples, rows of kPixTile bytes
  const Image im = image_of(desc, blockIdx.y);
  const int tiles_x = (im.w + kPixTile - 1) / kPixTile;
  const int tiles = tiles_x * ((im.h + kPixTile - 1) / kPixTile);
  if ((int)blockIdx.x >= tiles) return;
  const int x0 = ((int)blockIdx.x % tiles_x) * kPixTile, y0 = ((int)blockIdx.x / tiles_x) * kPixTile;
  const uint8_t* qtab = tabs + (int64_t)blockIdx.y * DM4D_JPEGDEC_TABLE_BYTES + kQuantAt;
  const int16_t* coef = coef_all + im.block0 * 64;
  // the blocks to invert: 64 of the luma, then those of the two chroma regions (the same count each)
  const Comp chroma = comp_of(im, 1, x0, y0);
  const int per_chroma = im.ncomp == 1 ? 0 : chroma.nbx * chroma.nby;
  bool out_of_range = false;
  for (int i = threadIdx.x; i < 64 + 2 * per_chroma; i += kPixThreads) {
    const int c = i < 64 ? 0 : i < 64 + per_chroma ? 1 : 2;
    const Comp cp = comp_of(im, c, x0, y0);
    const int j = c == 0 ? i : i - 64 - (c - 1) * per_chroma;
    const int ry = j / cp.nbx, rx = j - ry * cp.nbx;
    const int bx = cp.bx0 + rx, by = cp.by0 + ry;
    if (bx < 0 || by < 0 || bx >= (cp.dw + 7) / 8 || by >= (cp.dh + 7) / 8) continue;  // no sample of it is read
    const int ch = im.hs / cp.fx, cv = im.vs / cp.fy;  // the component's blocks in an MCU
    const int64_t blk = ((int64_t)(by / cv) * im.mcux + bx / ch) * im.nb + cp.slot0 + (by % cv) * ch + bx % ch;
    const U4* src = reinterpret_cast<const U4*>(coef + blk * 64);
    const uint8_t* q = qtab + 64 * c;
    uint32_t ws[64];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const U4 v = src[r];
      const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int32_t cf = (int16_t)(wd[e >> 1] >> (16 * (e & 1)));
        const int32_t dq = cf * (int32_t)q[r * 8 + e];
        out_of_range |= dq < -8192 || dq > 8191;
        ws[r * 8 + e] = (uint32_t)dq;
      }
    }
#pragma unroll
    for (int col = 0; col < 8; ++col) {
      uint32_t d[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) d[r] = ws[r * 8 + col];
      idct8<11>(d);
#pragma unroll
      for (int r = 0; r < 8; ++r) ws[r * 8 + col] = d[r];
    }
    uint8_t* dst = plane[c] + (ry * 8) * kPixTile + rx * 8;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      uint32_t d[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) d[e] = ws[r * 8 + e];
      idct8<18>(d);
      uint32_t lo = 0, hi = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) lo |= range_limit(d[e]) << (8 * e), hi |= range_limit(d[4 + e]) << (8 * e);
      *reinterpret_cast<uint32_t*>(dst + r * kPixTile) = lo;
      *reinterpret_cast<uint32_t*>(dst + r * kPixTile + 4) = hi;
    }
  }
  if (out_of_range) status[blockIdx.y] = DM4D_JPEGDEC_ST_RANGE;  // every lane that stores, stores this value
  __syncthreads();
  uint8_t* out = out_all + im.out;
  for (int i = threadIdx.x; i < kPixTile * kPixTile; i += kPixThreads) {
    const int x = x0 + (i & (kPixTile - 1)), y = y0 + i / kPixTile;
    if (x >= im.w || y >= im.h) continue;
    const int32_t yy = plane[0][(y - y0) * kPixTile + (x - x0)];
    uint8_t* dst = out + ((int64_t)y * im.w + x) * im.channels;
    if (im.ncomp == 1) {
      dst[0] = (uint8_t)yy;
      if (im.channels == 3) dst[1] = (uint8_t)yy, dst[2] = (uint8_t)yy;
      continue;
    }
    int32_t cc[2];
#pragma unroll
    for (int c = 1; c <= 2; ++c) {
      const Comp cp = comp_of(im, c, x0, y0);
      // sample (sy, sx) of the cut plane is pl[at + sy * kPixTile + sx]
      const uint8_t* pl = plane[c];
      const int at = -(cp.by0 * 8) * kPixTile - cp.bx0 * 8;
      const int cx = x / cp.fx, cy = y / cp.fy;
      int32_t v;
      if (cp.fx == 1 || cp.dw <= 2) {  // full size, or too narrow for the triangle filter: replication
        v = pl[at + cy * kPixTile + cx];
      } else if (cp.fy == 1) {  // h2v1
        const int32_t s = pl[at + cy * kPixTile + cx];
        if (x & 1) v = cx == cp.dw - 1 ? s : (3 * s + pl[at + cy * kPixTile + cx + 1] + 2) >> 2;
        else v = cx == 0 ? s : (3 * s + pl[at + cy * kPixTile + cx - 1] + 1) >> 2;
      } else {  // h2v2: three parts of the nearer row and one of the farther, then the same along the row
        const int far = (y & 1) ? min(cy + 1, cp.dh - 1) : max(cy - 1, 0);
        const uint8_t* rn = pl + (at + cy * kPixTile);
        const uint8_t* rf = pl + (at + far * kPixTile);
        const int32_t cur = 3 * rn[cx] + rf[cx];
        if (x & 1) v = cx == cp.dw - 1 ? (4 * cur + 7) >> 4 : (3 * cur + 3 * rn[cx + 1] + rf[cx + 1] + 7) >> 4;
        else v = cx == 0 ? (4 * cur + 8) >> 4 : (3 * cur + 3 * rn[cx - 1] + rf[cx - 1] + 8) >> 4;
      }
      cc[c - 1] = v - 128;
    }
    // jdcolor.c: FIX(x) = (int)(x * 65536 + 0.5)
    const int32_t r = yy + ((91881 * cc[1] + 32768) >> 16);
    const int32_t b = yy + ((116130 * cc[0] + 32768) >> 16);
    const int32_t g = yy + ((-22554 * cc[0] + 32768 - 46802 * cc[1]) >> 16);
    dst[0] = (uint8_t)min(max(r, 0), 255), dst[1] = (uint8_t)min(max(g, 0), 255), dst[2] = (uint8_t)min(max(b, 0), 255);
  }
}

bool size_ok(int64_t v) { return v >= 1 && v <= 65535; }

// libjpeg's jpeg_make_d_derived_tbl: no code may overflow its length; DC categories are at most 15
bool huff_ok(const uint8_t* bits, const uint8_t* vals, int room, bool dc) {
  int64_t code = 0;
  int cnt = 0;
  for (int l = 1; l <= 16; ++l) {
    code += bits[l - 1], cnt += bits[l - 1];
    if (code > (1ll << l)) return false;
    code <<= 1;
  }
  if (cnt > room) return false;
  if (dc)
    for (int i = 0; i < cnt; ++i)
      if (vals[i] > 15) return false;
  return true;
}

}  // namespace

extern "C" size_t dm4d_jpeg_decode_ws_bytes(int64_t total_blocks, int n) {
  if (total_blocks <= 0 || total_blocks > kMaxBlocks || n <= 0 || n > 65535) return 0;
  return (size_t)(total_blocks * 128);
}

extern "C" int dm4d_jpeg_decode_u8(void* stream, const void* scans, int64_t scans_bytes, const int64_t* desc_host, const int64_t* desc_dev,
                                   int n, const uint8_t* tab_host, const uint8_t* tab_dev, void* workspace, int64_t workspace_bytes, void* out,
                                   int64_t out_bytes, int32_t* status) {
  if (!scans || !desc_host || !desc_dev || !tab_host || !tab_dev || !workspace || !out || !status)
    return dm4d_set_error(DM4D_ERR_ARG, "jpeg_decode: null pointer");
  if (n <= 0 || n > 65535 || scans_bytes <= 0 || out_bytes <= 0) return dm4d_set_error(DM4D_ERR_ARG, "jpeg_decode: empty or oversized batch");
  if (((uintptr_t)workspace & 15) || ((uintptr_t)scans & 3) || ((uintptr_t)status & 3))
    return dm4d_set_error(DM4D_ERR_ARG, "jpeg_decode: workspace must be 16-byte aligned, scans and status 4-byte");
  int64_t block0 = 0, max_tiles = 0;
  for (int i = 0; i < n; ++i) {
    const int64_t* d = desc_host + (int64_t)i * DM4D_JPEGDEC_FIELDS;
    if (!size_ok(d[D_H]) || !size_ok(d[D_W])) return dm4d_set_error(DM4D_ERR_ARG, "jpeg_decode: a dimension outside 1..65535 in a descriptor");
    const int64_t nc = d[D_NCOMP], hs = d[D_HS], vs = d[D_VS], chn = d[D_CHANNELS];
    if (!((nc == 1 && hs == 1 && vs == 1) || (nc == 3 && ((hs == 2 && vs == 2) || (hs == 2 && vs == 1) || (hs == 1 && vs == 1)))))
      return dm4d_set_error(DM4D_ERR_ARG, "jpeg_decode: a descriptor's components or sampling factors are not of the supported set");
    if (!(chn == 3 || (chn == 1 && nc == 1))) return dm4d_set_error(DM4D_ERR_ARG, "jpeg_decode: output channels must be 3, or 1 for grayscale");
    if (d[D_BYTES] < 1 || d[D_BYTES] >= DM4D_JPEGDEC_MAX_SCAN_BYTES || d[D_SCAN] < 0 || (d[D_SCAN] & 3) || d[D_SCAN] > scans_bytes ||
        d[D_BYTES] > scans_bytes - d[D_SCAN])
      return dm4d_set_error(DM4D_ERR_ARG, "jpeg_decode: a scan is empty, too long, misaligned or outside the scan buffer");
    if (d[D_OUT] < 0 || d[D_OUT] > out_bytes || d[D_H] * d[D_W] * chn > out_bytes - d[D_OUT])
      return dm4d_set_error(DM4D_ERR_ARG, "jpeg_decode: an image lies outside the output buffer");
    for (int f = D_BLOCK0 + 1; f < DM4D_JPEGDEC_FIELDS; ++f)
      if (d[f] != 0) return dm4d_set_error(DM4D_ERR_ARG, "jpeg_decode: a descriptor's spare fields must be zero");
    if (d[D_BLOCK0] != block0) return dm4d_set_error(DM4D_ERR_ARG, "jpeg_decode: a descriptor's first block is not the running sum");
    const Image im = image_of(desc_host, i);
    block0 += (int64_t)im.mcus * im.nb;
    if (block0 > kMaxBlocks) return dm4d_set_error(DM4D_ERR_ARG, "jpeg_decode: too many blocks in one batch");
    const uint8_t* t = tab_host + (int64_t)i * DM4D_JPEGDEC_TABLE_BYTES;
    for (int c = 0; c < 3; ++c)
      if (!huff_ok(t + c * kHuffRec, t + c * kHuffRec + 16, 16, true) || !huff_ok(t + c * kHuffRec + 32, t + c * kHuffRec + 48, 256, false))
        return dm4d_set_error(DM4D_ERR_ARG, "jpeg_decode: a Huffman table overflows its code lengths or names a DC category above 15");
    const int64_t tiles = ((d[D_W] + kPixTile - 1) / kPixTile) * ((d[D_H] + kPixTile - 1) / kPixTile);
    if (tiles > max_tiles) max_tiles = tiles;
  }
  if (workspace_bytes < block0 * 128) return dm4d_set_error(DM4D_ERR_ARG, "jpeg_decode: workspace too small (dm4d_jpeg_decode_ws_bytes)");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(workspace, 0, (size_t)(block0 * 128), st) != hipSuccess)
    return dm4d_set_error(DM4D_ERR_LAUNCH, "jpeg_decode: hipMemsetAsync of the coefficient buffer failed");
  hipLaunchKernelGGL(jpegdec_entropy_kernel, dim3((unsigned)n), dim3(kLanes), 0, st, desc_dev, (const uint8_t*)scans, tab_dev,
                     (int16_t*)workspace, status);
  int rc = dm4d_check_launch("jpegdec_entropy_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(jpegdec_pixel_kernel, dim3((unsigned)max_tiles, (unsigned)n), dim3(kPixThreads), 0, st, desc_dev, tab_dev,
                     (const int16_t*)workspace, (uint8_t*)out, status);
  return dm4d_check_launch("jpegdec_pixel_kernel");
}
