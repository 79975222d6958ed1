// Result images on the device: restore_cropped_image (image_utils.py:62-93) and the entropy-coded segment of the baseline JPEG that
// Image.save(path, quality=q) writes (sampling_utils.py:95-114), for a batch of RGB uint8 HWC images of different sizes.
//
// The file is libjpeg's default for an RGB image: YCbCr 4:2:0, jfdctint "islow", the Annex-K quantisation tables scaled by the quality,
// the Annex-K Huffman tables, one interleaved scan (Y00 Y01 Y10 Y11 Cb Cr per 16 x 16 MCU), no restart markers.  All of it is integer
// arithmetic, so the bytes are defined exactly (DESIGN.md "Device JPEG"; tests/jpeg_model.py is the same definition in numpy).
//
// Encoder = eight launches on one stream for the whole batch; launch boundaries are the only ordering between workgroups:
//   coef    one wave per MCU: colour conversion, chroma downsample, level shift, two DCT passes in LDS (6 blocks x 8 rows = 48 lanes),
//           quantisation, zig-zag; int16 coefficients to the workspace
//   size    one wave per MCU, one lane per zig-zag coefficient of a block: __ballot(coef != 0) gives the zero runs, a wave prefix sum
//           the bit position of every symbol; writes the MCU's bit length and its first 8 bits ("head bits").  The DC predictor is read
//           from the coefficient workspace (the previous block of the component in scan order), never carried
//   scan    one block per image: bit lengths -> bit positions; bytes of the unstuffed scan
//   emit    one wave per MCU: the symbols again, OR-ed into LDS at their positions, then every byte that STARTS in this MCU is stored;
//           an MCU is at least 32 bits, so a byte is shared by at most two, and the last byte takes its trailing bits from the next
//           MCU's head bits (1-bits after the last MCU)
//   count   0xFF bytes per DM4D_JPEG_CHUNK bytes of the unstuffed scan;  scan: one block per image;  offsets: the images' places in the blob
//   stuff   FF -> FF 00 into the blob
// Every position comes from a scan; the only atomics are LDS-local ORs inside one wave's buffer.
//
// Crop restore = Pillow's two-pass bicubic resize by the one definition of its rule in image_common.h (coefficient tables from
// host/resample.py), pasted onto a white canvas.
#include <stdint.h>

#include "common.h"
#include "dm4d.h"
#include "errors.h"
#include "image_common.h"
#include "stripe_emit.h"

namespace {

constexpr int kWave = 64;
constexpr int kScanThreads = 1024;
constexpr int kStuffThreads = DM4D_JPEG_CHUNK / 16;  // one lane per 16 bytes
constexpr int kMcuWords = 320;                       // LDS words of one MCU's bit stream: 7 + 9948 bits and two words of slack
constexpr int64_t kMcuBits = 9948;                   // see dm4d.h

enum { J_SPACE = 0, J_PIX, J_H, J_W, J_MCU0, J_CHUNK0 };
enum { R_SRC = 0, R_H, R_W, R_CT, R_CL, R_CH, R_CW, R_CANVAS_H, R_CANVAS_W, R_HTAB, R_HK, R_VTAB, R_VK, R_SCRATCH, R_DST };

// -- tables ----------------------------------------------------------------------------------------------------------------------------
struct HuffTab {
  uint32_t e[256];  // symbol -> (length << 16) | code; 0 = the table has no such symbol
};

// Annex C: codes in order of length, then of value
constexpr HuffTab make_tab(const uint8_t (&bits)[16], const uint8_t* vals) {
  HuffTab t{};
  uint32_t code = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < bits[len - 1]; ++i) t.e[vals[k++]] = ((uint32_t)len << 16) | code++;
    code <<= 1;
  }
  return t;
}

// Annex K.3 - K.6
constexpr uint8_t kDcLumaBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr uint8_t kDcChromaBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
constexpr uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t kAcLumaBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
constexpr uint8_t kAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
    0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
    0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
    0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
    0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
    0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};
constexpr uint8_t kAcChromaBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
constexpr uint8_t kAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
    0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
    0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
    0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
    0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
    0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};

// [0] luma, [1] chroma
__device__ const HuffTab kDc[2] = {make_tab(kDcLumaBits, kDcVals), make_tab(kDcChromaBits, kDcVals)};
__device__ const HuffTab kAc[2] = {make_tab(kAcLumaBits, kAcLumaVals), make_tab(kAcChromaBits, kAcChromaVals)};

// natural (row-major) index of the k-th coefficient of the scan
__device__ const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                        41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                        30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Image {
  const uint8_t* pix;
  int h, w, mx, mcus;
  int64_t mcu0, chunk0;
};

__device__ __forceinline__ Image image_of(const int64_t* __restrict__ desc, int i, const uint8_t* pixels, const uint8_t* canvases) {
  const int64_t* d = desc + (int64_t)i * DM4D_JPEG_FIELDS;
  Image im;
  im.pix = (d[J_SPACE] ? canvases : pixels) + d[J_PIX];
  im.h = (int)d[J_H], im.w = (int)d[J_W];
  im.mx = (im.w + 15) >> 4;
  im.mcus = im.mx * ((im.h + 15) >> 4);
  im.mcu0 = d[J_MCU0], im.chunk0 = d[J_CHUNK0];
  return im;
}

// -- coefficients ------------------------------------------------------------------------------------------------------------------------
// jfdctint.c, one pass over eight values: CONST_BITS 13, PASS1_BITS 2
template <bool FIRST>
__device__ __forceinline__ void dct8(int32_t (&d)[8]) {
  constexpr int n = FIRST ? 11 : 15;
  const int32_t t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
  const int32_t t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
  const int32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  if (FIRST) {
    d[0] = (t10 + t11) << 2;
    d[4] = (t10 - t11) << 2;
  } else {
    d[0] = (t10 + t11 + 2) >> 2;
    d[4] = (t10 - t11 + 2) >> 2;
  }
  constexpr int32_t rnd = 1 << (n - 1);
  int32_t z1 = (t12 + t13) * 4433;
  d[2] = (z1 + t13 * 6270 + rnd) >> n;
  d[6] = (z1 - t12 * 15137 + rnd) >> n;
  z1 = t4 + t7;
  int32_t z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int32_t z5 = (z3 + z4) * 9633;
  const int32_t m4 = t4 * 2446, m5 = t5 * 16819, m6 = t6 * 25172, m7 = t7 * 12299;
  z1 = -z1 * 7373, z2 = -z2 * 20995, z3 = -z3 * 16069 + z5, z4 = -z4 * 3196 + z5;
  d[7] = (m4 + z1 + z3 + rnd) >> n;
  d[5] = (m5 + z2 + z4 + rnd) >> n;
  d[3] = (m6 + z2 + z3 + rnd) >> n;
  d[1] = (m7 + z1 + z4 + rnd) >> n;
}

__global__ void __launch_bounds__(kWave) jpeg_coef_kernel(const int64_t* __restrict__ desc, const uint8_t* __restrict__ pixels,
                                                          const uint8_t* __restrict__ canvases, const uint16_t* __restrict__ qtab,
                                                          int16_t* __restrict__ coef) {
  __shared__ int32_t s[6][64];
  const Image im = image_of(desc, blockIdx.y, pixels, canvases);
  const int m = blockIdx.x;
  if (m >= im.mcus) return;
  const int lane = threadIdx.x;
  const int mcy = m / im.mx, mcx = m - mcy * im.mx;
  const int h = im.h, w = im.w;
  {  // luma: a lane converts 4 pixels of one row; rows and columns beyond the image repeat the last one
    const int row = lane >> 2, c0 = (lane & 3) * 4;
    const int y = min(mcy * 16 + row, h - 1);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = c0 + j;
      const int x = min(mcx * 16 + c, w - 1);
      const uint8_t* p = im.pix + ((int64_t)y * w + x) * 3;
      const int32_t r = p[0], g = p[1], b = p[2];
      s[(row >> 3) * 2 + (c >> 3)][(row & 7) * 8 + (c & 7)] = ((19595 * r + 38470 * g + 7471 * b + 32768) >> 16) - 128;
    }
  }
  {  // chroma: a lane makes one sample of each plane from 2 x 2 pixels.  Columns repeat the last one BEFORE the downsample; rows are
     // padded to an even count only, and it is the downsampled last row that repeats
    const int cy = lane >> 3, cx = lane & 7;
    const int gcy = min(mcy * 8 + cy, ((h + 1) >> 1) - 1), gcx = mcx * 8 + cx;
    const int ry[2] = {min(2 * gcy, h - 1), min(2 * gcy + 1, h - 1)};
    const int rx[2] = {min(2 * gcx, w - 1), min(2 * gcx + 1, w - 1)};
    int32_t cb = 0, cr = 0;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const uint8_t* p = im.pix + ((int64_t)ry[a] * w + rx[e]) * 3;
        const int32_t r = p[0], g = p[1], b = p[2];
        cb += (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
        cr += (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
      }
    const int32_t bias = 1 + (cx & 1);  // 1, 2, 1, 2, ... along output columns (an MCU starts at an even one)
    s[4][lane] = ((cb + bias) >> 2) - 128;
    s[5][lane] = ((cr + bias) >> 2) - 128;
  }
  __syncthreads();
  const int blk = lane >> 3, line = lane & 7;
  if (lane < 48) {  // rows
    int32_t d[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = s[blk][line * 8 + i];
    dct8<true>(d);
#pragma unroll
    for (int i = 0; i < 8; ++i) s[blk][line * 8 + i] = d[i];
  }
  __syncthreads();
  if (lane < 48) {  // columns
    int32_t d[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = s[blk][i * 8 + line];
    dct8<false>(d);
#pragma unroll
    for (int i = 0; i < 8; ++i) s[blk][i * 8 + line] = d[i];
  }
  __syncthreads();
  // quantise (the DCT's output carries a factor 8) in zig-zag order: lane = position in the scan
  const int nat = kZigzag[lane];
  int32_t v[6];
#pragma unroll
  for (int b = 0; b < 6; ++b) {
    const int32_t c = s[b][nat];
    const uint32_t q8 = (uint32_t)qtab[(b >= 4 ? 64 : 0) + nat] * 8u;
    const int32_t a = (int32_t)(((uint32_t)(c < 0 ? -c : c) + (q8 >> 1)) / q8);
    v[b] = c < 0 ? -a : a;
  }
  // a luma block outside the component is not a DCT of repeated pixels: zero AC, and the DC of the block before it in the MCU
  const int bw = (w + 7) >> 3, bh = (h + 7) >> 3;
#pragma unroll
  for (int b = 1; b < 4; ++b)
    if (2 * mcx + (b & 1) >= bw || 2 * mcy + (b >> 1) >= bh) v[b] = lane == 0 ? v[b - 1] : 0;
  int16_t* out = coef + (im.mcu0 + m) * 384 + lane;
#pragma unroll
  for (int b = 0; b < 6; ++b) out[b * 64] = (int16_t)v[b];
}

// -- entropy coding ----------------------------------------------------------------------------------------------------------------------
// What lane `lane` (= zig-zag position) of a block emits, left-aligned in 64 bits: lane 0 the DC difference, a non-zero AC lane its
// ZRLs + run/size code + value bits (at most 3 x 11 + 16 + 10 = 59 bits), lane 63 the EOB when the block ends in zeros.
__device__ __forceinline__ void block_symbol(int lane, int32_t v, int32_t pred, int chroma, uint64_t& sym, int& len) {
  const unsigned long long nz = __ballot(v != 0) & ~1ull;  // AC only
  uint64_t s = 0;
  int n = 0;
  if (lane == 0) {
    const int32_t d = v - pred;
    const int nb = min(32 - __clz(d < 0 ? -d : d), 11);
    const uint32_t e = kDc[chroma].e[nb];
    s = e & 0xffffu, n = (int)(e >> 16);
    s = (s << nb) | ((uint32_t)(d < 0 ? d - 1 : d) & ((1u << nb) - 1u)), n += nb;
  } else if (v != 0) {
    const unsigned long long below = nz & ((1ull << lane) - 1ull);
    const int prev = below ? 63 - __clzll((long long)below) : 0;
    const int run = lane - 1 - prev;
    const uint32_t zrl = kAc[chroma].e[0xf0];
    for (int i = 0; i < (run >> 4); ++i) s = (s << (zrl >> 16)) | (zrl & 0xffffu), n += (int)(zrl >> 16);
    const int nb = min(32 - __clz(v < 0 ? -v : v), 10);
    const uint32_t e = kAc[chroma].e[((run & 15) << 4) | nb];
    s = (s << (e >> 16)) | (e & 0xffffu), n += (int)(e >> 16);
    s = (s << nb) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << nb) - 1u)), n += nb;
  } else if (lane == 63) {
    const uint32_t e = kAc[chroma].e[0];
    s = e & 0xffffu, n = (int)(e >> 16);
  }
  sym = n ? s << (64 - n) : 0ull;
  len = n;
}

// DC of the previous block of the same component in scan order (0 at the start of an image)
__device__ __forceinline__ int32_t dc_pred(const int16_t* __restrict__ mcu, int m, int b) {
  if (b >= 1 && b <= 3) return mcu[(b - 1) * 64];
  if (m == 0) return 0;
  return mcu[-384 + (b == 0 ? 3 : b) * 64];
}

// exclusive prefix sum of `len` over the wave; total = the wave's sum
__device__ __forceinline__ int wave_excl(int len, int& total) {
  const int s = wave_incl_scan(len);
  total = __shfl(s, 63);
  return s - len;
}

__global__ void __launch_bounds__(kWave) jpeg_size_kernel(const int64_t* __restrict__ desc, const int16_t* __restrict__ coef,
                                                          uint32_t* __restrict__ bits, uint32_t* __restrict__ head) {
  const Image im = image_of(desc, blockIdx.y, nullptr, nullptr);
  const int m = blockIdx.x;
  if (m >= im.mcus) return;
  const int lane = threadIdx.x;
  const int16_t* mcu = coef + (im.mcu0 + m) * 384;
  int pos = 0;
  uint32_t first = 0;
  for (int b = 0; b < 6; ++b) {
    uint64_t sym;
    int len, total;
    block_symbol(lane, mcu[b * 64 + lane], dc_pred(mcu, m, b), b >= 4, sym, len);
    const int at = pos + wave_excl(len, total);
    if (pos < 8) {  // the same for every lane
      uint32_t c = (len && at < 8) ? (uint32_t)(sym >> 56) >> at : 0u;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) c |= __shfl_xor(c, off);
      first |= c;
    }
    pos += total;
  }
  if (lane == 0) {
    bits[im.mcu0 + m] = (uint32_t)pos;
    head[im.mcu0 + m] = first;
  }
}

// bit lengths of an image's MCUs -> bit positions; nbytes[i] = bytes of its unstuffed scan (the last one padded)
__global__ void __launch_bounds__(kScanThreads) jpeg_scan_bits_kernel(const int64_t* __restrict__ desc, uint32_t* __restrict__ bits,
                                                                      int64_t* __restrict__ nbytes) {
  const Image im = image_of(desc, blockIdx.x, nullptr, nullptr);
  const uint32_t total = block_excl_scan_inplace<uint32_t, kScanThreads>(bits + im.mcu0, im.mcus);
  if (threadIdx.x == 0) nbytes[blockIdx.x] = ((int64_t)total + 7) >> 3;
}

__global__ void __launch_bounds__(kWave) jpeg_emit_kernel(const int64_t* __restrict__ desc, const int16_t* __restrict__ coef,
                                                          const uint32_t* __restrict__ bitpos, const uint32_t* __restrict__ head,
                                                          uint8_t* __restrict__ raw) {
  __shared__ uint32_t buf[kMcuWords];
  const Image im = image_of(desc, blockIdx.y, nullptr, nullptr);
  const int m = blockIdx.x;
  if (m >= im.mcus) return;
  const int lane = threadIdx.x;
  const int16_t* mcu = coef + (im.mcu0 + m) * 384;
  for (int i = lane; i < kMcuWords; i += kWave) buf[i] = 0;
  __syncthreads();
  const uint32_t start = bitpos[im.mcu0 + m];
  int pos = (int)(start & 7u);  // LDS byte j = byte (start >> 3) + j of the image's scan
  for (int b = 0; b < 6; ++b) {
    uint64_t sym;
    int len, total;
    block_symbol(lane, mcu[b * 64 + lane], dc_pred(mcu, m, b), b >= 4, sym, len);
    const int at = pos + wave_excl(len, total);
    const int w = at >> 5, sh = at & 31;
    if (len && w + 2 < kMcuWords) {
      const uint32_t hi = (uint32_t)(sym >> 32), lo = (uint32_t)sym;
      const uint32_t a0 = hi >> sh;
      const uint32_t a1 = sh ? (hi << (32 - sh)) | (lo >> sh) : lo;
      const uint32_t a2 = sh ? lo << (32 - sh) : 0u;
      if (a0) atomicOr(&buf[w], a0);
      if (a1) atomicOr(&buf[w + 1], a1);
      if (a2) atomicOr(&buf[w + 2], a2);
    }
    pos += total;
  }
  __syncthreads();
  const int end = min(pos, kMcuWords * 32 - 64);
  const int first = (start & 7u) ? 1 : 0;  // a byte that started in the previous MCU is that MCU's
  const int full = end >> 3;
  uint8_t* out = raw + im.mcu0 * DM4D_JPEG_MCU_UNSTUFFED + (start >> 3);
  for (int j = first + lane; j < full; j += kWave) out[j] = (uint8_t)(buf[j >> 2] >> (24 - 8 * (j & 3)));
  if ((end & 7) && lane == 0) {  // the byte this MCU leaves unfinished: the next MCU's first bits, or 1-bits at the end of the image
    const uint32_t tail = m + 1 < im.mcus ? head[im.mcu0 + m + 1] : 0xffu;
    out[full] = (uint8_t)((buf[full >> 2] >> (24 - 8 * (full & 3))) | (tail >> (end & 7)));
  }
}

// -- stuffing ----------------------------------------------------------------------------------------------------------------------------
// the 16 bytes of lane t of chunk c (zeros beyond the scan), and how many of them are 0xFF
__device__ __forceinline__ int load16(const uint8_t* __restrict__ raw, int64_t off, int64_t nbytes, uint8_t (&v)[16]) {
  U4 q{0u, 0u, 0u, 0u};
  if (off < nbytes) q = *reinterpret_cast<const U4*>(raw + off);  // 16-aligned, inside the image's reservation
  const uint32_t w[4] = {q.x, q.y, q.z, q.w};
  int n = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    v[i] = off + i < nbytes ? (uint8_t)(w[i >> 2] >> (8 * (i & 3))) : (uint8_t)0;
    n += v[i] == 0xff;
  }
  return n;
}

__global__ void __launch_bounds__(kStuffThreads) jpeg_count_kernel(const int64_t* __restrict__ desc, const uint8_t* __restrict__ raw,
                                                                   const int64_t* __restrict__ nbytes, uint32_t* __restrict__ counts) {
  __shared__ int wave_n[kStuffThreads / 64];
  const Image im = image_of(desc, blockIdx.y, nullptr, nullptr);
  const int64_t nb = nbytes[blockIdx.y];
  const int64_t off = (int64_t)blockIdx.x * DM4D_JPEG_CHUNK + threadIdx.x * 16;
  if ((int64_t)blockIdx.x * DM4D_JPEG_CHUNK >= nb) return;
  uint8_t v[16];
  int n = load16(raw + im.mcu0 * DM4D_JPEG_MCU_UNSTUFFED, off, nb, v);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
  if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int w = 0; w < kStuffThreads / 64; ++w) t += wave_n[w];
    counts[im.chunk0 + blockIdx.x] = (uint32_t)t;
  }
}

// 0xFF counts of an image's chunks -> 0xFF bytes before each chunk; lens[i] = bytes of its stuffed scan
__global__ void __launch_bounds__(kScanThreads) jpeg_scan_ff_kernel(const int64_t* __restrict__ desc, uint32_t* __restrict__ counts,
                                                                    const int64_t* __restrict__ nbytes, int64_t* __restrict__ lens) {
  const Image im = image_of(desc, blockIdx.x, nullptr, nullptr);
  const int64_t nb = nbytes[blockIdx.x];
  const uint32_t total = block_excl_scan_inplace<uint32_t, kScanThreads>(counts + im.chunk0, (nb + DM4D_JPEG_CHUNK - 1) / DM4D_JPEG_CHUNK);
  if (threadIdx.x == 0) lens[blockIdx.x] = nb + (int64_t)total;
}

// ONE block: offs[i] = sum of lens[0 .. i)
__global__ void __launch_bounds__(kScanThreads) jpeg_offsets_kernel(const int64_t* __restrict__ lens, int64_t* __restrict__ offs, int n) {
  offsets_block<kScanThreads>(lens, offs, n);
}

__global__ void __launch_bounds__(kStuffThreads) jpeg_stuff_kernel(const int64_t* __restrict__ desc, const uint8_t* __restrict__ raw,
                                                                   const int64_t* __restrict__ nbytes, const uint32_t* __restrict__ before,
                                                                   const int64_t* __restrict__ offs, uint8_t* __restrict__ blob) {
  __shared__ int wave_n[kStuffThreads / 64];
  const Image im = image_of(desc, blockIdx.y, nullptr, nullptr);
  const int64_t nb = nbytes[blockIdx.y];
  const int64_t off = (int64_t)blockIdx.x * DM4D_JPEG_CHUNK + threadIdx.x * 16;
  if ((int64_t)blockIdx.x * DM4D_JPEG_CHUNK >= nb) return;
  uint8_t v[16];
  const int n = load16(raw + im.mcu0 * DM4D_JPEG_MCU_UNSTUFFED, off, nb, v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int s = wave_incl_scan(n);
  if (lane == 63) wave_n[wave] = s;
  __syncthreads();
  int64_t at = offs[blockIdx.y] + off + (int64_t)before[im.chunk0 + blockIdx.x] + (s - n);
  for (int w = 0; w < wave; ++w) at += wave_n[w];
  uint8_t* out = blob + at;
#pragma unroll
  for (int i = 0; i < 16; ++i)
    if (off + i < nb) {
      *out++ = v[i];
      if (v[i] == 0xff) *out++ = 0;
    }
}

// -- crop restore ------------------------------------------------------------------------------------------------------------------------
// Horizontal pass: one lane = one pixel of scratch [H][cw][3]
__global__ void __launch_bounds__(kWave) restore_hpass_kernel(const uint8_t* __restrict__ pixels, const int64_t* __restrict__ desc,
                                                              const int32_t* __restrict__ tab, uint8_t* __restrict__ scratch) {
  const int64_t* d = desc + (int64_t)blockIdx.z * DM4D_RESTORE_FIELDS;
  const int H = (int)d[R_H], W = (int)d[R_W], cw = (int)d[R_CW];
  const int r = blockIdx.y, ox = blockIdx.x * kWave + threadIdx.x;
  if (r >= H || ox >= cw) return;
  const int ksize = (int)d[R_HK];
  const int32_t* bounds = tab + d[R_HTAB];
  const int32_t* k = bounds + 2 * cw + (int64_t)ox * ksize;
  const int xmin = bounds[2 * ox], cnt = bounds[2 * ox + 1];
  uint32_t o[3];
  pillow_rgb(ByteRgb{pixels + d[R_SRC] + ((int64_t)r * W + xmin) * 3, 3}, k, cnt, o);
  uint8_t* dst = scratch + d[R_SCRATCH] + ((int64_t)r * cw + ox) * 3;
  dst[0] = (uint8_t)o[0], dst[1] = (uint8_t)o[1], dst[2] = (uint8_t)o[2];
}

// Vertical pass + paste: one lane = one canvas pixel; white where the patch does not cover it
__global__ void __launch_bounds__(kWave) restore_vpass_kernel(const int64_t* __restrict__ desc, const int32_t* __restrict__ tab,
                                                              const uint8_t* __restrict__ scratch, uint8_t* __restrict__ canvases) {
  const int64_t* d = desc + (int64_t)blockIdx.z * DM4D_RESTORE_FIELDS;
  const int h = (int)d[R_CANVAS_H], w = (int)d[R_CANVAS_W];
  const int y = blockIdx.y, x = blockIdx.x * kWave + threadIdx.x;
  if (y >= h || x >= w) return;
  const int ch = (int)d[R_CH], cw = (int)d[R_CW];
  const int py = y - (int)d[R_CT], px = x - (int)d[R_CL];
  uint32_t o[3] = {255u, 255u, 255u};
  if (py >= 0 && py < ch && px >= 0 && px < cw) {
    const int ksize = (int)d[R_VK];
    const int32_t* bounds = tab + d[R_VTAB];
    const int32_t* k = bounds + 2 * ch + (int64_t)py * ksize;
    const int ymin = bounds[2 * py], cnt = bounds[2 * py + 1];
    pillow_rgb(ByteRgb{scratch + d[R_SCRATCH] + ((int64_t)ymin * cw + px) * 3, (int64_t)cw * 3}, k, cnt, o);
  }
  uint8_t* dst = canvases + d[R_DST] + ((int64_t)y * w + x) * 3;
  dst[0] = (uint8_t)o[0], dst[1] = (uint8_t)o[1], dst[2] = (uint8_t)o[2];
}

bool size_ok(int64_t v) { return v >= 1 && v <= 65535; }
int64_t mcus_of(int64_t h, int64_t w) { return ((h + 15) / 16) * ((w + 15) / 16); }
int64_t chunks_of(int64_t mcus) { return (mcus * DM4D_JPEG_MCU_UNSTUFFED + DM4D_JPEG_CHUNK - 1) / DM4D_JPEG_CHUNK; }
constexpr int64_t kMaxMcus = (1ll << 32) / kMcuBits;  // an image's bit positions are 32-bit
constexpr int64_t kMaxTotalMcus = 1ll << 28;

// workspace: coefficients | bit lengths -> positions | head bits | unstuffed scans | 0xFF counts | bytes per image
struct Layout {
  int64_t coef, bits, head, raw, counts, nbytes, total;
};
Layout layout_of(int64_t total_mcus, int64_t n) {
  Layout l;
  l.coef = 0;
  l.bits = l.coef + total_mcus * 768;
  l.head = l.bits + pad16(total_mcus * 4);
  l.raw = l.head + pad16(total_mcus * 4);
  l.counts = l.raw + total_mcus * DM4D_JPEG_MCU_UNSTUFFED;
  l.nbytes = l.counts + pad16((chunks_of(total_mcus) + n) * 4);
  l.total = l.nbytes + pad16(n * 8);
  return l;
}

}  // namespace

extern "C" int dm4d_restore_crop_u8(void* stream, const void* pixels, int64_t pixels_bytes, const int64_t* desc_host, const int64_t* desc_dev,
                                    int n, const int32_t* tab_host, const int32_t* tab_dev, int64_t tab_len, void* scratch,
                                    int64_t scratch_bytes, void* canvases, int64_t canvases_bytes) {
  if (!pixels || !desc_host || !desc_dev || !tab_host || !tab_dev || !scratch || !canvases)
    return dm4d_set_error(DM4D_ERR_ARG, "restore_crop: null pointer");
  if (n <= 0 || n > 65535 || pixels_bytes <= 0 || tab_len <= 0 || scratch_bytes <= 0 || canvases_bytes <= 0)
    return dm4d_set_error(DM4D_ERR_ARG, "restore_crop: empty or oversized batch");
  int64_t max_h = 0, max_cw = 0, max_ch_canvas = 0, max_w = 0, canvas_end = 0;
  for (int i = 0; i < n; ++i) {
    const int64_t* d = desc_host + (int64_t)i * DM4D_RESTORE_FIELDS;
    const int64_t H = d[R_H], W = d[R_W], ch = d[R_CH], cw = d[R_CW], h = d[R_CANVAS_H], w = d[R_CANVAS_W];
    if (!size_ok(H) || !size_ok(W) || !size_ok(ch) || !size_ok(cw) || !size_ok(h) || !size_ok(w))
      return dm4d_set_error(DM4D_ERR_ARG, "restore_crop: a dimension outside 1..65535 in a descriptor");
    if (d[R_CT] < -(1 << 20) || d[R_CT] > (1 << 20) || d[R_CL] < -(1 << 20) || d[R_CL] > (1 << 20))
      return dm4d_set_error(DM4D_ERR_ARG, "restore_crop: crop offset out of range in a descriptor");
    if (d[R_SRC] < 0 || d[R_SRC] > pixels_bytes || H * W * 3 > pixels_bytes - d[R_SRC])
      return dm4d_set_error(DM4D_ERR_ARG, "restore_crop: a source image lies outside the pixel buffer");
    if (!pillow_table_ok(tab_host, tab_len, d[R_HTAB], d[R_HK], 1 << 18, cw, W, false) ||
        !pillow_table_ok(tab_host, tab_len, d[R_VTAB], d[R_VK], 1 << 18, ch, H, false))
      return dm4d_set_error(DM4D_ERR_ARG, "restore_crop: a coefficient table is out of range or its windows leave the image");
    if (d[R_SCRATCH] < 0 || d[R_SCRATCH] > scratch_bytes || H * cw * 3 > scratch_bytes - d[R_SCRATCH])
      return dm4d_set_error(DM4D_ERR_ARG, "restore_crop: a scratch region lies outside the scratch buffer");
    if (d[R_DST] < canvas_end || d[R_DST] > canvases_bytes || h * w * 3 > canvases_bytes - d[R_DST])
      return dm4d_set_error(DM4D_ERR_ARG, "restore_crop: a canvas lies outside the canvas buffer or overlaps the one before it");
    canvas_end = d[R_DST] + h * w * 3;
    if (H > max_h) max_h = H;
    if (cw > max_cw) max_cw = cw;
    if (h > max_ch_canvas) max_ch_canvas = h;
    if (w > max_w) max_w = w;
  }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(restore_hpass_kernel, dim3((unsigned)((max_cw + kWave - 1) / kWave), (unsigned)max_h, (unsigned)n), dim3(kWave), 0, st,
                     (const uint8_t*)pixels, desc_dev, tab_dev, (uint8_t*)scratch);
  int rc = dm4d_check_launch("restore_hpass_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(restore_vpass_kernel, dim3((unsigned)((max_w + kWave - 1) / kWave), (unsigned)max_ch_canvas, (unsigned)n), dim3(kWave), 0,
                     st, desc_dev, tab_dev, (const uint8_t*)scratch, (uint8_t*)canvases);
  return dm4d_check_launch("restore_vpass_kernel");
}

extern "C" size_t dm4d_jpeg_scan_bound(int h, int w) {
  if (!size_ok(h) || !size_ok(w) || mcus_of(h, w) > kMaxMcus) return 0;
  return (size_t)(mcus_of(h, w) * DM4D_JPEG_MCU_BOUND);
}

extern "C" size_t dm4d_jpeg_ws_bytes(int64_t total_mcus, int n) {
  if (total_mcus <= 0 || total_mcus > kMaxTotalMcus || n <= 0 || n > 65535) return 0;
  return (size_t)layout_of(total_mcus, n).total;
}

extern "C" int dm4d_jpeg_encode_rgb_u8(void* stream, const void* pixels, int64_t pixels_bytes, const void* canvases, int64_t canvases_bytes,
                                       const int64_t* desc_host, const int64_t* desc_dev, int n, const uint16_t* qtab_host,
                                       const uint16_t* qtab_dev, void* workspace, int64_t workspace_bytes, void* blob, int64_t blob_bytes,
                                       int64_t* out) {
  if (!desc_host || !desc_dev || !qtab_host || !qtab_dev || !workspace || !blob || !out)
    return dm4d_set_error(DM4D_ERR_ARG, "jpeg_encode: null pointer");
  if (n <= 0 || n > 65535) return dm4d_set_error(DM4D_ERR_ARG, "jpeg_encode: empty or oversized batch");
  if (((uintptr_t)workspace & 15) || ((uintptr_t)out & 7)) return dm4d_set_error(DM4D_ERR_ARG, "jpeg_encode: workspace must be 16-byte aligned, out 8-byte");
  for (int i = 0; i < 128; ++i)
    if (qtab_host[i] < 1 || qtab_host[i] > 255) return dm4d_set_error(DM4D_ERR_ARG, "jpeg_encode: a quantisation value outside 1..255");
  int64_t mcu0 = 0, chunk0 = 0, bound = 0, max_mcus = 0, max_chunks = 0;
  for (int i = 0; i < n; ++i) {
    const int64_t* d = desc_host + (int64_t)i * DM4D_JPEG_FIELDS;
    const int64_t h = d[J_H], w = d[J_W];
    if (!size_ok(h) || !size_ok(w)) return dm4d_set_error(DM4D_ERR_ARG, "jpeg_encode: a dimension outside 1..65535 in a descriptor");
    const int64_t mcus = mcus_of(h, w);
    if (mcus > kMaxMcus) return dm4d_set_error(DM4D_ERR_ARG, "jpeg_encode: an image has too many MCUs for 32-bit bit positions");
    const bool canvas = d[J_SPACE] == 1;
    if (d[J_SPACE] != 0 && !canvas) return dm4d_set_error(DM4D_ERR_ARG, "jpeg_encode: a descriptor names neither pixels nor canvases");
    const int64_t space = canvas ? canvases_bytes : pixels_bytes;
    if (!(canvas ? canvases : pixels) || space <= 0 || d[J_PIX] < 0 || d[J_PIX] > space || h * w * 3 > space - d[J_PIX])
      return dm4d_set_error(DM4D_ERR_ARG, "jpeg_encode: an image lies outside its buffer");
    if (d[J_MCU0] != mcu0 || d[J_CHUNK0] != chunk0 || d[6] != 0 || d[7] != 0)
      return dm4d_set_error(DM4D_ERR_ARG, "jpeg_encode: a descriptor's first MCU or first chunk is not the running sum");
    mcu0 += mcus, chunk0 += chunks_of(mcus), bound += mcus * DM4D_JPEG_MCU_BOUND;
    if (mcu0 > kMaxTotalMcus) return dm4d_set_error(DM4D_ERR_ARG, "jpeg_encode: too many MCUs in one batch");
    if (mcus > max_mcus) max_mcus = mcus;
    if (chunks_of(mcus) > max_chunks) max_chunks = chunks_of(mcus);
  }
  const Layout l = layout_of(mcu0, n);
  if (workspace_bytes < l.total) return dm4d_set_error(DM4D_ERR_ARG, "jpeg_encode: workspace too small (dm4d_jpeg_ws_bytes)");
  if (blob_bytes < bound) return dm4d_set_error(DM4D_ERR_ARG, "jpeg_encode: blob capacity below the sum of dm4d_jpeg_scan_bound");
  char* ws = (char*)workspace;
  int16_t* coef = (int16_t*)(ws + l.coef);
  uint32_t* bits = (uint32_t*)(ws + l.bits);
  uint32_t* head = (uint32_t*)(ws + l.head);
  uint8_t* raw = (uint8_t*)(ws + l.raw);
  uint32_t* counts = (uint32_t*)(ws + l.counts);
  int64_t* nbytes = (int64_t*)(ws + l.nbytes);
  int64_t* offs = out;
  int64_t* lens = out + n;
  hipStream_t st = (hipStream_t)stream;
  const dim3 per_mcu((unsigned)max_mcus, (unsigned)n), per_chunk((unsigned)max_chunks, (unsigned)n);
  int rc;
  hipLaunchKernelGGL(jpeg_coef_kernel, per_mcu, dim3(kWave), 0, st, desc_dev, (const uint8_t*)pixels, (const uint8_t*)canvases, qtab_dev, coef);
  if ((rc = dm4d_check_launch("jpeg_coef_kernel"))) return rc;
  hipLaunchKernelGGL(jpeg_size_kernel, per_mcu, dim3(kWave), 0, st, desc_dev, (const int16_t*)coef, bits, head);
  if ((rc = dm4d_check_launch("jpeg_size_kernel"))) return rc;
  hipLaunchKernelGGL(jpeg_scan_bits_kernel, dim3((unsigned)n), dim3(kScanThreads), 0, st, desc_dev, bits, nbytes);
  if ((rc = dm4d_check_launch("jpeg_scan_bits_kernel"))) return rc;
  hipLaunchKernelGGL(jpeg_emit_kernel, per_mcu, dim3(kWave), 0, st, desc_dev, (const int16_t*)coef, (const uint32_t*)bits,
                     (const uint32_t*)head, raw);
  if ((rc = dm4d_check_launch("jpeg_emit_kernel"))) return rc;
  hipLaunchKernelGGL(jpeg_count_kernel, per_chunk, dim3(kStuffThreads), 0, st, desc_dev, (const uint8_t*)raw, (const int64_t*)nbytes, counts);
  if ((rc = dm4d_check_launch("jpeg_count_kernel"))) return rc;
  hipLaunchKernelGGL(jpeg_scan_ff_kernel, dim3((unsigned)n), dim3(kScanThreads), 0, st, desc_dev, counts, (const int64_t*)nbytes, lens);
  if ((rc = dm4d_check_launch("jpeg_scan_ff_kernel"))) return rc;
  hipLaunchKernelGGL(jpeg_offsets_kernel, dim3(1), dim3(kScanThreads), 0, st, (const int64_t*)lens, offs, n);
  if ((rc = dm4d_check_launch("jpeg_offsets_kernel"))) return rc;
  hipLaunchKernelGGL(jpeg_stuff_kernel, per_chunk, dim3(kStuffThreads), 0, st, desc_dev, (const uint8_t*)raw, (const int64_t*)nbytes,
                     (const uint32_t*)counts, (const int64_t*)offs, (uint8_t*)blob);
  return dm4d_check_launch("jpeg_stuff_kernel");
}
