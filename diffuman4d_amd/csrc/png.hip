// PNG files on the device: a batch of 8-bit L or RGBA images of different sizes -> complete files (signature, IHDR, IDAT chunks, IEND)
// in one blob, every byte of them -- chunk CRC-32s, zlib header, Adler-32 -- made here.  The definition is tests/png_model.py (DESIGN.md
// "Device PNG"): Paeth filter on every row; the filtered stream cut into stripes of whole rows; within a stripe maximal runs of equal
// bytes become a literal plus distance-1 matches; one dynamic-Huffman block per stripe whose canonical code is built here from the
// stripe's histogram; an empty stored block after it, so that every stripe is whole bytes and is its own IDAT chunk.
//
// Five launches on one stream for the whole batch; launch boundaries are the only ordering between workgroups.  The run finder of
// `stripe`, the bit window of `emit` and the body of `offsets` are stripe_emit.h's, shared with webp.hip; the code lengths are
// prefix_code.h's:
//   filter   one lane per pixel: the filtered scanlines to the workspace (an RGBA pixel is read from the packed RGB image and the alpha
//            plane; no RGBA buffer exists)
//   stripe   one workgroup per stripe: run boundaries per lane segment, the token of every byte position to the workspace (uint16:
//            literal, 256 + match length, or none), histogram (integer LDS atomics), Adler sums, code lengths (rank sort by all lanes,
//            the two-queue tree by lane 0), canonical codes, the block header, the chunk's size
//   scan     one workgroup per image: chunk sizes -> chunk offsets, the file's length, the Adler-32
//   offsets  one workgroup: the files' places in the blob
//   emit     one workgroup per stripe: tokens -> bits, OR-ed into an LDS window of 4096 positions at positions from a prefix sum, whole
//            bytes stored, the unfinished byte carried; chunk framing; the chunk's CRC-32 from 256 segment CRCs combined in GF(2)
// Integer arithmetic only; the atomics are LDS-local integer adds and ORs, whose result does not depend on their order.
#include <stdint.h>

#include "common.h"
#include "dm4d.h"
#include "errors.h"
#include "image_common.h"
#include "prefix_code.h"
#include "stripe_emit.h"

namespace {

constexpr int kThreads = 256;
constexpr int kScanThreads = 1024;
constexpr int kSyms = 286;                 // literal / length symbols
constexpr int kSeq = 288;                  // + the two distance codes
constexpr int kPer = 16;                   // byte positions per lane and round of the emitter
constexpr int kWinWords = 2704;            // 7 + 4096 x 21 bits and slack
constexpr int kHdrWords = 136;             // 17 + 57 + 288 x 14 bits at most
constexpr int kRecWords = DM4D_PNG_STRIPE_REC / 4;
constexpr int kRecHdr = kSeq;              // words of a stripe record: codes [288] | header [136] | header bits, Adler s1, s2, 0
constexpr int kRecMeta = kSeq + kHdrWords;
constexpr uint32_t kAdler = 65521u;
constexpr uint32_t kPoly = 0xedb88320u;
constexpr uint16_t kNone = 0xffffu;
static_assert(kRecMeta + 4 == kRecWords, "stripe record layout");
static_assert(kThreads == kPrefixThreads && kSeq <= kPrefixMaxSyms, "prefix_code.h is written for this workgroup and alphabet");

enum { P_KIND = 0, P_H, P_W, P_PIX, P_PIX_STRIDE, P_ALPHA, P_ALPHA_STRIDE, P_FILT0, P_STRIPE0 };

// RFC 1951 3.2.5: length 3..258 -> index of its code (symbol 257 + index), the code's base length and extra bits
struct LenTab {
  uint8_t idx[259];
  uint16_t base[29];
  uint8_t extra[29];
};
constexpr LenTab make_len_tab() {
  LenTab t{};
  int len = 3;
  for (int k = 0; k < 28; ++k) {
    const int eb = k < 8 ? 0 : (k - 4) / 4;
    t.base[k] = (uint16_t)len, t.extra[k] = (uint8_t)eb;
    for (int i = 0; i < (1 << eb); ++i) t.idx[len++] = (uint8_t)k;
  }
  t.base[28] = 258, t.extra[28] = 0, t.idx[258] = 28;  // 258 has a code of its own (227 + 31 is not used)
  return t;
}
__device__ const LenTab kLen = make_len_tab();
__device__ const uint8_t kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

struct Image {
  int kind, h, w, bpp, rows, stripes;
  int64_t R, pix, pstride, alpha, astride, filt0, stripe0;
};

__host__ __device__ inline int rows_of(int64_t R) { return R >= DM4D_PNG_STRIPE_BYTES ? 1 : (int)(DM4D_PNG_STRIPE_BYTES / R); }

__device__ __forceinline__ Image image_of(const int64_t* __restrict__ desc, int i) {
  const int64_t* d = desc + (int64_t)i * DM4D_PNG_FIELDS;
  Image im;
  im.kind = (int)d[P_KIND], im.h = (int)d[P_H], im.w = (int)d[P_W];
  im.bpp = im.kind ? 4 : 1;
  im.R = 1 + (int64_t)im.w * im.bpp;
  im.rows = rows_of(im.R);
  im.stripes = (im.h + im.rows - 1) / im.rows;
  im.pix = d[P_PIX], im.pstride = d[P_PIX_STRIDE], im.alpha = d[P_ALPHA], im.astride = d[P_ALPHA_STRIDE];
  im.filt0 = d[P_FILT0], im.stripe0 = d[P_STRIPE0];
  return im;
}

// -- filter ------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// cur - Paeth(left, up, up-left) of the byte at p; `step` bytes to the left neighbour, `stride` to the row above; zeros outside
__device__ __forceinline__ uint8_t filtered(const uint8_t* p, int step, int64_t stride, bool left, bool up) {
  const int a = left ? p[-step] : 0, b = up ? p[-stride] : 0, c = (left && up) ? p[-stride - step] : 0;
  return (uint8_t)(p[0] - paeth(a, b, c));
}

__global__ void __launch_bounds__(kThreads) png_filter_kernel(const int64_t* __restrict__ desc, const uint8_t* __restrict__ planes,
                                                              const uint8_t* __restrict__ rgb, uint8_t* __restrict__ filt) {
  const Image im = image_of(desc, blockIdx.z);
  const int y = blockIdx.y, x = blockIdx.x * kThreads + threadIdx.x;
  if (y >= im.h || x >= im.w) return;
  uint8_t* out = filt + im.filt0 + (int64_t)y * im.R;
  if (x == 0) out[0] = 4;
  out += 1 + (int64_t)x * im.bpp;
  const bool left = x > 0, up = y > 0;
  if (im.kind == 0) {
    out[0] = filtered(planes + im.pix + (int64_t)y * im.pstride + x, 1, im.pstride, left, up);
  } else {
    const uint8_t* p = rgb + im.pix + (int64_t)y * im.pstride + (int64_t)x * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = filtered(p + c, 3, im.pstride, left, up);
    out[3] = filtered(planes + im.alpha + (int64_t)y * im.astride + x, 1, im.astride, left, up);
  }
}

// -- the stripe: tokens, histogram, code, header, size --------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) png_stripe_kernel(const int64_t* __restrict__ desc, const uint8_t* __restrict__ filt,
                                                              uint16_t* __restrict__ tok, uint32_t* __restrict__ recs,
                                                              uint32_t* __restrict__ clen) {
  __shared__ uint32_t hist[kSeq], work[kSeq], codes[kSeq], clfreq[20], clcodes[20], hdr[kHdrWords];
  __shared__ uint8_t lens[kSeq], cllens[20], clsym[kSeq], clval[kSeq];
  __shared__ HuffScratch sc;
  __shared__ int sh_first[kThreads], sh_last[kThreads];
  __shared__ uint32_t xbits, a1, a2;
  __shared__ int ncl;
  const Image im = image_of(desc, blockIdx.y);
  const int s = blockIdx.x;
  if (s >= im.stripes) return;
  const int tid = threadIdx.x;
  const int row0 = s * im.rows, nrows = min(im.rows, im.h - row0);
  const int S = (int)(nrows * im.R);  // at most max(R, DM4D_PNG_STRIPE_BYTES) <= 65537
  const uint8_t* f = filt + im.filt0 + (int64_t)row0 * im.R;
  uint16_t* tk = tok + im.filt0 + (int64_t)row0 * im.R;
  for (int i = tid; i < kSeq; i += kThreads) hist[i] = 0;
  for (int i = tid; i < kHdrWords; i += kThreads) hdr[i] = 0;
  if (tid < 20) clfreq[tid] = 0;
  if (tid == 0) xbits = 0, a1 = 0, a2 = 0;
  // pass 1: the runs that reach over this lane's segment [a, b) (stripe_emit.h), and the Adler sums
  uint64_t s1 = 0, s2 = 0;
  const LaneRuns lr = lane_runs<kThreads>(
      S, sh_first, sh_last, [&](int i) { return (int)f[i]; }, [](int prev, int v) { return v != prev; },
      [&](int i, int v) { s1 += (uint32_t)v, s2 += (uint64_t)(uint32_t)(S - i) * (uint32_t)v; });
  const int a = lr.a, b = lr.b, s_in = lr.s_in, e_out = lr.e_out;
  if (a < b) atomicAdd(&a1, (uint32_t)(s1 % kAdler)), atomicAdd(&a2, (uint32_t)(s2 % kAdler));
  // pass 2: run by run; every position gets its token
  for (int i = a; i < b;) {
    const int v = f[i];
    const int rs = (i == 0 || f[i - 1] != v) ? i : s_in;  // only the segment's first position can lie inside a run
    int k = i + 1;
    while (k < b && f[k] == v) ++k;
    const int re = k < b ? k : e_out;
    const int m = re - rs - 1, full = m / 258, r = m - full * 258;
    for (int p = i; p < k; ++p) {
      const int j = p - rs;
      uint16_t t = (uint16_t)v;
      if (j > 0) {
        const int q = j - 1, blk = q / 258, pos = q - blk * 258;
        const int len = blk < full ? 258 : r;
        if (len >= 3) t = pos == 0 ? (uint16_t)(256 + len) : kNone;
      }
      tk[p] = t;
      if (t < 256) {
        atomicAdd(&hist[t], 1u);
      } else if (t != kNone) {
        const int li = kLen.idx[t - 256];
        atomicAdd(&hist[257 + li], 1u);
        atomicAdd(&xbits, (uint32_t)kLen.extra[li] + 1u);  // + the distance code's one bit
      }
    }
    i = k;
  }
  __syncthreads();
  if (tid == 0) hist[256] = 1;
  __syncthreads();
  for (int i = tid; i < kSeq; i += kThreads) work[i] = hist[i];
  __syncthreads();
  build_lengths(work, kSyms, 15, lens, sc);
  __syncthreads();
  if (tid == 0) {  // the 288 lengths as code-length symbols
    lens[286] = 1, lens[287] = 1;
    int n = 0;
    for (int i = 0; i < kSeq;) {
      const int v = lens[i];
      int sym = v, val = 0, step = 1;
      if (v == 0) {
        int z = 1;
        while (i + z < kSeq && lens[i + z] == 0) ++z;
        if (z >= 11) {
          z = min(z, 138), sym = 18, val = z - 11, step = z;
        } else if (z >= 3) {
          sym = 17, val = z - 3, step = z;
        }
      }
      clsym[n] = (uint8_t)sym, clval[n] = (uint8_t)val, ++n;
      ++clfreq[sym];
      i += step;
    }
    ncl = n;
  }
  __syncthreads();
  build_lengths(clfreq, 19, 7, cllens, sc);
  __syncthreads();
  if (tid == 0) {
    canonical_codes(lens, kSyms, codes);
    codes[286] = codes[287] = 0;
    canonical_codes(cllens, 19, clcodes);
    BitOut o{hdr, 0};
    o.put(0, 1), o.put(2, 2), o.put(29, 5), o.put(1, 5), o.put(15, 4);
    for (int i = 0; i < 19; ++i) o.put(cllens[kClOrder[i]], 3);
    for (int i = 0; i < ncl; ++i) {
      const int sym = clsym[i], l = cllens[sym];
      const int eb = sym == 18 ? 7 : (sym == 17 ? 3 : 0);
      o.put((clcodes[sym] & 0xffffu) | ((uint32_t)clval[i] << l), l + eb);
    }
    uint32_t bits = (uint32_t)o.pos + xbits + 3u;  // + the stored block's header bits
    for (int i = 0; i < kSyms; ++i) bits += hist[i] * lens[i];
    const bool first_stripe = s == 0, last_stripe = s == im.stripes - 1;
    clen[im.stripe0 + s] = 12u + (first_stripe ? 2u : 0u) + ((bits + 7u) >> 3) + 4u + (last_stripe ? 4u : 0u);
    sc.n = o.pos;
  }
  __syncthreads();
  uint32_t* rec = recs + (im.stripe0 + s) * kRecWords;
  for (int i = tid; i < kSeq; i += kThreads) rec[i] = codes[i];
  for (int i = tid; i < kHdrWords; i += kThreads) rec[kRecHdr + i] = hdr[i];
  if (tid == 0) rec[kRecMeta] = (uint32_t)sc.n, rec[kRecMeta + 1] = a1 % kAdler, rec[kRecMeta + 2] = a2 % kAdler, rec[kRecMeta + 3] = 0;
}

// -- per image: chunk offsets, file length, Adler-32 -----------------------------------------------------------------------------------
__global__ void __launch_bounds__(kScanThreads) png_scan_kernel(const int64_t* __restrict__ desc, const uint32_t* __restrict__ recs,
                                                                uint32_t* __restrict__ clen, uint32_t* __restrict__ adler,
                                                                int64_t* __restrict__ lens) {
  __shared__ uint32_t sa, sb;
  const Image im = image_of(desc, blockIdx.x);
  if (threadIdx.x == 0) sa = 0, sb = 0;
  __syncthreads();
  const int64_t N = im.h * im.R;
  for (int s = threadIdx.x; s < im.stripes; s += kScanThreads) {
    const uint32_t* rec = recs + (im.stripe0 + s) * kRecWords + kRecMeta;
    const int64_t end = (int64_t)min(im.h, (s + 1) * im.rows) * im.R;
    const uint64_t after = (uint64_t)(N - end) % kAdler;
    atomicAdd(&sa, rec[1]);
    atomicAdd(&sb, (uint32_t)((rec[2] + after * rec[1]) % kAdler));
  }
  __syncthreads();
  const uint32_t total = block_excl_scan_inplace<uint32_t, kScanThreads>(clen + im.stripe0, im.stripes);
  if (threadIdx.x == 0) {
    lens[blockIdx.x] = 45 + (int64_t)total;
    adler[blockIdx.x] = (uint32_t)(((uint64_t)N + sb) % kAdler) << 16 | ((1u + sa) % kAdler);
  }
}

// ONE block: offs[i] = sum of lens[0 .. i)
__global__ void __launch_bounds__(kScanThreads) png_offsets_kernel(const int64_t* __restrict__ lens, int64_t* __restrict__ offs, int n) {
  offsets_block<kScanThreads>(lens, offs, n);
}

// -- emit ----------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void put_be32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)(v >> 24), p[1] = (uint8_t)(v >> 16), p[2] = (uint8_t)(v >> 8), p[3] = (uint8_t)v;
}

__device__ __forceinline__ uint32_t crc_byte(uint32_t c, uint32_t byte) {
  c ^= byte;
#pragma unroll
  for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (kPoly & (0u - (c & 1u)));
  return c;
}

// a(x) b(x) mod the CRC-32 polynomial, reflected: bit 31 is x^0
__device__ __forceinline__ uint32_t gf2_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (uint32_t m = 1u << 31; m; m >>= 1) {
    if (a & m) p ^= b;
    b = (b >> 1) ^ (kPoly & (0u - (b & 1u)));
  }
  return p;
}

__global__ void __launch_bounds__(kThreads) png_emit_kernel(const int64_t* __restrict__ desc, const uint16_t* __restrict__ tok,
                                                            const uint32_t* __restrict__ recs, const uint32_t* __restrict__ clen,
                                                            const uint32_t* __restrict__ adler, const int64_t* __restrict__ offs,
                                                            const int64_t* __restrict__ lens, uint8_t* __restrict__ blob) {
  __shared__ uint32_t tab[kSeq], win[kWinWords], wave_tot[kThreads / 64], crcs[kThreads];
  __shared__ uint32_t datalen_s;
  const Image im = image_of(desc, blockIdx.y);
  const int s = blockIdx.x;
  if (s >= im.stripes) return;
  const int tid = threadIdx.x;
  const bool first_stripe = s == 0, last_stripe = s == im.stripes - 1;
  const int row0 = s * im.rows, nrows = min(im.rows, im.h - row0);
  const int S = (int)(nrows * im.R);
  const uint16_t* tk = tok + im.filt0 + (int64_t)row0 * im.R;
  const uint32_t* rec = recs + (im.stripe0 + s) * kRecWords;
  const uint32_t* cl = clen + im.stripe0;
  uint8_t* file = blob + offs[blockIdx.y];
  const uint32_t chunk_at = cl[s];
  const uint32_t chunk_len = (last_stripe ? (uint32_t)(lens[blockIdx.y] - 45) : cl[s + 1]) - chunk_at;
  uint8_t* ck = file + 33 + chunk_at;
  uint8_t* d = ck + 8 + (first_stripe ? 2 : 0);
  const uint32_t cap = chunk_len - 12u - (first_stripe ? 2u : 0u) - (last_stripe ? 4u : 0u);  // bytes of deflate data the sizing pass counted
  for (int i = tid; i < kSeq; i += kThreads) tab[i] = rec[i];
  const uint32_t hdr_bits = rec[kRecMeta];
  const uint8_t* hdr = reinterpret_cast<const uint8_t*>(rec + kRecHdr);
  uint64_t done = hdr_bits >> 3;
  int carry_bits = (int)(hdr_bits & 7u);
  for (uint32_t i = tid; i < done; i += kThreads)
    if (i < cap) d[i] = hdr[i];
  for (int i = tid; i < kWinWords; i += kThreads) win[i] = (i == 0 && carry_bits) ? hdr[done] : 0u;
  __syncthreads();
  emit_window<kThreads, kPer, kWinWords, uint32_t>(
      S, win, wave_tot, carry_bits, done,
      [&](int p, uint32_t& v, int& nb) {
        const uint32_t t = p < S ? tk[p] : kNone;
        if (t < 256u) {
          const uint32_t e = tab[t];
          v = e & 0xffffu, nb = (int)(e >> 16);
        } else if (t != kNone) {
          const int len = (int)t - 256, li = kLen.idx[len];
          const uint32_t e = tab[257 + li];
          const int l = (int)(e >> 16);
          v = (e & 0xffffu) | ((uint32_t)(len - kLen.base[li]) << l);
          nb = l + kLen.extra[li] + 1;  // the distance code (0, one bit) is the top bit
        }
      },
      [&](uint64_t i, uint32_t byte) {
        if (i < cap) d[i] = (uint8_t)byte;
      });
  if (tid == 0) {
    // end of block, then the empty stored block that brings the stripe to a byte boundary
    uint64_t acc = win[0];
    int cb = carry_bits;
    const uint32_t e = tab[256];
    acc |= (uint64_t)(e & 0xffffu) << cb, cb += (int)(e >> 16);
    acc |= (uint64_t)(last_stripe ? 1u : 0u) << cb, cb += 3;
    for (int i = 0; i < (cb + 7) >> 3; ++i, ++done)
      if (done < cap) d[done] = (uint8_t)(acc >> (8 * i));
    const uint8_t stored[4] = {0, 0, 0xff, 0xff};
    for (int i = 0; i < 4; ++i, ++done)
      if (done < cap) d[done] = stored[i];
    uint32_t datalen = (uint32_t)done + (first_stripe ? 2u : 0u);
    if (last_stripe) put_be32(d + done, adler[blockIdx.y]), datalen += 4;
    put_be32(ck, datalen);
    ck[4] = 'I', ck[5] = 'D', ck[6] = 'A', ck[7] = 'T';
    if (first_stripe) {
      ck[8] = 0x78, ck[9] = 0x01;
      const uint8_t sig[16] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n', 0, 0, 0, 13, 'I', 'H', 'D', 'R'};
      for (int i = 0; i < 16; ++i) file[i] = sig[i];
      put_be32(file + 16, (uint32_t)im.w), put_be32(file + 20, (uint32_t)im.h);
      file[24] = 8, file[25] = im.kind ? 6 : 0, file[26] = 0, file[27] = 0, file[28] = 0;
      uint32_t c = 0xffffffffu;
      for (int i = 12; i < 29; ++i) c = crc_byte(c, file[i]);
      put_be32(file + 29, ~c);
    }
    if (last_stripe) {
      const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xae, 0x42, 0x60, 0x82};
      for (int i = 0; i < 12; ++i) ck[12 + datalen + i] = iend[i];
    }
    datalen_s = datalen;
  }
  __syncthreads();  // the chunk's bytes, written by this workgroup, are visible to all of it
  // CRC-32 of type + data: 256 equal segments of the message (zeros in front, which a zero register ignores; the initial value is the
  // complement of the first four bytes), then eight levels of crc(A | B) = crc(A) x^(8 |B|) + crc(B)
  const uint32_t datalen = datalen_s;
  const int64_t n = 4 + (int64_t)datalen;
  const int64_t seg = (n + kThreads - 1) / kThreads, pad = seg * kThreads - n;
  uint32_t c = 0;
  for (int64_t i = 0; i < seg; ++i) {
    const int64_t idx = tid * seg + i - pad;
    if (idx >= 0) c = crc_byte(c, idx < 4 ? (uint32_t)ck[4 + idx] ^ 0xffu : (uint32_t)ck[4 + idx]);
  }
  crcs[tid] = c;
  uint32_t m = 1u << 31, pw = 1u << 30;  // x^0, x^1 -> m = x^(8 seg)
  for (uint64_t e = (uint64_t)seg * 8; e; e >>= 1) {
    if (e & 1) m = gf2_mul(m, pw);
    pw = gf2_mul(pw, pw);
  }
  for (int k = 0; k < 8; ++k) {
    __syncthreads();
    if ((tid & ((2 << k) - 1)) == 0) crcs[tid] = gf2_mul(m, crcs[tid]) ^ crcs[tid + (1 << k)];
    m = gf2_mul(m, m);
  }
  if (tid == 0) put_be32(ck + 8 + datalen, ~crcs[0]);
}

// -- host ----------------------------------------------------------------------------------------------------------------------------------
bool side_ok(int64_t v) { return v >= 1 && v <= DM4D_MATTING_MAX_SIDE; }
int64_t stripes_of(int64_t h, int64_t R) {
  const int64_t rows = rows_of(R);
  return (h + rows - 1) / rows;
}
int64_t bound_of(int64_t h, int64_t w, int64_t bpp) {
  const int64_t R = 1 + w * bpp;
  return 64 + 576 * stripes_of(h, R) + 2 * h * R;
}
constexpr int64_t kMaxFiltered = 1ll << 40;
constexpr int64_t kMaxStripes = 1ll << 26;

// workspace: filtered scanlines | tokens | stripe records | chunk sizes -> offsets | Adler-32 per image
struct Layout {
  int64_t filt, tok, recs, clen, adler, total;
};
Layout layout_of(int64_t filtered, int64_t stripes, int64_t n) {
  Layout l;
  l.filt = 0;
  l.tok = l.filt + pad16(filtered);
  l.recs = l.tok + pad16(filtered * 2);
  l.clen = l.recs + stripes * DM4D_PNG_STRIPE_REC;
  l.adler = l.clen + pad16((stripes + 1) * 4);
  l.total = l.adler + pad16(n * 4);
  return l;
}

}  // namespace

extern "C" size_t dm4d_png_bound(int h, int w, int channels) {
  if (!side_ok(h) || !side_ok(w) || (channels != 1 && channels != 4)) return 0;
  return (size_t)bound_of(h, w, channels);
}

extern "C" size_t dm4d_png_ws_bytes(int64_t filtered_bytes, int64_t stripes, int n) {
  if (filtered_bytes < 2 || filtered_bytes > kMaxFiltered || stripes < 1 || stripes > kMaxStripes || n <= 0 || n > 65535 || stripes < n) return 0;
  return (size_t)layout_of(filtered_bytes, stripes, n).total;
}

extern "C" int dm4d_png_encode_u8(void* stream, const void* planes, int64_t planes_bytes, const void* rgb, int64_t rgb_bytes,
                                  const int64_t* desc_host, const int64_t* desc_dev, int n, void* workspace, int64_t workspace_bytes,
                                  void* blob, int64_t blob_bytes, int64_t* out) {
  if (!planes || !desc_host || !desc_dev || !workspace || !blob || !out) return dm4d_set_error(DM4D_ERR_ARG, "png_encode: null pointer");
  if (n <= 0 || n > 65535) return dm4d_set_error(DM4D_ERR_ARG, "png_encode: empty or oversized batch");
  if (((uintptr_t)workspace & 15) || ((uintptr_t)out & 7)) return dm4d_set_error(DM4D_ERR_ARG, "png_encode: workspace must be 16-byte aligned, out 8-byte");
  if (planes_bytes <= 0 || rgb_bytes < 0) return dm4d_set_error(DM4D_ERR_ARG, "png_encode: a buffer size is not positive");
  int64_t filt0 = 0, stripe0 = 0, bound = 0, max_h = 0, max_w = 0, max_stripes = 0;
  for (int i = 0; i < n; ++i) {
    const int64_t* d = desc_host + (int64_t)i * DM4D_PNG_FIELDS;
    const int64_t h = d[P_H], w = d[P_W];
    if (d[P_KIND] != DM4D_PNG_L && d[P_KIND] != DM4D_PNG_RGBA) return dm4d_set_error(DM4D_ERR_ARG, "png_encode: a descriptor's kind is neither L nor RGBA");
    if (!side_ok(h) || !side_ok(w)) return dm4d_set_error(DM4D_ERR_ARG, "png_encode: a dimension outside 1..DM4D_MATTING_MAX_SIDE in a descriptor");
    const bool rgba = d[P_KIND] == DM4D_PNG_RGBA;
    if (rgba) {
      if (!rgb || !plane_ok(d[P_PIX], d[P_PIX_STRIDE], h, 3 * w, rgb_bytes) || !plane_ok(d[P_ALPHA], d[P_ALPHA_STRIDE], h, w, planes_bytes))
        return dm4d_set_error(DM4D_ERR_ARG, "png_encode: an RGB image or its alpha plane lies outside its buffer");
    } else if (!plane_ok(d[P_PIX], d[P_PIX_STRIDE], h, w, planes_bytes) || d[P_ALPHA] != 0 || d[P_ALPHA_STRIDE] != 0) {
      return dm4d_set_error(DM4D_ERR_ARG, "png_encode: a plane lies outside its buffer");
    }
    if (d[P_FILT0] != filt0 || d[P_STRIPE0] != stripe0) return dm4d_set_error(DM4D_ERR_ARG, "png_encode: a descriptor's first byte or first stripe is not the running sum");
    for (int k = P_STRIPE0 + 1; k < DM4D_PNG_FIELDS; ++k)
      if (d[k] != 0) return dm4d_set_error(DM4D_ERR_ARG, "png_encode: a descriptor's spare field is not zero");
    const int64_t R = 1 + w * (rgba ? 4 : 1), stripes = stripes_of(h, R);
    filt0 += h * R, stripe0 += stripes, bound += bound_of(h, w, rgba ? 4 : 1);
    if (filt0 > kMaxFiltered || stripe0 > kMaxStripes) return dm4d_set_error(DM4D_ERR_ARG, "png_encode: too many bytes or stripes in one batch");
    if (h > max_h) max_h = h;
    if (w > max_w) max_w = w;
    if (stripes > max_stripes) max_stripes = stripes;
  }
  const Layout l = layout_of(filt0, stripe0, n);
  if (workspace_bytes < l.total) return dm4d_set_error(DM4D_ERR_ARG, "png_encode: workspace too small (dm4d_png_ws_bytes)");
  if (blob_bytes < bound) return dm4d_set_error(DM4D_ERR_ARG, "png_encode: blob capacity below the sum of dm4d_png_bound");
  char* ws = (char*)workspace;
  uint8_t* filt = (uint8_t*)(ws + l.filt);
  uint16_t* tok = (uint16_t*)(ws + l.tok);
  uint32_t* recs = (uint32_t*)(ws + l.recs);
  uint32_t* clen = (uint32_t*)(ws + l.clen);
  uint32_t* adler = (uint32_t*)(ws + l.adler);
  int64_t* offs = out;
  int64_t* lens = out + n;
  hipStream_t st = (hipStream_t)stream;
  const dim3 per_stripe((unsigned)max_stripes, (unsigned)n);
  int rc;
  hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)((max_w + kThreads - 1) / kThreads), (unsigned)max_h, (unsigned)n), dim3(kThreads), 0, st,
                     desc_dev, (const uint8_t*)planes, (const uint8_t*)rgb, filt);
  if ((rc = dm4d_check_launch("png_filter_kernel"))) return rc;
  hipLaunchKernelGGL(png_stripe_kernel, per_stripe, dim3(kThreads), 0, st, desc_dev, (const uint8_t*)filt, tok, recs, clen);
  if ((rc = dm4d_check_launch("png_stripe_kernel"))) return rc;
  hipLaunchKernelGGL(png_scan_kernel, dim3((unsigned)n), dim3(kScanThreads), 0, st, desc_dev, (const uint32_t*)recs, clen, adler, lens);
  if ((rc = dm4d_check_launch("png_scan_kernel"))) return rc;
  hipLaunchKernelGGL(png_offsets_kernel, dim3(1), dim3(kScanThreads), 0, st, (const int64_t*)lens, offs, n);
  if ((rc = dm4d_check_launch("png_offsets_kernel"))) return rc;
  hipLaunchKernelGGL(png_emit_kernel, per_stripe, dim3(kThreads), 0, st, desc_dev, (const uint16_t*)tok, (const uint32_t*)recs,
                     (const uint32_t*)clen, (const uint32_t*)adler, (const int64_t*)offs, (const int64_t*)lens, (uint8_t*)blob);
  return dm4d_check_launch("png_emit_kernel");
}
