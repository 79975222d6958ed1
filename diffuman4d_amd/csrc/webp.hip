// Lossless WebP files on the device: a batch of packed 8-bit RGB images of different sizes -> complete files (RIFF framing, one VP8L chunk)
// in one blob.  The definition is tests/webp_model.py (DESIGN.md "Device WebP (lossless)"): no transform, no colour cache, one group of
// five prefix codes per image; a pixel's kind -- U (equals the pixel above), else L (equals the pixel before), else literal -- is a
// function of the pixels alone; within a stripe of DM4D_WEBP_STRIPE_PIXELS pixels a maximal run of one kind is cut into backward
// references of at most 4096 pixels (distance plane code 1 or 2).
//
// Five launches on one stream for the whole batch; launch boundaries are the only ordering between workgroups.  The run finder of
// `tokens`, the bit window of `emit` and the body of `offsets` are stripe_emit.h's, shared with png.hip; the code lengths are
// prefix_code.h's:
//   tokens   one workgroup per stripe: kinds to LDS, run boundaries per lane segment, the token of every pixel to the workspace (uint16:
//            literal, kind + length of a reference, or none), the stripe's histograms (integer LDS atomics) and extra-bit count
//   image    one workgroup per image: the histograms summed, the five codes (prefix_code.h), the header and code tables, every stripe's
//            bit count (one wave per stripe) scanned to bit offsets, the file's length
//   offsets  one workgroup: the files' places in the blob
//   emit     one workgroup per stripe: tokens -> bits, OR-ed into an LDS window at positions from a prefix sum; the bytes the stripe
//            fills alone are stored, its first and last partial bytes recorded (stripes are not byte aligned, and may be empty)
//   seam     one workgroup per image: a byte shared by several pieces (the header, then the stripes) is written by the lane of the piece
//            that covers its first bit, which ORs in the recorded heads of the pieces that start inside it, in order
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
constexpr int kStripe = DM4D_WEBP_STRIPE_PIXELS;
constexpr int kMaxLen = 4096;
constexpr int kG = 0, kR = 280, kB = 536, kD = 792;  // the alphabets' places in a histogram or code table (alpha has one symbol: no place)
constexpr int kSyms = 794;
constexpr int kTabWords = kD + 40;                   // the image kernel's tables: the distance alphabet in full
constexpr int kXbits = kSyms;                        // word of a stripe record: the extra bits of its references
constexpr int kSrecWords = DM4D_WEBP_STRIPE_REC / 4;
constexpr int kIrecWords = DM4D_WEBP_IMAGE_REC / 4;
constexpr int kHdrAt = 800, kHdrWords = 192;         // 43 + 2023 + 2 x 1855 + 11 + 12 bits at most
constexpr int kMetaAt = kHdrAt + kHdrWords;          // header bits | payload bits lo, hi | 0
constexpr int kPer = 8;                              // pixels per lane and round of the emitter
constexpr int kWinWords = 2884;                      // 7 + 2048 x 45 bits and slack
constexpr int kFraming = 20;                         // RIFF, size, WEBP, VP8L, size
constexpr uint16_t kNone = 0xffffu, kLiteral = 0x8000u, kLeft = 0x4000u;
static_assert(kSyms + 1 <= kSrecWords && kMetaAt + 4 <= kIrecWords && kSyms <= kHdrAt, "record layouts");
static_assert(kThreads == kPrefixThreads && 280 <= kPrefixMaxSyms, "prefix_code.h is written for this workgroup and alphabet");
static_assert(kStripe % kThreads == 0 && kMaxLen <= 4096, "a token holds length - 1 in 12 bits");

enum { W_H = 0, W_W, W_PIX, W_STRIDE, W_PIX0, W_STRIPE0 };
__device__ const uint8_t kClOrder[19] = {17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};

struct Image {
  int h, w, N, stripes;
  int64_t pix, stride, pix0, stripe0;
};

__device__ __forceinline__ Image image_of(const int64_t* __restrict__ desc, int i) {
  const int64_t* d = desc + (int64_t)i * DM4D_WEBP_FIELDS;
  Image im;
  im.h = (int)d[W_H], im.w = (int)d[W_W];
  im.N = im.h * im.w;  // at most 16383^2 < 2^31
  im.stripes = (im.N + kStripe - 1) / kStripe;
  im.pix = d[W_PIX], im.stride = d[W_STRIDE], im.pix0 = d[W_PIX0], im.stripe0 = d[W_STRIPE0];
  return im;
}

__device__ __forceinline__ const uint8_t* pixel_at(const uint8_t* __restrict__ rgb, const Image& im, int p) {
  const int y = p / im.w, x = p - y * im.w;
  return rgb + im.pix + (int64_t)y * im.stride + 3 * x;
}

__device__ __forceinline__ bool same(const uint8_t* a, const uint8_t* b) { return a[0] == b[0] && a[1] == b[1] && a[2] == b[2]; }

// prefix symbol, number of extra bits and their value of a length 1 .. 4096
__device__ __forceinline__ void length_prefix(int len, int& sym, int& extra, uint32_t& ev) {
  if (len <= 4) {
    sym = len - 1, extra = 0, ev = 0;
    return;
  }
  const uint32_t v = (uint32_t)len - 1u;
  const int hb = 31 - __clz(v);
  sym = 2 * hb + (int)((v >> (hb - 1)) & 1u), extra = hb - 1, ev = v & ((1u << extra) - 1u);
}

// -- tokens ------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) webp_tokens_kernel(const int64_t* __restrict__ desc, const uint8_t* __restrict__ rgb,
                                                               uint16_t* __restrict__ tok, uint32_t* __restrict__ srecs) {
  __shared__ uint8_t kind[kStripe];  // 0 literal, 1 U, 2 L
  __shared__ uint32_t hist[kSrecWords];
  __shared__ int sh_first[kThreads], sh_last[kThreads];
  const Image im = image_of(desc, blockIdx.y);
  const int s = blockIdx.x;
  if (s >= im.stripes) return;
  const int tid = threadIdx.x;
  const int p0 = s * kStripe, P = min(kStripe, im.N - p0);
  uint16_t* tk = tok + im.pix0 + p0;
  for (int i = tid; i < kSrecWords; i += kThreads) hist[i] = 0;
  for (int i = tid; i < P; i += kThreads) {
    const int p = p0 + i;
    const uint8_t* c = pixel_at(rgb, im, p);
    int k = 0;
    if (p >= im.w && same(c, pixel_at(rgb, im, p - im.w)))
      k = 1;
    else if (p >= 1 && same(c, pixel_at(rgb, im, p - 1)))
      k = 2;
    kind[i] = (uint8_t)k;
  }
  __syncthreads();
  // pass 1: the runs that reach over this lane's segment [a, b) (stripe_emit.h; a literal is a run of its own)
  const LaneRuns lr = lane_runs<kThreads>(
      P, sh_first, sh_last, [&](int i) { return (int)kind[i]; }, [](int prev, int k) { return k == 0 || k != prev; }, [](int, int) {});
  const int a = lr.a, b = lr.b, s_in = lr.s_in, e_out = lr.e_out;
  // pass 2: run by run; every position gets its token
  for (int i = a; i < b;) {
    const int k = kind[i];
    if (k == 0) {
      const uint8_t* c = pixel_at(rgb, im, p0 + i);
      tk[i] = kLiteral;
      atomicAdd(&hist[kG + c[1]], 1u), atomicAdd(&hist[kR + c[0]], 1u), atomicAdd(&hist[kB + c[2]], 1u);
      ++i;
      continue;
    }
    const int rs = (i == 0 || kind[i - 1] != k) ? i : s_in;  // only the segment's first position can lie inside a run
    int e = i + 1;
    while (e < b && kind[e] == k) ++e;
    const int re = e < b ? e : e_out;
    for (int p = i; p < e; ++p) {
      uint16_t t = kNone;
      if (((p - rs) & (kMaxLen - 1)) == 0) {
        const int len = min(kMaxLen, re - p);
        int sym, extra;
        uint32_t ev;
        length_prefix(len, sym, extra, ev);
        t = (uint16_t)((k == 2 ? kLeft : 0) | (len - 1));
        atomicAdd(&hist[kG + 256 + sym], 1u), atomicAdd(&hist[kD + k - 1], 1u);
        if (extra) atomicAdd(&hist[kXbits], (uint32_t)extra);
      }
      tk[p] = t;
    }
    i = e;
  }
  __syncthreads();
  uint32_t* rec = srecs + (im.stripe0 + s) * kSrecWords;
  for (int i = tid; i < kSrecWords; i += kThreads) rec[i] = hist[i];
}

// -- per image: codes, header, bit offsets, file length -----------------------------------------------------------------------------------
// One code's description to the header and its table (length << 16 | bits as they enter the stream; all zero where a use costs no bits)
// to codes[0 .. nsym).  Called by every lane; hist[0 .. nsym) is the code's histogram.
__device__ void write_code(const uint32_t* hist, int nsym, uint32_t* codes, BitOut& o, uint32_t* work, uint8_t* lens, uint32_t* clfreq,
                           uint8_t* cllens, uint32_t* clcodes, HuffScratch& sc, int& shared_flag) {
  const int tid = threadIdx.x;
  for (int i = tid; i < nsym; i += kThreads) work[i] = hist[i];
  __syncthreads();
  build_lengths(work, nsym, 15, lens, sc);
  __syncthreads();
  if (tid == 0) {
    const int n = sc.n;
    int lo = 0, hi = 0;
    if (n >= 1) lo = hi = sc.order[0];
    if (n == 2) lo = min(lo, (int)sc.order[1]), hi = max(hi, (int)sc.order[1]);
    const bool simple = n <= 2 && hi < 256;
    if (simple) {
      const int wide = lo < 2 ? 0 : 1;
      o.put(1, 1), o.put(n == 2 ? 1 : 0, 1), o.put((uint32_t)wide, 1), o.put((uint32_t)lo, wide ? 8 : 1);
      if (n == 2) o.put((uint32_t)hi, 8);
    } else {
      for (int i = 0; i < 19; ++i) clfreq[i] = 0;
      for (int i = 0; i < nsym; ++i) ++clfreq[lens[i]];
    }
    canonical_codes(lens, nsym, codes);
    if (n <= 1)
      for (int i = 0; i < nsym; ++i) codes[i] = 0;
    shared_flag = simple ? 0 : 1;
  }
  __syncthreads();
  if (!shared_flag) return;  // the same for every lane
  build_lengths(clfreq, 19, 7, cllens, sc);
  __syncthreads();
  if (tid == 0) {
    const bool one = sc.n == 1;
    canonical_codes(cllens, 19, clcodes);
    o.put(0, 1), o.put(15, 4);
    for (int i = 0; i < 19; ++i) o.put(cllens[kClOrder[i]], 3);
    o.put(0, 1);
    if (!one)
      for (int i = 0; i < nsym; ++i) {
        const uint32_t e = clcodes[lens[i]];
        o.put(e & 0xffffu, (int)(e >> 16));
      }
  }
  __syncthreads();
}

__global__ void __launch_bounds__(kThreads) webp_image_kernel(const int64_t* __restrict__ desc, const uint32_t* __restrict__ srecs,
                                                              uint32_t* __restrict__ irecs, uint64_t* __restrict__ bits,
                                                              uint32_t* __restrict__ seam, int64_t* __restrict__ lens_out) {
  __shared__ uint32_t hist[kTabWords], codes[kTabWords], work[kPrefixMaxSyms], clfreq[20], clcodes[20], hdr[kHdrWords];
  __shared__ uint8_t lens[kPrefixMaxSyms], cllens[20];
  __shared__ HuffScratch sc;
  __shared__ int flag, hdr_bits_s;
  const Image im = image_of(desc, blockIdx.x);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t* rec0 = srecs + im.stripe0 * kSrecWords;
  for (int i = tid; i < kTabWords; i += kThreads) {
    uint32_t sum = 0;
    if (i < kSyms)
      for (int s = 0; s < im.stripes; ++s) sum += rec0[(int64_t)s * kSrecWords + i];
    hist[i] = sum, codes[i] = 0;
  }
  for (int i = tid; i < kHdrWords; i += kThreads) hdr[i] = 0;
  __syncthreads();
  BitOut o{hdr, 0};  // lane 0's is the one that counts
  if (tid == 0) {
    o.put(0x2f, 8), o.put((uint32_t)(im.w - 1), 14), o.put((uint32_t)(im.h - 1), 14), o.put(0, 1), o.put(0, 3);
    o.put(0, 1), o.put(0, 1), o.put(0, 1);  // no transform, no colour cache, no meta prefix image
  }
  write_code(hist + kG, 280, codes + kG, o, work, lens, clfreq, cllens, clcodes, sc, flag);
  write_code(hist + kR, 256, codes + kR, o, work, lens, clfreq, cllens, clcodes, sc, flag);
  write_code(hist + kB, 256, codes + kB, o, work, lens, clfreq, cllens, clcodes, sc, flag);
  if (tid == 0) o.put(1, 1), o.put(0, 1), o.put(1, 1), o.put(255, 8);  // alpha: the one symbol 255
  write_code(hist + kD, 40, codes + kD, o, work, lens, clfreq, cllens, clcodes, sc, flag);  // of its 40 symbols two are ever used
  if (tid == 0) hdr_bits_s = o.pos;
  __syncthreads();
  const int hdr_bits = hdr_bits_s;
  // bits of every stripe: one wave per stripe
  const int64_t piece0 = im.stripe0 + blockIdx.x;
  uint64_t* pb = bits + piece0;
  for (int s = wave; s < im.stripes; s += kThreads / 64) {
    const uint32_t* rec = rec0 + (int64_t)s * kSrecWords;
    uint64_t sum = 0;
    for (int i = lane; i < kSyms; i += 64) sum += (uint64_t)rec[i] * (codes[i] >> 16);
    for (int off = 32; off; off >>= 1) sum += __shfl_down(sum, off);
    if (lane == 0) pb[1 + s] = sum + rec[kXbits];
  }
  if (tid == 0) pb[0] = (uint64_t)hdr_bits;
  __syncthreads();
  const uint64_t total = block_excl_scan_inplace<uint64_t, kThreads>(pb, (int64_t)im.stripes + 1);
  uint32_t* irec = irecs + (int64_t)blockIdx.x * kIrecWords;
  for (int i = tid; i < kHdrAt; i += kThreads) irec[i] = codes[i];
  for (int i = tid; i < kHdrWords; i += kThreads) irec[kHdrAt + i] = hdr[i];
  if (tid == 0) {
    irec[kMetaAt] = (uint32_t)hdr_bits, irec[kMetaAt + 1] = (uint32_t)total, irec[kMetaAt + 2] = (uint32_t)(total >> 32), irec[kMetaAt + 3] = 0;
    seam[2 * piece0] = 0;
    seam[2 * piece0 + 1] = (hdr_bits & 7) ? (hdr[hdr_bits >> 5] >> (hdr_bits & 24)) & 0xffu : 0u;  // the header's last, partial byte
    const int64_t payload = (int64_t)((total + 7) >> 3);
    lens_out[blockIdx.x] = kFraming + payload + (payload & 1);
  }
}

// ONE block: offs[i] = sum of lens[0 .. i)
__global__ void __launch_bounds__(kScanThreads) webp_offsets_kernel(const int64_t* __restrict__ lens, int64_t* __restrict__ offs, int n) {
  offsets_block<kScanThreads>(lens, offs, n);
}

// -- emit ----------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void put_le32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)v, p[1] = (uint8_t)(v >> 8), p[2] = (uint8_t)(v >> 16), p[3] = (uint8_t)(v >> 24);
}

__global__ void __launch_bounds__(kThreads) webp_emit_kernel(const int64_t* __restrict__ desc, const uint8_t* __restrict__ rgb,
                                                             const uint16_t* __restrict__ tok, const uint32_t* __restrict__ irecs,
                                                             const uint64_t* __restrict__ bits, uint32_t* __restrict__ seam,
                                                             const int64_t* __restrict__ offs, uint8_t* __restrict__ blob) {
  __shared__ uint32_t tab[kHdrAt], win[kWinWords], wave_tot[kThreads / 64];
  const Image im = image_of(desc, blockIdx.y);
  const int s = blockIdx.x;
  if (s >= im.stripes) return;
  const int tid = threadIdx.x;
  const int p0 = s * kStripe, P = min(kStripe, im.N - p0);
  const uint16_t* tk = tok + im.pix0 + p0;
  const uint32_t* irec = irecs + (int64_t)blockIdx.y * kIrecWords;
  const int64_t piece = im.stripe0 + blockIdx.y + 1 + s;
  const uint64_t total = (uint64_t)irec[kMetaAt + 1] | ((uint64_t)irec[kMetaAt + 2] << 32);
  const uint64_t begin = bits[piece];
  const uint64_t cap = (total + 7) >> 3;  // bytes of the payload
  uint8_t* file = blob + offs[blockIdx.y];
  uint8_t* out = file + kFraming + (begin >> 3);  // the byte the stripe's first bit lies in
  const uint64_t room = cap - (begin >> 3);      // begin <= total
  const bool head_partial = (begin & 7) != 0;
  for (int i = tid; i < kHdrAt; i += kThreads) tab[i] = irec[i];
  for (int i = tid; i < kWinWords; i += kThreads) win[i] = 0;
  if (s == 0) {  // the framing and the header's whole bytes
    const uint32_t hdr_bytes = irec[kMetaAt] >> 3;
    const uint8_t* hdr = reinterpret_cast<const uint8_t*>(irec + kHdrAt);
    for (uint32_t i = tid; i < hdr_bytes; i += kThreads)
      if (i < cap) file[kFraming + i] = hdr[i];
    if (tid == 0) {
      const uint32_t padded = (uint32_t)(cap + (cap & 1));
      file[0] = 'R', file[1] = 'I', file[2] = 'F', file[3] = 'F';
      put_le32(file + 4, 12u + padded);
      file[8] = 'W', file[9] = 'E', file[10] = 'B', file[11] = 'P', file[12] = 'V', file[13] = 'P', file[14] = '8', file[15] = 'L';
      put_le32(file + 16, (uint32_t)cap);
    }
  }
  __syncthreads();
  uint64_t done = 0;
  int carry_bits = (int)(begin & 7);
  uint32_t head = 0;
  emit_window<kThreads, kPer, kWinWords, uint64_t>(
      P, win, wave_tot, carry_bits, done,
      [&](int q, uint64_t& v, int& nb) {
        const uint32_t t = q < P ? tk[q] : kNone;
        if (t == kLiteral) {
          const uint8_t* c = pixel_at(rgb, im, p0 + q);
          const uint32_t eg = tab[kG + c[1]], er = tab[kR + c[0]], eb = tab[kB + c[2]];
          const int lg = (int)(eg >> 16), lr = (int)(er >> 16), lb = (int)(eb >> 16);
          v = (uint64_t)(eg & 0xffffu) | ((uint64_t)(er & 0xffffu) << lg) | ((uint64_t)(eb & 0xffffu) << (lg + lr));
          nb = lg + lr + lb;
        } else if (t != kNone) {
          int sym, extra;
          uint32_t ev;
          length_prefix((int)(t & 0xfffu) + 1, sym, extra, ev);
          const uint32_t e = tab[kG + 256 + sym], d = tab[kD + ((t & kLeft) ? 1 : 0)];
          const int l = (int)(e >> 16);
          v = (uint64_t)(e & 0xffffu) | ((uint64_t)ev << l) | ((uint64_t)(d & 0xffffu) << (l + extra));
          nb = l + extra + (int)(d >> 16);
        }
      },
      [&](uint64_t i, uint32_t byte) {
        if (i == 0 && head_partial)
          head = byte;  // lane 0: the stripe's first byte holds bits of the piece before it
        else if (i < room)
          out[i] = (uint8_t)byte;
      });
  if (tid == 0) {
    // the last, partial byte: the stripe's tail -- or its head, where the whole stripe lies inside the byte it starts in
    uint32_t tail = 0;
    const uint32_t rest = carry_bits ? win[0] & 0xffu : 0u;
    if (done == 0 && head_partial)
      head = rest;
    else
      tail = rest;
    seam[2 * piece] = head, seam[2 * piece + 1] = tail;
  }
}

// -- seam bytes ----------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) webp_seam_kernel(const int64_t* __restrict__ desc, const uint32_t* __restrict__ irecs,
                                                             const uint64_t* __restrict__ bits, const uint32_t* __restrict__ seam,
                                                             const int64_t* __restrict__ offs, uint8_t* __restrict__ blob) {
  const Image im = image_of(desc, blockIdx.x);
  const uint32_t* irec = irecs + (int64_t)blockIdx.x * kIrecWords;
  const int64_t piece0 = im.stripe0 + blockIdx.x;
  const uint64_t total = (uint64_t)irec[kMetaAt + 1] | ((uint64_t)irec[kMetaAt + 2] << 32);
  const uint64_t cap = (total + 7) >> 3;
  uint8_t* payload = blob + offs[blockIdx.x] + kFraming;
  const int pieces = im.stripes + 1;  // the header, then the stripes
  for (int t = threadIdx.x; t < pieces; t += kThreads) {
    const uint64_t begin = bits[piece0 + t], end = t + 1 < pieces ? bits[piece0 + t + 1] : total;
    const uint64_t byte = end >> 3;
    // this piece writes the byte its last bit lies in if it does not fill it and covers its first bit
    if (end == begin || (end & 7) == 0 || begin > 8 * byte) continue;
    uint32_t val = seam[2 * (piece0 + t) + 1];
    for (int u = t + 1; u < pieces; ++u) {  // the pieces that start inside the byte, in order
      if (bits[piece0 + u] >= 8 * byte + 8) break;
      val |= seam[2 * (piece0 + u)];
    }
    if (byte < cap) payload[byte] = (uint8_t)val;
  }
  if (threadIdx.x == 0 && (cap & 1)) payload[cap] = 0;  // RIFF chunks are padded to an even length
}

// -- host ----------------------------------------------------------------------------------------------------------------------------------
bool side_ok(int64_t v) { return v >= 1 && v <= DM4D_WEBP_MAX_SIDE; }
int64_t stripes_of(int64_t h, int64_t w) { return (h * w + kStripe - 1) / kStripe; }
int64_t bound_of(int64_t h, int64_t w) { return 800 + 6 * h * w; }
constexpr int64_t kMaxPixels = 1ll << 38;
constexpr int64_t kMaxStripes = 1ll << 26;

// workspace: tokens | stripe records | image records | bit offsets of the pieces | their partial bytes
struct Layout {
  int64_t tok, srecs, irecs, bits, seam, total;
};
Layout layout_of(int64_t pixels, int64_t stripes, int64_t n) {
  Layout l;
  l.tok = 0;
  l.srecs = l.tok + pad16(pixels * 2);
  l.irecs = l.srecs + stripes * DM4D_WEBP_STRIPE_REC;
  l.bits = l.irecs + n * DM4D_WEBP_IMAGE_REC;
  l.seam = l.bits + pad16((stripes + n) * 8);
  l.total = l.seam + pad16((stripes + n) * 8);
  return l;
}

}  // namespace

extern "C" size_t dm4d_webp_bound(int h, int w) {
  if (!side_ok(h) || !side_ok(w)) return 0;
  return (size_t)bound_of(h, w);
}

extern "C" size_t dm4d_webp_ws_bytes(int64_t pixels, int64_t stripes, int n) {
  if (pixels < 1 || pixels > kMaxPixels || stripes < 1 || stripes > kMaxStripes || n <= 0 || n > 65535 || stripes < n || pixels < stripes) return 0;
  return (size_t)layout_of(pixels, stripes, n).total;
}

extern "C" int dm4d_webp_encode_u8(void* stream, const void* rgb, int64_t rgb_bytes, const int64_t* desc_host, const int64_t* desc_dev, int n,
                                   void* workspace, int64_t workspace_bytes, void* blob, int64_t blob_bytes, int64_t* out) {
  if (!rgb || !desc_host || !desc_dev || !workspace || !blob || !out) return dm4d_set_error(DM4D_ERR_ARG, "webp_encode: null pointer");
  if (n <= 0 || n > 65535) return dm4d_set_error(DM4D_ERR_ARG, "webp_encode: empty or oversized batch");
  if (((uintptr_t)workspace & 15) || ((uintptr_t)out & 7)) return dm4d_set_error(DM4D_ERR_ARG, "webp_encode: workspace must be 16-byte aligned, out 8-byte");
  if (rgb_bytes <= 0) return dm4d_set_error(DM4D_ERR_ARG, "webp_encode: a buffer size is not positive");
  int64_t pix0 = 0, stripe0 = 0, bound = 0, max_stripes = 0;
  for (int i = 0; i < n; ++i) {
    const int64_t* d = desc_host + (int64_t)i * DM4D_WEBP_FIELDS;
    const int64_t h = d[W_H], w = d[W_W], off = d[W_PIX], stride = d[W_STRIDE];
    if (!side_ok(h) || !side_ok(w)) return dm4d_set_error(DM4D_ERR_ARG, "webp_encode: a dimension outside 1..DM4D_WEBP_MAX_SIDE in a descriptor");
    if (stride < 3 * w || stride > (1ll << 32)) return dm4d_set_error(DM4D_ERR_ARG, "webp_encode: a row stride below 3 w (or above 2^32) in a descriptor");
    if (!plane_ok(off, stride, h, 3 * w, rgb_bytes))
      return dm4d_set_error(DM4D_ERR_ARG, "webp_encode: an image lies outside its buffer");
    if (d[W_PIX0] != pix0 || d[W_STRIPE0] != stripe0) return dm4d_set_error(DM4D_ERR_ARG, "webp_encode: a descriptor's first pixel or first stripe is not the running sum");
    for (int k = W_STRIPE0 + 1; k < DM4D_WEBP_FIELDS; ++k)
      if (d[k] != 0) return dm4d_set_error(DM4D_ERR_ARG, "webp_encode: a descriptor's spare field is not zero");
    const int64_t stripes = stripes_of(h, w);
    pix0 += h * w, stripe0 += stripes, bound += bound_of(h, w);
    if (pix0 > kMaxPixels || stripe0 > kMaxStripes) return dm4d_set_error(DM4D_ERR_ARG, "webp_encode: too many pixels or stripes in one batch");
    if (stripes > max_stripes) max_stripes = stripes;
  }
  const Layout l = layout_of(pix0, stripe0, n);
  if (workspace_bytes < l.total) return dm4d_set_error(DM4D_ERR_ARG, "webp_encode: workspace too small (dm4d_webp_ws_bytes)");
  if (blob_bytes < bound) return dm4d_set_error(DM4D_ERR_ARG, "webp_encode: blob capacity below the sum of dm4d_webp_bound");
  char* ws = (char*)workspace;
  uint16_t* tok = (uint16_t*)(ws + l.tok);
  uint32_t* srecs = (uint32_t*)(ws + l.srecs);
  uint32_t* irecs = (uint32_t*)(ws + l.irecs);
  uint64_t* bits = (uint64_t*)(ws + l.bits);
  uint32_t* seam = (uint32_t*)(ws + l.seam);
  int64_t* offs = out;
  int64_t* lens = out + n;
  hipStream_t st = (hipStream_t)stream;
  const dim3 per_stripe((unsigned)max_stripes, (unsigned)n);
  const uint8_t* px = (const uint8_t*)rgb;
  int rc;
  hipLaunchKernelGGL(webp_tokens_kernel, per_stripe, dim3(kThreads), 0, st, desc_dev, px, tok, srecs);
  if ((rc = dm4d_check_launch("webp_tokens_kernel"))) return rc;
  hipLaunchKernelGGL(webp_image_kernel, dim3((unsigned)n), dim3(kThreads), 0, st, desc_dev, (const uint32_t*)srecs, irecs, bits, seam, lens);
  if ((rc = dm4d_check_launch("webp_image_kernel"))) return rc;
  hipLaunchKernelGGL(webp_offsets_kernel, dim3(1), dim3(kScanThreads), 0, st, (const int64_t*)lens, offs, n);
  if ((rc = dm4d_check_launch("webp_offsets_kernel"))) return rc;
  hipLaunchKernelGGL(webp_emit_kernel, per_stripe, dim3(kThreads), 0, st, desc_dev, px, (const uint16_t*)tok, (const uint32_t*)irecs,
                     (const uint64_t*)bits, seam, (const int64_t*)offs, (uint8_t*)blob);
  if ((rc = dm4d_check_launch("webp_emit_kernel"))) return rc;
  hipLaunchKernelGGL(webp_seam_kernel, dim3((unsigned)n), dim3(kThreads), 0, st, desc_dev, (const uint32_t*)irecs, (const uint64_t*)bits,
                     (const uint32_t*)seam, (const int64_t*)offs, (uint8_t*)blob);
  return dm4d_check_launch("webp_seam_kernel");
}
