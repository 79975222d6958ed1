// 8-bit PNG files decoded on the device: what np.asarray(Image.open(file)) of Pillow gives for a file of the supported set
// (host/pngdec.py::probe: bit depth 8, colour type 0, 2 or 6, not interlaced), for a batch of files of different sizes and colour types.
// All of it is integer arithmetic with one right answer (DESIGN.md "Device PNG decode"; tests/pngdec_model.py is the same definition
// in numpy, with an emulation of exactly the scheme below).
//
// Decoder = two launches on one stream; the launch boundary is the only ordering between workgroups, there are no atomics, and an
// image's bytes depend on its file alone:
//   inflate   one workgroup of ONE wave per image (the batch is the parallelism across the device).  Where a token starts is known only
//             by decoding everything before it, so the wave walks the blocks and decodes the symbols in sequence, every lane holding
//             the same bit buffer; what is done by all lanes is the work per token: literals are gathered (lane k keeps the k-th) and
//             stored 64 at a time, and byte i of a match is window[start - dist + i mod dist], valid for dist < len too because
//             everything before `start` is final.  The last 32 KiB of output live in an LDS ring of 64 KiB; match sources are read
//             from the ring, never from global memory this launch wrote; whenever the output crosses a multiple of 32 KiB the half of
//             the ring that was just completed goes to the workspace with 16-byte stores and into the Adler-32.  The lookup tables of
//             a block (10 bits for literal/length, 8 for distance and for the code-length code; longer codes by the canonical
//             first-code / count walk) are built in LDS from the code lengths with ballots.
//   unfilter  one wave per image: a skewed wavefront over bands of 64 rows.  Lane j has row 64 b + j and is one pixel behind lane
//             j - 1, so the pixel above comes by __shfl_up from the register lane j - 1 stored a step earlier, and the pixel above-left
//             is the one it received a step before.  All five predictors are evaluated and selected by the row's filter byte.  The
//             last row of a band is kept in LDS for lane 0 of the next band (lane 63 writes pixel x 63 steps after lane 0 read it).
// Every loop is bounded by the stream's bit count, the image's expected output size or a constant, whatever the bits say; every read
// of the stream is masked by its length (bits beyond it are zeros); every store is below the image's expected size.
#include <stdint.h>

#include "common.h"
#include "dm4d.h"
#include "errors.h"
#include "stripe_emit.h"

namespace {

constexpr uint32_t kRing = DM4D_PNGDEC_RING_BYTES;
constexpr uint32_t kRingMask = kRing - 1u;
constexpr uint32_t kHalf = kRing / 2u;
constexpr int kHalfShift = 15;
constexpr int kLitBits = 10, kDistBits = 8;
constexpr int64_t kMaxWorkspace = 1ll << 40;
static_assert(kHalf == (1u << kHalfShift) && kHalf == 32768u, "a half of the ring is the DEFLATE window");

enum { D_STREAM = 0, D_BYTES, D_H, D_W, D_CHANNELS, D_OUT, D_OUT_CHANNELS, D_WS };
static_assert(D_WS + 1 == DM4D_PNGDEC_FIELDS, "descriptor");

struct Image {
  int64_t stream, out, ws;
  uint32_t nbytes, expect;  // bytes of the zlib stream; bytes of the filtered scanlines
  int h, w, bpp;
};

__host__ __device__ inline Image image_of(const int64_t* desc, int i) {
  const int64_t* d = desc + (int64_t)i * DM4D_PNGDEC_FIELDS;
  Image im;
  im.stream = d[D_STREAM], im.nbytes = (uint32_t)d[D_BYTES], im.out = d[D_OUT], im.ws = d[D_WS];
  im.h = (int)d[D_H], im.w = (int)d[D_W], im.bpp = (int)d[D_CHANNELS];
  im.expect = (uint32_t)(d[D_H] * (1 + d[D_W] * d[D_CHANNELS]));
  return im;
}

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// -- inflate -----------------------------------------------------------------------------------------------------------------------------
// The stream as 32-bit words, least significant bit first; the same in every lane.
// Memory latency is kept off the token loop: lane l holds word base + l of the current 64 words and of the 64 after them (two
// coalesced loads, the second in flight while the first is used), and the word the bit buffer needs next is read from its lane.
struct BitReader {
  const uint32_t* words;
  uint32_t nbytes, next;  // next = index of the word to load
  uint64_t hold;
  int have;
  uint32_t base, cur, ahead;  // cur = word base + lane, ahead = word base + 64 + lane

  __device__ __forceinline__ uint32_t load(uint32_t i) const {
    const uint64_t off = 4ull * i;
    if (off + 4u <= nbytes) return words[i];
    if (off < nbytes) return words[i] & ((1u << (8u * (nbytes - (uint32_t)off))) - 1u);  // the stream is padded to a multiple of 4
    return 0u;
  }
  __device__ __forceinline__ uint32_t word(uint32_t i) {  // i >= base, the same in every lane
    if (i >= base + 64u) {
      base += 64u, cur = ahead;
      ahead = load(base + 64u + threadIdx.x);
    }
    return (uint32_t)__builtin_amdgcn_readlane((int)cur, (int)(i - base));
  }
  __device__ __forceinline__ void seek(uint32_t byte) {
    next = byte >> 2, hold = 0, have = 0;
    base = next & ~63u;
    cur = load(base + threadIdx.x), ahead = load(base + 64u + threadIdx.x);
    refill();
    drop((int)(byte & 3u) * 8);
  }
  __device__ __forceinline__ void refill() {  // afterwards have >= 33
    if (have <= 32) {
      hold |= (uint64_t)word(next) << have;
      have += 32, next += 1u;
    }
  }
  __device__ __forceinline__ uint32_t peek(int n) const { return (uint32_t)hold & ((1u << n) - 1u); }
  __device__ __forceinline__ void drop(int n) { hold >>= n, have -= n; }
  __device__ __forceinline__ uint32_t take(int n) {
    const uint32_t v = peek(n);
    drop(n);
    return v;
  }
  __device__ __forceinline__ uint64_t bitpos() const { return 32ull * next - (uint64_t)have; }
  __device__ __forceinline__ bool over() const { return bitpos() > 8ull * nbytes; }
};

struct Code {
  uint16_t sorted[288];  // the symbols in canonical order: by length, then by value
  uint16_t first_code[16], first_idx[16], count[16];
};

struct Inflate {
  alignas(16) uint8_t ring[kRing];  // byte p of the output is ring[p & kRingMask]; halves are read 16 bytes at a time
  uint16_t lit[1 << kLitBits];  // the next bits -> (symbol << 4) | length of the code they start with; 0 = a longer code or none
  uint16_t dist[1 << kDistBits];
  Code code[2];  // [0] literal/length, [1] distance (and the code-length code while a block's header is read)
  uint8_t lens[320];  // a block's literal/length code lengths, then its distance code lengths
  uint8_t cl[32];     // the code-length code's own lengths
};

// zlib's inflate_table on the code lengths lens[0 .. n): the primary table of `bits` bits and the canonical walk's arrays.
// -> 0 valid; 1 over-subscribed; 2 incomplete (the caller decides: a single 1-bit code is accepted for the two data codes); max_len out.
__device__ int build_code(const uint8_t* lens, int n, Code& cd, uint16_t* table, int bits, int& max_len) {
  const int lane = threadIdx.x;
  for (int i = lane; i < (1 << bits); i += 64) table[i] = 0;
  int cnt[16];
#pragma unroll
  for (int l = 0; l < 16; ++l) cnt[l] = 0;
  for (int s0 = 0; s0 < n; s0 += 64) {
    const int l = s0 + lane < n ? (int)lens[s0 + lane] : 0;
#pragma unroll
    for (int L = 1; L < 16; ++L) cnt[L] += __popcll(__ballot(l == L));
  }
  int left = 1, fc[16], fi[16];
  bool oversub = false;
  max_len = 0;
  int code = 0, idx = 0;
#pragma unroll
  for (int L = 1; L < 16; ++L) {
    left = 2 * left - cnt[L];
    oversub |= left < 0;
    if (left < 0) left = 0;
    if (cnt[L]) max_len = L;
    code = (code + cnt[L - 1]) << 1;
    fc[L] = L == 1 ? 0 : code;
    fi[L] = idx;
    idx += cnt[L];
  }
  if (oversub) return 1;
  if (lane < 16) {
    int c = 0, f = 0, k = 0;
#pragma unroll
    for (int L = 1; L < 16; ++L)
      if (lane == L) c = cnt[L], f = fc[L], k = fi[L];
    cd.count[lane] = (uint16_t)c, cd.first_code[lane] = (uint16_t)f, cd.first_idx[lane] = (uint16_t)k;
  }
  int run[16];
#pragma unroll
  for (int l = 0; l < 16; ++l) run[l] = 0;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int s0 = 0; s0 < n; s0 += 64) {
    const int sym = s0 + lane;
    const int l = sym < n ? (int)lens[sym] : 0;
#pragma unroll
    for (int L = 1; L < 16; ++L) {
      const unsigned long long m = __ballot(l == L);
      if (l == L) {
        const int r = run[L] + __popcll(m & below);
        cd.sorted[fi[L] + r] = (uint16_t)sym;
        if (L <= bits) {
          const uint32_t c = (uint32_t)(fc[L] + r);
          const uint32_t rev = __brev(c) >> (32 - L);
          const uint16_t e = (uint16_t)((sym << 4) | L);
          for (uint32_t j = rev; j < (1u << bits); j += 1u << L) table[j] = e;
        }
      }
      run[L] += __popcll(m);
    }
  }
  __syncthreads();
  return left > 0 ? 2 : 0;
}

// The symbol the next bits start, and its length; len = 0: no code of the set starts them.
__device__ __forceinline__ void decode_sym(const BitReader& br, const uint16_t* table, int bits, const Code& cd, int& sym, int& len) {
  const uint32_t e = uni(table[br.peek(bits)]);
  if (e) {
    sym = (int)(e >> 4), len = (int)(e & 15u);
    return;
  }
  const uint32_t rev = __brev(br.peek(15)) >> 17;  // the next 15 bits, first bit on top
  sym = 0, len = 0;
  for (int l = bits + 1; l <= 15; ++l) {
    const uint32_t c = rev >> (15 - l);
    const uint32_t first = uni(cd.first_code[l]), count = uni(cd.count[l]);
    if (c >= first && c - first < count) {
      sym = (int)uni(cd.sorted[uni(cd.first_idx[l]) + (c - first)]), len = l;
      return;
    }
  }
}

struct Writer {
  uint8_t* ring;
  uint8_t* dst;     // the image's filtered stream in the workspace, 16-byte aligned
  uint32_t expect;  // its size: no byte at or beyond it is produced
  uint32_t pos;     // bytes produced (those of pending literals not counted)
  uint32_t s1, s2;  // Adler-32 of the flushed bytes
  int nlit;         // pending literals: lane k holds the k-th in `mine`
  uint32_t mine;

  // bytes [k * kHalf, k * kHalf + n) of the output, which lie in half k & 1 of the ring: to the workspace and into the checksum
  __device__ void flush(uint32_t k, uint32_t n) {
    __syncthreads();
    const int lane = threadIdx.x;
    const uint8_t* src = ring + (k & 1u) * kHalf;
    uint8_t* to = dst + (uint64_t)k * kHalf;
    uint32_t sum = 0;
    unsigned long long weighted = 0;
    for (uint32_t off = 16u * lane; off + 16u <= n; off += 1024u) {
      const U4 v = *reinterpret_cast<const U4*>(src + off);
      stg16(to + off, v);
      const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const uint32_t b = (wd[j >> 2] >> (8 * (j & 3))) & 255u;
        sum += b;
        weighted += (unsigned long long)(n - off - j) * b;
      }
    }
    for (uint32_t i = (n & ~15u) + lane; i < n; i += 64u) {
      const uint32_t b = src[i];
      to[i] = (uint8_t)b;
      sum += b;
      weighted += (unsigned long long)(n - i) * b;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      sum += __shfl_xor(sum, o);
      weighted += __shfl_xor(weighted, o);
    }
    const unsigned long long t2 = (unsigned long long)s2 + (unsigned long long)n * s1 + weighted;
    s2 = uni((uint32_t)(t2 % 65521ull));
    s1 = uni((s1 + sum) % 65521u);
    __syncthreads();
  }
  // n <= kHalf bytes were stored at pos: at most one half was completed
  __device__ __forceinline__ void produced(uint32_t n) {
    const uint32_t to = pos + n;
    if ((to >> kHalfShift) != (pos >> kHalfShift)) flush(pos >> kHalfShift, kHalf);
    pos = to;
  }
  __device__ __forceinline__ void flush_literals() {
    if (nlit == 0) return;
    if ((int)threadIdx.x < nlit) ring[(pos + threadIdx.x) & kRingMask] = (uint8_t)mine;
    produced((uint32_t)nlit);
    nlit = 0;
  }
  __device__ __forceinline__ void finish() {
    flush_literals();
    const uint32_t k = pos >> kHalfShift;
    if (pos > k * kHalf) flush(k, pos - k * kHalf);
  }
};

__global__ void __launch_bounds__(64) pngdec_inflate_kernel(const int64_t* __restrict__ desc, const uint8_t* __restrict__ streams,
                                                            uint8_t* __restrict__ workspace, int32_t* __restrict__ status) {
  __shared__ Inflate s;
  const Image im = image_of(desc, blockIdx.x);
  const int lane = threadIdx.x;
  BitReader br;
  br.words = reinterpret_cast<const uint32_t*>(streams + im.stream), br.nbytes = im.nbytes;
  br.seek(0);
  Writer wr{s.ring, workspace + im.ws, im.expect, 0u, 1u, 0u, 0, 0u};
  int st = 0;
  {
    const uint32_t cmf = br.take(8), flg = br.take(8);
    if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0u || (flg & 32u)) st |= DM4D_PNGDEC_ST_HEADER;
  }
  bool last = false;
  while (!st && !last) {  // a block consumes at least three bits
    br.refill();
    if (br.over()) {
      st |= DM4D_PNGDEC_ST_END;
      break;
    }
    last = br.take(1) != 0u;
    const uint32_t type = br.take(2);
    if (type == 3u) {
      st |= DM4D_PNGDEC_ST_BLOCK;
      break;
    }
    if (type == 0u) {
      br.drop(br.have & 7);  // to the byte boundary
      br.refill();
      const uint32_t len = br.take(16), nlen = br.take(16);
      if (len != (~nlen & 0xffffu)) {
        st |= DM4D_PNGDEC_ST_BLOCK;
        break;
      }
      const uint32_t from = (uint32_t)(br.bitpos() >> 3);
      wr.flush_literals();
      if (len > im.expect - wr.pos) {
        st |= DM4D_PNGDEC_ST_END;
        break;
      }
      const uint8_t* src = streams + im.stream;
      for (uint32_t off = 0; off < len; off += 64u) {
        const uint32_t i = off + lane;
        if (i < len) s.ring[(wr.pos + lane) & kRingMask] = from + i < im.nbytes ? src[from + i] : (uint8_t)0;
        wr.produced(min(64u, len - off));
      }
      br.seek(from + len);
      if (br.over()) {
        st |= DM4D_PNGDEC_ST_END;
        break;
      }
      continue;
    }
    int nl, nd;
    if (type == 1u) {
      nl = 288, nd = 32;
      for (int i = lane; i < 320; i += 64) s.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
    } else {
      nl = 257 + (int)br.take(5), nd = 1 + (int)br.take(5);
      const int ncl = 4 + (int)br.take(4);
      if (nl > 286 || nd > 30) {
        st |= DM4D_PNGDEC_ST_BLOCK;
        break;
      }
      // the code-length code: up to 19 lengths of 3 bits, for the symbols 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
      if (lane < 19) s.cl[lane] = 0;
      for (int i = 0; i < ncl; ++i) {
        br.refill();
        const uint32_t v = br.take(3);
        const int at = i < 3 ? 16 + i : i == 3 ? 0 : (i & 1) ? 7 - (i - 5) / 2 : 8 + (i - 4) / 2;
        if (lane == 0) s.cl[at] = (uint8_t)v;
      }
      __syncthreads();
      int max_len;
      if (build_code(s.cl, 19, s.code[1], s.dist, kDistBits, max_len) != 0) {  // must be complete
        st |= DM4D_PNGDEC_ST_BLOCK;
        break;
      }
      __syncthreads();
      // the nl + nd code lengths; every symbol gives at least one
      const int total = nl + nd;
      int i = 0, prev = 0;
      while (i < total) {
        br.refill();
        int sym, len;
        decode_sym(br, s.dist, kDistBits, s.code[1], sym, len);
        if (len == 0) {  // cannot happen with a complete code
          st |= DM4D_PNGDEC_ST_BLOCK;
          break;
        }
        br.drop(len);
        int rep = 1, val = sym;
        if (sym == 16) {
          if (i == 0) {
            st |= DM4D_PNGDEC_ST_BLOCK;
            break;
          }
          val = prev, rep = 3 + (int)br.take(2);
        } else if (sym == 17) {
          val = 0, rep = 3 + (int)br.take(3);
        } else if (sym == 18) {
          val = 0, rep = 11 + (int)br.take(7);
        }
        if (i + rep > total) {
          st |= DM4D_PNGDEC_ST_BLOCK;
          break;
        }
        for (int k = lane; k < rep; k += 64) s.lens[i + k] = (uint8_t)val;
        i += rep, prev = val;
      }
      if (st) break;
      __syncthreads();
      if (br.over()) {
        st |= DM4D_PNGDEC_ST_END;
        break;
      }
      if (uni(s.lens[256]) == 0u) {  // no end-of-block code
        st |= DM4D_PNGDEC_ST_BLOCK;
        break;
      }
    }
    __syncthreads();
    int max_len;
    int rc = build_code(s.lens, nl, s.code[0], s.lit, kLitBits, max_len);
    if (rc == 1 || (rc == 2 && max_len != 1)) {
      st |= DM4D_PNGDEC_ST_BLOCK;
      break;
    }
    rc = build_code(s.lens + nl, nd, s.code[1], s.dist, kDistBits, max_len);
    if (rc == 1 || (rc == 2 && max_len > 1)) {  // no distance code at all is accepted
      st |= DM4D_PNGDEC_ST_BLOCK;
      break;
    }
    __syncthreads();
    // the block's tokens; a token consumes at least one bit
    for (;;) {
      br.refill();
      if (br.over()) {
        st |= DM4D_PNGDEC_ST_END;
        break;
      }
      int sym, len;
      decode_sym(br, s.lit, kLitBits, s.code[0], sym, len);
      if (len == 0 || sym >= 286) {
        st |= DM4D_PNGDEC_ST_CODE;
        break;
      }
      br.drop(len);
      if (sym < 256) {
        if (wr.pos + (uint32_t)wr.nlit >= im.expect) {
          st |= DM4D_PNGDEC_ST_END;
          break;
        }
        if (lane == wr.nlit) wr.mine = (uint32_t)sym;
        if (++wr.nlit == 64) wr.flush_literals();
        continue;
      }
      if (sym == 256) break;
      const int k = sym - 257;
      const int lext = k < 8 || k == 28 ? 0 : (k >> 2) - 1;
      const uint32_t mlen = (k < 8 ? (uint32_t)k + 3u : k == 28 ? 258u : ((4u + (uint32_t)(k & 3)) << lext) + 3u) + br.take(lext);
      br.refill();
      int dsym, dlen;
      decode_sym(br, s.dist, kDistBits, s.code[1], dsym, dlen);
      if (dlen == 0 || dsym >= 30) {
        st |= DM4D_PNGDEC_ST_CODE;
        break;
      }
      br.drop(dlen);
      const int dext = dsym < 4 ? 0 : (dsym >> 1) - 1;
      const uint32_t d = (dsym < 4 ? (uint32_t)dsym + 1u : ((2u + (uint32_t)(dsym & 1)) << dext) + 1u) + br.take(dext);
      wr.flush_literals();
      if (d > wr.pos) {
        st |= DM4D_PNGDEC_ST_DISTANCE;
        break;
      }
      if (mlen > im.expect - wr.pos) {
        st |= DM4D_PNGDEC_ST_END;
        break;
      }
      __syncthreads();  // the bytes before pos are final and visible
      const uint32_t from = wr.pos - d;
      // 64 bytes a step; every source lies before pos (i mod d < d), so no step reads what this match stores
      if (d >= mlen) {
        for (uint32_t i = lane; i < mlen; i += 64u) s.ring[(wr.pos + i) & kRingMask] = s.ring[(from + i) & kRingMask];
      } else {
        for (uint32_t i = lane; i < mlen; i += 64u) s.ring[(wr.pos + i) & kRingMask] = s.ring[(from + i % d) & kRingMask];
      }
      wr.produced(mlen);
    }
  }
  if (!st) {
    wr.finish();
    if (wr.pos != im.expect) st |= DM4D_PNGDEC_ST_END;
  }
  if (!st) {
    br.drop(br.have & 7);
    br.refill();
    const uint32_t lo = br.take(16), hi = br.take(16);  // four bytes, the most significant first
    const uint32_t want = __builtin_bswap32(lo | (hi << 16));
    if (br.over()) st |= DM4D_PNGDEC_ST_END;
    else if (want != ((wr.s2 << 16) | wr.s1)) st |= DM4D_PNGDEC_ST_ADLER;
  }
  if (lane == 0) status[blockIdx.x] = st;
}

// -- unfilter ----------------------------------------------------------------------------------------------------------------------------
// A row's filtered bytes in order, from aligned words of the workspace; one word is in flight ahead of the one in use.
struct RowReader {
  const uint32_t* words;  // the image's filtered stream (16-byte aligned)
  uint32_t nwords, next;
  uint64_t win;
  int have;
  uint32_t ahead;

  __device__ __forceinline__ uint32_t word(uint32_t i) const { return i < nwords ? words[i] : 0u; }
  __device__ __forceinline__ void start(uint32_t byte) {
    next = byte >> 2;
    win = (uint64_t)(word(next) >> (8u * (byte & 3u)));
    have = 4 - (int)(byte & 3u);
    ahead = word(next + 1u);
    next += 2u;
  }
  __device__ __forceinline__ uint32_t take(int nb) {
    if (have < nb) {
      win |= (uint64_t)ahead << (8 * have);
      have += 4;
      ahead = word(next);
      next += 1u;
    }
    const uint32_t v = (uint32_t)win & (nb == 4 ? 0xffffffffu : (1u << (8 * nb)) - 1u);
    win >>= 8 * nb, have -= nb;
    return v;
  }
};

template <int BPP>
__device__ bool unfilter_image(const Image& im, const uint8_t* __restrict__ src, uint8_t* __restrict__ out, uint8_t* above) {
  const int lane = threadIdx.x;
  const uint32_t rb = (uint32_t)im.w * BPP, stride = rb + 1u;
  for (uint32_t i = lane; i < rb; i += 64u) above[i] = 0;  // the row above the first row
  __syncthreads();
  RowReader rd;
  rd.words = reinterpret_cast<const uint32_t*>(src), rd.nwords = (im.expect + 3u) >> 2;
  bool bad = false;
  for (int row0 = 0; row0 < im.h; row0 += 64) {
    const int row = row0 + lane;
    const bool live = row < im.h;
    uint32_t ft = 0;
    if (live) {
      rd.start((uint32_t)row * stride);
      ft = rd.take(1);
      bad |= ft > 4u;
    }
    uint32_t left = 0, corner = 0, mine = 0;  // packed pixels: left, above-left, and the one this lane decoded last
    uint8_t* dst = out + (uint64_t)(live ? row : 0) * rb;
    for (int t = 0; t < im.w + 63; ++t) {
      const int x = t - lane;
      uint32_t up = __shfl_up(mine, 1);
      if (lane == 0) {
        up = 0;
        if (x < im.w)
#pragma unroll
          for (int c = 0; c < BPP; ++c) up |= (uint32_t)above[x * BPP + c] << (8 * c);
      }
      if (live && x >= 0 && x < im.w) {
        const uint32_t raw = rd.take(BPP);
        uint32_t px = 0;
#pragma unroll
        for (int c = 0; c < BPP; ++c) {
          const int a = (int)((left >> (8 * c)) & 255u), b = (int)((up >> (8 * c)) & 255u), cc = (int)((corner >> (8 * c)) & 255u);
          const int pa = abs(b - cc), pb = abs(a - cc), pc = abs(a + b - 2 * cc);
          const int paeth = (pa <= pb && pa <= pc) ? a : pb <= pc ? b : cc;
          const int pred = ft == 1u ? a : ft == 2u ? b : ft == 3u ? (a + b) >> 1 : ft == 4u ? paeth : 0;
          const uint32_t v = (((raw >> (8 * c)) & 255u) + (uint32_t)pred) & 255u;
          px |= v << (8 * c);
          dst[(uint32_t)x * BPP + c] = (uint8_t)v;
          if (lane == 63) above[x * BPP + c] = (uint8_t)v;
        }
        corner = up, left = px, mine = px;
      }
    }
    __syncthreads();
  }
  return bad;
}

__global__ void __launch_bounds__(64) pngdec_unfilter_kernel(const int64_t* __restrict__ desc, const uint8_t* __restrict__ workspace,
                                                             uint8_t* __restrict__ out_all, int32_t* __restrict__ status) {
  __shared__ uint8_t above[DM4D_PNGDEC_MAX_ROW_BYTES];
  const Image im = image_of(desc, blockIdx.x);
  if (status[blockIdx.x] != 0) return;  // written by the launch before this one; the filtered stream is incomplete
  const uint8_t* src = workspace + im.ws;
  uint8_t* out = out_all + im.out;
  bool bad;
  if (im.bpp == 1) bad = unfilter_image<1>(im, src, out, above);
  else if (im.bpp == 3) bad = unfilter_image<3>(im, src, out, above);
  else bad = unfilter_image<4>(im, src, out, above);
  if (__ballot(bad) != 0ull && threadIdx.x == 0) status[blockIdx.x] = DM4D_PNGDEC_ST_FILTER;
}

}  // namespace

extern "C" size_t dm4d_png_decode_ws_bytes(int64_t total_filtered_bytes, int n) {
  if (total_filtered_bytes <= 0 || total_filtered_bytes > kMaxWorkspace || n <= 0 || n > 65535) return 0;
  return (size_t)pad16(total_filtered_bytes);
}

extern "C" int dm4d_png_decode_u8(void* stream, const void* streams, int64_t streams_bytes, const int64_t* desc_host, const int64_t* desc_dev,
                                  int n, void* workspace, int64_t workspace_bytes, void* out, int64_t out_bytes, int32_t* status) {
  if (!streams || !desc_host || !desc_dev || !workspace || !out || !status) return dm4d_set_error(DM4D_ERR_ARG, "png_decode: null pointer");
  if (n <= 0 || n > 65535 || streams_bytes <= 0 || out_bytes <= 0) return dm4d_set_error(DM4D_ERR_ARG, "png_decode: empty or oversized batch");
  if (((uintptr_t)workspace & 15) || ((uintptr_t)streams & 3) || ((uintptr_t)status & 3))
    return dm4d_set_error(DM4D_ERR_ARG, "png_decode: workspace must be 16-byte aligned, streams and status 4-byte");
  int64_t ws0 = 0;
  for (int i = 0; i < n; ++i) {
    const int64_t* d = desc_host + (int64_t)i * DM4D_PNGDEC_FIELDS;
    const int64_t h = d[D_H], w = d[D_W], ch = d[D_CHANNELS];
    if (!(ch == 1 || ch == 3 || ch == 4)) return dm4d_set_error(DM4D_ERR_ARG, "png_decode: a descriptor's channels are not 1, 3 or 4");
    if (d[D_OUT_CHANNELS] != ch) return dm4d_set_error(DM4D_ERR_ARG, "png_decode: output channels must equal the file's channels");
    if (h < 1 || w < 1 || w * ch > DM4D_PNGDEC_MAX_ROW_BYTES || h > 0x7fffffffll || h * (1 + w * ch) > 0x7fffffffll)
      return dm4d_set_error(DM4D_ERR_ARG, "png_decode: a dimension below 1, a row above DM4D_PNGDEC_MAX_ROW_BYTES or an image of 2^31 bytes");
    if (d[D_BYTES] < 2 || d[D_BYTES] >= DM4D_PNGDEC_MAX_STREAM_BYTES || d[D_STREAM] < 0 || (d[D_STREAM] & 3) || d[D_STREAM] > streams_bytes ||
        (d[D_BYTES] + 3) / 4 * 4 > streams_bytes - d[D_STREAM])
      return dm4d_set_error(DM4D_ERR_ARG, "png_decode: a stream is too short, too long, misaligned or outside the stream buffer (padding included)");
    if (d[D_OUT] < 0 || d[D_OUT] > out_bytes || h * w * ch > out_bytes - d[D_OUT])
      return dm4d_set_error(DM4D_ERR_ARG, "png_decode: an image lies outside the output buffer");
    if (d[D_WS] != ws0) return dm4d_set_error(DM4D_ERR_ARG, "png_decode: a descriptor's workspace offset is not the running sum");
    ws0 += pad16(h * (1 + w * ch));
    if (ws0 > kMaxWorkspace) return dm4d_set_error(DM4D_ERR_ARG, "png_decode: too many bytes in one batch");
  }
  if (workspace_bytes < ws0) return dm4d_set_error(DM4D_ERR_ARG, "png_decode: workspace too small (dm4d_png_decode_ws_bytes)");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(pngdec_inflate_kernel, dim3((unsigned)n), dim3(64), 0, st, desc_dev, (const uint8_t*)streams, (uint8_t*)workspace, status);
  int rc = dm4d_check_launch("pngdec_inflate_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(pngdec_unfilter_kernel, dim3((unsigned)n), dim3(64), 0, st, desc_dev, (const uint8_t*)workspace, (uint8_t*)out, status);
  return dm4d_check_launch("pngdec_unfilter_kernel");
}
