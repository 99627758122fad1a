// Lossless 8-bit RGB PNG encoder on the device (include/upr.h upr_png_encode).
//
// File: signature, IHDR, one IDAT per strip of rows_per_strip rows, one trailing
// IDAT with the Adler-32, IEND.  A strip is one deflate block of dynamic Huffman
// codes over literals and end-of-block (no LZ77 matches), followed by an empty
// stored block, so every strip starts on a byte boundary and one workgroup
// writes it without knowing the others; a strip whose Huffman form would be no
// smaller is written as stored blocks.  Filters see raw pixels only, so the
// row above a strip's first row is simply the image row above it.
//
//   png_strip_kernel   one workgroup per (strip, image): row filters, histogram,
//                      Adler partial sums, code lengths (<= 15 bits), the bit
//                      stream into the strip's scratch slot, the chunk's CRC-32
//   png_layout_kernel  one workgroup per image: scan of the chunk sizes, the
//                      Adler-32 of the image, signature / IHDR / trailer / IEND
//   png_gather_kernel  one workgroup per (strip, image): chunk -> its place in the file
//
// With match = UPR_PNG_MATCH_LZ (upr_png_encode_ex) the strip kernel also stages the strip's
// filtered bytes in scratch (and in LDS when they fit), finds LZ77 matches inside the strip
// (64 positions per step, four candidates per position: distance 1 / 3, the byte above, the earliest equal hash of the step,
// the most recent equal hash before it), resolves the greedy parse with per-run exit tables
// instead of one serial walk, builds the literal/length and distance codes and writes the
// matched block when it is smaller than both the literal-only block and the stored form.
//
// Every byte is written with ordinary vector stores; nothing is computed on the host.
#include "upr_common.h"

namespace upr {

namespace {

constexpr int kThreads = 256;
constexpr int kRun = 16;                   // consecutive symbols one thread packs per chunk
constexpr int kChunk = kThreads * kRun;    // symbols per chunk
constexpr int kStageWords = 2048;          // >= (kChunk * 15 + 3 + 31) / 32 + 2; match mode: see emit_chunk
constexpr int kLit = 257;                  // literals + end-of-block
constexpr int kCl = 19;                    // code-length alphabet
constexpr int kSymPad = 288;
constexpr unsigned kAdlerMod = 65521u;
constexpr unsigned kCrcPoly = 0xEDB88320u;
constexpr int kFilterAdaptive = 5;
constexpr int kHeadBytes = 33;             // signature + IHDR chunk
constexpr int kTailBytes = 16 + 12;        // Adler IDAT + IEND
// rows_per_strip * (3W + 1) limit: histogram counts, bit offsets (15 bits per
// symbol) and the 64-bit Adler partial sums all stay in range below it
constexpr long long kMaxStripBytes = 1LL << 24;
// match mode LZ
constexpr int kMatchLz = 1;
constexpr int kLl = 286;                   // literal/length alphabet
constexpr int kDist = 30;                  // distance alphabet
constexpr int kMinMatch = 3, kMaxMatch = 258;
constexpr unsigned kMaxDist = 32768;
constexpr unsigned kFar3 = 4096;           // a match of 3 bytes further back costs more than 3 literals
constexpr int kHashBits = 12;
constexpr int kHashSize = 1 << kHashBits;
constexpr int kStep = kThreads / 4;        // positions matched per step, 4 threads each
constexpr int kStepTab = 256;              // hash slots of the earliest-in-step table
constexpr int kSuper = kRun * kRun;        // positions per super-run of the parse
constexpr unsigned kTaken = 0x8000u;       // match word: length | kTaken | distance << 16
constexpr int kFbSlack = 48;               // bytes readable behind a strip's staged bytes
// dynamic LDS for a strip's bytes at the most: with the static 40 KB a workgroup stays within
// 64 KB, two or more to a compute unit; 16 rows of 512 pixels (24592 + 48 bytes) still fit
constexpr unsigned kLzLdsMax = 24640;
static_assert(kStep == 64, "the step table packs the position in 6 bits");
static_assert(kChunk == kRun * kSuper && kChunk + kMaxMatch < 0xFFFF, "parse tables are u16 over three levels of kRun");
static_assert(kStepTab + (kRun + kThreads) / 2 <= kStageWords, "the step table and the entry lists live in the stage");

struct PngGeom {
  int H, W, rps, ns;        // ns strips of rps rows (the last may be shorter)
  int rowb;                 // filtered bytes per row, 3W + 1
  size_t cap;               // bytes of one strip's scratch slot
  size_t file_bound;        // bytes of one image's file, at most
  size_t scratch_image;     // scratch bytes of one image
  size_t off_sizes, off_adler, off_offs, off_ftype;  // arrays behind the ns slots
  // match mode LZ: per strip lz_stride bytes at off_lz, the filtered bytes (+ kFbSlack) and
  // from lz_md one match word per filtered byte
  size_t off_lz, lz_md, lz_stride;
};

inline size_t stored_bytes(size_t n) { return n + 5 * ((n + 65534) / 65535) + 5; }

// kOk and the geometry, or the status of a shape the encoder does not take
int png_geom(int H, int W, int rps, int match, PngGeom* g) {
  if (H <= 0 || W <= 0 || rps <= 0) return kErrArg;
  if (rps > H) rps = H;
  const long long rowb = 3LL * W + 1;
  if (rowb * rps > kMaxStripBytes) return kErrShape;
  const long long ns = ((long long)H + rps - 1) / rps;
  const long long last = H - (ns - 1) * rps;
  // per strip: the chunk's 12 bytes and the stored form, rounded up to n + 32 for a strip of one
  // stored block; 128 covers the fixed parts (63 bytes)
  const long long bound = 128 + (ns - 1) * (22 + (long long)stored_bytes(rowb * rps)) +
                          (22 + (long long)stored_bytes(rowb * last));
  if (bound > (1LL << 31)) return kErrShape;
  g->H = H; g->W = W; g->rps = rps; g->ns = (int)ns; g->rowb = (int)rowb;
  // chunk length + type, zlib header, data, CRC; the bit stream is flushed in whole words
  g->cap = align_up(8 + 2 + stored_bytes((size_t)(rowb * rps)) + 4 + 8, 16);
  g->file_bound = (size_t)bound;
  g->off_sizes = (size_t)ns * g->cap;
  g->off_adler = g->off_sizes + align_up((size_t)ns * 4, 16);
  g->off_offs = g->off_adler + align_up((size_t)ns * 8, 16);
  g->off_ftype = g->off_offs + align_up((size_t)ns * 4, 16);
  g->scratch_image = g->off_ftype + align_up((size_t)H, 16);
  g->off_lz = g->scratch_image;
  g->lz_md = align_up((size_t)(rowb * rps) + kFbSlack, 16);
  g->lz_stride = g->lz_md + align_up(4 * (size_t)(rowb * rps), 16);
  if (match == kMatchLz) g->scratch_image += (size_t)ns * g->lz_stride;
  return kOk;
}

struct PngArgs {
  const uint8_t* img;       // [B][H][W][3]
  uint8_t* scratch;
  uint8_t* out;
  long long* sizes;
  size_t out_stride;
  PngGeom g;
  int filter;
  unsigned lds_bytes;       // dynamic LDS of the strip kernel's launch
};

// RFC 1951 3.2.5: code and number of extra bits of a match length 3 .. 258 / distance 1 .. 32768;
// the extra bits' value is the low `eb` bits of len - 3 / dist - 1
__host__ __device__ __forceinline__ unsigned len_code(unsigned len, unsigned* eb) {
  const unsigned l = len - 3;
  if (len == 258 || l < 8) { *eb = 0; return len == 258 ? 285u : 257u + l; }
  const unsigned k = 31u - (unsigned)__builtin_clz(l);
  *eb = k - 2;
  return 261u + 4u * (k - 2) + ((l >> (k - 2)) & 3u);
}
__host__ __device__ __forceinline__ unsigned dist_code(unsigned dist, unsigned* eb) {
  const unsigned x = dist - 1;
  if (x < 4) { *eb = 0; return x; }
  const unsigned k = 31u - (unsigned)__builtin_clz(x);
  *eb = k - 1;
  return 2u * k + ((x >> (k - 1)) & 1u);
}

// ---- small workgroup helpers (kThreads = 4 waves of 64) -----------------------------------------
__device__ __forceinline__ unsigned wave_incl_scan(unsigned v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  return v;
}

// exclusive scan of one value per thread; *total = the workgroup's sum.  red: 8 words of LDS.
__device__ __forceinline__ unsigned block_excl_scan(unsigned v, unsigned* red, unsigned* total) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const unsigned inc = wave_incl_scan(v, lane);
  __syncthreads();
  if (lane == 63) red[w] = inc;
  __syncthreads();
  unsigned base = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < kThreads / 64; ++k) {
    const unsigned s = red[k];
    if (k < w) base += s;
    tot += s;
  }
  *total = tot;
  return base + inc - v;
}

__device__ __forceinline__ unsigned long long block_sum_u64(unsigned long long v, unsigned long long* red) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

__device__ __forceinline__ unsigned block_xor_u32(unsigned v, unsigned* red) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v ^= __shfl_xor(v, d, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] ^ red[1] ^ red[2] ^ red[3];
}

// ---- filters ------------------------------------------------------------------------------------
__device__ __forceinline__ int paeth_pred(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// filtered byte of raw byte `col` (0 .. 3W-1) of image row r under filter ft; row: the image's
// row r, up: row r - 1 or nullptr above the image
__device__ __forceinline__ unsigned filt_byte(const uint8_t* row, const uint8_t* up, int col, int ft) {
  const int x = row[col];
  if (ft == 0) return (unsigned)x;
  const int a = (ft != 2 && col >= 3) ? row[col - 3] : 0;
  const int b = (ft != 1 && up) ? up[col] : 0;
  int pred;
  if (ft == 1) pred = a;
  else if (ft == 2) pred = b;
  else if (ft == 3) pred = (a + b) >> 1;
  else {
    const int c = (up && col >= 3) ? up[col - 3] : 0;
    pred = paeth_pred(a, b, c);
  }
  return (unsigned)(x - pred) & 255u;
}

__device__ __forceinline__ unsigned msad(unsigned v) { return v < 128u ? v : 256u - v; }

// ---- CRC-32 -------------------------------------------------------------------------------------
// polynomials mod the CRC polynomial in the reflected form: bit 31 is x^0
__device__ unsigned gf_mul(unsigned a, unsigned b) {
  unsigned p = 0;
  for (unsigned m = 0x80000000u; m && a; m >>= 1) {
    if (a & m) { p ^= b; a &= ~m; }
    b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
  }
  return p;
}
// x^(8 * 2^k) mod the CRC polynomial, k = 0 .. 27: constants of the polynomial, like the byte table
__device__ __constant__ const unsigned kX8Pow2[28] = {
    0x00800000u, 0x00008000u, 0xedb88320u, 0xb1e6b092u, 0xa06a2517u, 0xed627daeu, 0x88d14467u,
    0xd7bbfe6au, 0xec447f11u, 0x8e7ea170u, 0x6427800eu, 0x4d47bae0u, 0x09fe548fu, 0x83852d0fu,
    0x30362f1au, 0x7b5a9cc3u, 0x31fec169u, 0x9fec022au, 0x6c8dedc4u, 0x15d6874du, 0x5fde7a4eu,
    0xbad90e37u, 0x2e4e5eefu, 0x4eaba214u, 0xa8a472c0u, 0x429a969eu, 0x148d302au, 0xc40ba6d0u};
// x^(8 n), n < 2^28
__device__ unsigned gf_x8n(unsigned n) {
  unsigned p = 0x80000000u;  // 1
  for (int k = 0; n; n >>= 1, ++k)
    if (n & 1u) p = gf_mul(kX8Pow2[k], p);
  return p;
}
__device__ __forceinline__ unsigned crc_bitwise(unsigned crc, unsigned byte) {
  crc ^= byte;
#pragma unroll
  for (int k = 0; k < 8; ++k) crc = (crc & 1u) ? (crc >> 1) ^ kCrcPoly : crc >> 1;
  return crc;
}
__device__ __forceinline__ void put_be32(uint8_t* p, unsigned v) {
  p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v;
}

// ---- Huffman code lengths -----------------------------------------------------------------------
struct HuffWork {
  unsigned cnt[kSymPad];     // working counts (halved until the code fits)
  unsigned sw[kSymPad];      // counts of the used symbols, ascending (ties: lower symbol first)
  unsigned ss[kSymPad];      // their symbols
  unsigned nw[kSymPad];      // weights of the internal nodes, in creation order
  int parent[2 * kSymPad];   // leaves 0 .. m-1 in sorted order, then the internal nodes
  unsigned blc[16], next[16];
  unsigned m, maxd;
};

// lens[s] = code length of symbol s (0: unused) of a Huffman code over cnt[0 .. n) no deeper than
// `limit`: the plain Huffman code if it fits, else the code of the counts halved (non-zero counts
// kept >= 1) as often as needed.  Deterministic: the sort key is (count, symbol), the two-queue
// merge prefers a leaf on a tie.  All threads call it; at least one count is non-zero.  A single
// used symbol gets length 1 (the m == 1 branch): match mode relies on that for a strip whose
// matches share one distance code; the literal alphabets always hold two symbols or more.
__device__ void huff_lengths(const unsigned* cnt, int n, int limit, unsigned* lens, HuffWork& w) {
  const int tid = threadIdx.x;
  for (int s = tid; s < n; s += kThreads) { w.cnt[s] = cnt[s]; lens[s] = 0; }
  for (;;) {
    if (tid == 0) { w.m = 0; w.maxd = 0; }
    __syncthreads();
    for (int s = tid; s < n; s += kThreads) {
      const unsigned c = w.cnt[s];
      if (!c) continue;
      int rank = 0;
      for (int j = 0; j < n; ++j) {
        const unsigned cj = w.cnt[j];
        rank += (cj && (cj < c || (cj == c && j < s))) ? 1 : 0;
      }
      w.sw[rank] = c;
      w.ss[rank] = (unsigned)s;
      atomicAdd(&w.m, 1u);
    }
    __syncthreads();
    const int m = (int)w.m;
    if (tid == 0) {
      if (m == 1) {
        w.parent[0] = -1;
      } else {
        int li = 0, ni = 0, nn = 0;
        for (int t = 0; t < m - 1; ++t) {
          int id[2];
          unsigned sum = 0;
#pragma unroll
          for (int k = 0; k < 2; ++k) {
            if (li < m && (ni >= nn || w.sw[li] <= w.nw[ni])) { sum += w.sw[li]; id[k] = li++; }
            else { sum += w.nw[ni]; id[k] = m + ni++; }
          }
          w.nw[nn] = sum;
          w.parent[id[0]] = m + nn;
          w.parent[id[1]] = m + nn;
          ++nn;
        }
        w.parent[2 * m - 2] = -1;
      }
    }
    __syncthreads();
    for (int k = tid; k < m; k += kThreads) {
      unsigned d = 0;
      for (int p = w.parent[k]; p >= 0; p = w.parent[p]) ++d;
      if (d == 0) d = 1;
      lens[w.ss[k]] = d;
      atomicMax(&w.maxd, d);
    }
    __syncthreads();
    if ((int)w.maxd <= limit) break;
    for (int s = tid; s < n; s += kThreads) w.cnt[s] = (w.cnt[s] + 1) >> 1;
    __syncthreads();
  }
}

// canonical codes (RFC 1951 3.2.2) of lens[0 .. n), each bit-reversed for LSB-first packing:
// codes[s] = reversed code | length << 24
__device__ void huff_codes(const unsigned* lens, int n, unsigned* codes, HuffWork& w) {
  const int tid = threadIdx.x;
  if (tid < 16) w.blc[tid] = 0;
  __syncthreads();
  for (int s = tid; s < n; s += kThreads)
    if (lens[s]) atomicAdd(&w.blc[lens[s]], 1u);
  __syncthreads();
  if (tid == 0) {
    unsigned code = 0;
    w.next[0] = 0;
    for (int b = 1; b < 16; ++b) {
      code = (code + (b > 1 ? w.blc[b - 1] : 0u)) << 1;
      w.next[b] = code;
    }
  }
  __syncthreads();
  for (int s = tid; s < n; s += kThreads) {
    const unsigned l = lens[s];
    unsigned c = 0;
    if (l) {
      unsigned idx = 0;
      for (int j = 0; j < s; ++j) idx += lens[j] == l ? 1u : 0u;
      c = (__brev(w.next[l] + idx) >> (32 - l)) | (l << 24);
    }
    codes[s] = c;
  }
  __syncthreads();
}

__device__ __constant__ const uint8_t kClOrder[kCl] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

struct StripLds {
  unsigned hist[kSymPad];
  unsigned lens[kSymPad];
  unsigned codes[kSymPad];
  unsigned clhist[32], cllens[32], clcodes[32];
  unsigned stage[kStageWords];
  unsigned crctab[256];
  unsigned long long red64[4];
  unsigned red[8];
  HuffWork hw;
};

// ---- match mode LZ ------------------------------------------------------------------------------
struct LzLds {
  unsigned hist[kSymPad], lens[kSymPad], codes[kSymPad];  // literal/length alphabet of the parse
  unsigned dhist[32], dlens[32], dcodes[32];              // distance alphabet
  unsigned clhist[32], cllens[32], clcodes[32];
  union {
    unsigned recent[kHashSize];  // matching: hash -> 1 + the most recent position before the step
    struct {
      unsigned short e1[kChunk];  // parse: where the greedy walk from a position leaves its run ...
      unsigned short e2[kChunk];  // ... and its super-run (chunk-local positions)
    } p;
  } u;
  unsigned exitp, nl, nd;
};
struct LzNone {};
// what kLzLdsMax promises: static and dynamic LDS of the match-mode kernel within 64 KiB
static_assert(sizeof(StripLds) + sizeof(LzLds) + kLzLdsMax <= 64 * 1024, "LDS of the match-mode strip kernel");

// bytes i .. i + 7 of the staged bytes (fbw: their 8-byte words) from two aligned words; reads up
// to 15 bytes behind i
__device__ __forceinline__ unsigned long long load8(const unsigned long long* fbw, unsigned i) {
  const unsigned long long lo = fbw[i >> 3], hi = fbw[(i >> 3) + 1];
  const unsigned sh = (i & 7u) * 8u;
  return (lo >> sh) | ((hi << 1) << (63u - sh));
}

// common prefix of the bytes at i and at p, at most maxlen (0: none); x0 = load8(fbw, i).  The
// first 8 bytes decide most candidates; behind them 32 bytes per round, so that one LDS round
// trip covers them.  Reads up to 39 bytes behind i + maxlen - 1.
__device__ __forceinline__ unsigned match_len(const unsigned long long* fbw, unsigned i, unsigned p, unsigned maxlen,
                                              unsigned long long x0) {
  if (!maxlen) return 0;
  x0 ^= load8(fbw, p);
  if (x0) return min((unsigned)(__ffsll((long long)x0) - 1) >> 3, maxlen);
  unsigned l = 8;
  while (l < maxlen) {
    const unsigned ia = i + l, ip = p + l;
    const unsigned long long* wa = fbw + (ia >> 3);
    const unsigned long long* wp = fbw + (ip >> 3);
    const unsigned sa = (ia & 7u) * 8u, sp = (ip & 7u) * 8u;
    unsigned long long a[5], q[5], x[4];
#pragma unroll
    for (int k = 0; k < 5; ++k) { a[k] = wa[k]; q[k] = wp[k]; }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      x[k] = ((a[k] >> sa) | ((a[k + 1] << 1) << (63u - sa))) ^ ((q[k] >> sp) | ((q[k + 1] << 1) << (63u - sp)));
    if (x[0] | x[1] | x[2] | x[3]) {
      const int k = x[0] ? 0 : (x[1] ? 1 : (x[2] ? 2 : 3));
      const unsigned long long xk = x[0] ? x[0] : (x[1] ? x[1] : (x[2] ? x[2] : x[3]));
      l += 8u * (unsigned)k + ((unsigned)(__ffsll((long long)xk) - 1) >> 3);
      break;
    }
    l += 32;
  }
  return min(l, maxlen);
}

// kRun entries per thread, bits | count << 56 (count <= 48), appended to the strip's bit stream
// through the stage as the literal-only form does; all threads call it.  What a call may bring:
// the header chunk at most 16 + 17 + 3 kCl + 7 (kLl + kDist) bits; a chunk of kChunk positions at
// most 15 bits per position that its entries cover plus one entry of 48 bits, because a literal
// is at most 15 bits and a match of length L at most 15 L (3 <= L <= 10: no length extra bits,
// 15 + 15 + 13; a match of 3 reaches kFar3 back at the most, 10 distance extra bits; L >= 11:
// 48 <= 15 L), and only the chunk's last match covers positions behind the chunk.
static_assert(31 + kChunk * 15 + 48 <= (kStageWords - 2) * 32, "a chunk of matched entries fits the stage");
static_assert(31 + 16 + 17 + 3 * kCl + 7 * (kLl + kDist) <= (kStageWords - 2) * 32, "the header fits the stage");
__device__ __forceinline__ void emit_chunk(const unsigned long long (&sym)[kRun], StripLds& L, unsigned* dataw,
                                           unsigned& carry, unsigned& outw) {
  const int tid = threadIdx.x;
  unsigned nbits = 0;
#pragma unroll
  for (int k = 0; k < kRun; ++k) nbits += (unsigned)(sym[k] >> 56);
  unsigned total;
  const unsigned pos = carry + block_excl_scan(nbits, L.red, &total);
  unsigned wi = pos >> 5, nb = pos & 31u;
  unsigned long long acc = 0;
#pragma unroll
  for (int k = 0; k < kRun; ++k) {
    const unsigned c = (unsigned)(sym[k] >> 56), c1 = min(c, 24u);
    // two parts of at most 24 bits, so the accumulator never holds more than 31 + 24 bits
    acc |= (sym[k] & 0xffffffull) << nb;
    nb += c1;
    if (nb >= 32) { atomicOr(&L.stage[wi], (unsigned)acc); ++wi; acc >>= 32; nb -= 32; }
    acc |= ((sym[k] >> 24) & 0xffffffull) << nb;
    nb += c - c1;
    if (nb >= 32) { atomicOr(&L.stage[wi], (unsigned)acc); ++wi; acc >>= 32; nb -= 32; }
  }
  if (nb) atomicOr(&L.stage[wi], (unsigned)acc);
  __syncthreads();
  const unsigned T = carry + total;
  const unsigned full = T >> 5;
  for (unsigned k = tid; k < full; k += kThreads) dataw[outw + k] = L.stage[k];
  const unsigned cw = L.stage[full];
  __syncthreads();
  for (unsigned k = tid; k <= full; k += kThreads) L.stage[k] = 0;
  __syncthreads();
  if (tid == 0) L.stage[0] = cw;
  __syncthreads();
  outw += full;
  carry = T & 31u;
}

// Workgroup barrier that orders LDS accesses only: stores to global memory stay in flight.  The
// matcher's steps exchange data through LDS alone; what they store to scratch is read after a
// __syncthreads().
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Matches of the strip's staged bytes (fbw: their 8-byte words, in LDS when the strip fits the
// launch's dynamic LDS, else in scratch; kFbSlack readable bytes behind them): md[i] = length |
// distance << 16 of the match taken at i if the parse reaches i, 0 for a literal.  kStep
// positions per step, four threads
// each: distances 1 and 3, distance rowb, the earliest position of this step with the same
// 3-byte hash (tab, tagged with the step), the most recent one before the step (recent, filled
// by atomicMax after the step's lookups).  Longest wins, then the nearest: no dependence on timing.
__device__ __forceinline__ void lz_match(const unsigned long long* fbw, unsigned* md, unsigned n, unsigned rowb,
                                         LzLds& Z, unsigned* tab) {
  const int tid = threadIdx.x;
  const unsigned q = (unsigned)tid >> 2, role = (unsigned)tid & 3u;
  for (int k = tid; k < kHashSize; k += kThreads) Z.u.recent[k] = 0;
  bool pend = false;
  unsigned pend_h = 0, pend_i = 0;
  __syncthreads();
  for (unsigned base = 0, step = 1; base < n; base += kStep, ++step) {
    const unsigned i = base + q;
    const bool ok = i + kMinMatch <= n;
    const unsigned long long x0 = i < n ? load8(fbw, i) : 0ull;
    const unsigned h = (((unsigned)x0 & 0xffffffu) * 0x9E3779B1u) >> (32 - kHashBits);
    if (role == 0) {
      if (pend) atomicMax(&Z.u.recent[pend_h], pend_i + 1);
      if (ok) atomicMax(&tab[h & (kStepTab - 1)], step << 6 | (unsigned)(kStep - 1 - q));
    }
    lds_barrier();
    unsigned key = 0;  // length << 16 | 65536 - distance
    {
      // one instruction stream for the four roles: both tables are read by every thread, the
      // role only selects the distance (0: no candidate); role 0 has a second one
      const unsigned maxlen = ok ? min((unsigned)kMaxMatch, n - i) : 0u;
      const unsigned vt = tab[h & (kStepTab - 1)], vr = Z.u.recent[h];
      const unsigned pt = base + (unsigned)(kStep - 1) - (vt & 63u);
      const unsigned dt = ((vt >> 6) == step && pt < i) ? i - pt : 0u;
      const unsigned dr = (vr && i - (vr - 1) <= kMaxDist) ? i - (vr - 1) : 0u;
      const unsigned dup = (rowb <= kMaxDist && i >= rowb) ? rowb : 0u;
      const unsigned d0 = role == 0 ? (i >= 1 ? 1u : 0u) : (role == 1 ? dup : (role == 2 ? dt : dr));
      const unsigned d1 = (role == 0 && i >= 3) ? 3u : 0u;
      const unsigned l0 = match_len(fbw, i, i - d0, d0 ? maxlen : 0u, x0);
      if (l0 >= kMinMatch) key = l0 << 16 | (65536u - d0);
      const unsigned l1 = match_len(fbw, i, i - d1, d1 ? maxlen : 0u, x0);
      if (l1 >= kMinMatch) key = max(key, l1 << 16 | (65536u - d1));
    }
    key = max(key, (unsigned)__shfl_xor((int)key, 1, 64));
    key = max(key, (unsigned)__shfl_xor((int)key, 2, 64));
    if (role == 0 && i < n) {
      const unsigned len = key >> 16, dist = 65536u - (key & 0xffffu);
      md[i] = (len < kMinMatch || (len == kMinMatch && dist > kFar3)) ? 0u : (len | dist << 16);
    }
    pend = ok; pend_h = h; pend_i = i;
    lds_barrier();
  }
  __syncthreads();
}

// The greedy parse of md[0 .. n) ("after a match of length L at i go on at i + L") without a
// serial walk: per chunk of kChunk positions, e1 = where the walk from each position leaves
// its thread's run of kRun (kRun backward steps in the thread), e2 = where it leaves its
// super-run of kRun runs (kRun steps over e1); one thread then visits the chunk's super-runs,
// kRun threads the runs of theirs, every thread the positions of its run.  The positions on
// the walk get kTaken, their symbols go into Z.hist / Z.dhist.  Returns this thread's share of
// (extra bits, matches).  ent2 / ent1: kRun / kThreads u16 entry lists.
__device__ void lz_parse(const uint8_t* fb, unsigned* md, unsigned n, LzLds& Z, unsigned short* ent2,
                         unsigned short* ent1, unsigned long long* extra_bits, unsigned long long* matches) {
  const int tid = threadIdx.x;
  unsigned long long extra = 0, nm = 0;
  unsigned ent = 0;  // first position of the walk at or behind the chunk's base
  for (unsigned cb = 0; cb < n; cb += kChunk) {
    const unsigned nloc = min((unsigned)kChunk, n - cb);
    const unsigned run_end = (unsigned)(tid + 1) * kRun;
    for (int k = kRun - 1; k >= 0; --k) {
      const unsigned loc = (unsigned)tid * kRun + (unsigned)k;
      const unsigned len = loc < nloc ? (md[cb + loc] & 0xffffu) : 0u;
      const unsigned nx = loc + max(1u, len);
      Z.u.p.e1[loc] = (unsigned short)(nx >= run_end ? nx : Z.u.p.e1[nx]);
    }
    ent1[tid] = 0xFFFF;
    if (tid < kRun) ent2[tid] = 0xFFFF;
    __syncthreads();
    {
      const unsigned sbase = ((unsigned)tid / kRun) * kSuper, j = (unsigned)tid % kRun, send = sbase + kSuper;
      for (int r = kRun - 1; r >= 0; --r) {
        const unsigned loc = sbase + (unsigned)r * kRun + j;
        const unsigned x = Z.u.p.e1[loc];
        Z.u.p.e2[loc] = (unsigned short)(x >= send ? x : Z.u.p.e2[x]);
        __syncthreads();
      }
    }
    if (tid == 0) {
      unsigned p = ent - cb;
      while (p < nloc) { ent2[p / kSuper] = (unsigned short)p; p = Z.u.p.e2[p]; }
      Z.exitp = p;
    }
    __syncthreads();
    if (tid < kRun) {
      unsigned p = ent2[tid];
      const unsigned send = (unsigned)(tid + 1) * kSuper;
      if (p != 0xFFFF)
        while (p < send && p < nloc) { ent1[p / kRun] = (unsigned short)p; p = Z.u.p.e1[p]; }
    }
    __syncthreads();
    {
      unsigned p = ent1[tid];
      if (p != 0xFFFF)
        while (p < run_end && p < nloc) {
          const unsigned m = md[cb + p], len = m & 0xffffu;
          if (len) {
            unsigned le, de;
            atomicAdd(&Z.hist[len_code(len, &le)], 1u);
            atomicAdd(&Z.dhist[dist_code(m >> 16, &de)], 1u);
            extra += le + de;
            ++nm;
          } else {
            atomicAdd(&Z.hist[fb[cb + p]], 1u);
          }
          md[cb + p] = m | kTaken;
          p += max(1u, len);
        }
    }
    ent = cb + Z.exitp;
    __syncthreads();
  }
  *extra_bits = extra;
  *matches = nm;
}

extern __shared__ unsigned long long lz_dyn[];  // match mode LZ: a strip's filtered bytes + kFbSlack, if they fit

template <bool kLz>
__global__ __launch_bounds__(kThreads) void png_strip_kernel(PngArgs a) {
  __shared__ StripLds L;
  __shared__ typename std::conditional<kLz, LzLds, LzNone>::type Z;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int s = blockIdx.x, b = blockIdx.y;
  const PngGeom& g = a.g;
  const int W3 = g.rowb - 1;
  const int r0 = s * g.rps;
  const int rows = min(g.rps, g.H - r0);
  const unsigned n = (unsigned)rows * (unsigned)g.rowb;  // filtered bytes of the strip
  const uint8_t* img = a.img + (size_t)b * g.H * W3;
  uint8_t* sc = a.scratch + (size_t)b * g.scratch_image;
  uint8_t* slot = sc + (size_t)s * g.cap;
  uint8_t* ftypes = sc + g.off_ftype;
  const bool first = s == 0, last = s == g.ns - 1;
  uint8_t* fb = nullptr;    // match mode LZ: the strip's filtered bytes and match words
  unsigned* md = nullptr;
  // the matcher reads the bytes from LDS when the launch gave it room for a whole strip
  const bool in_lds = kLz && a.lds_bytes >= (unsigned)(g.rps * g.rowb + kFbSlack);
  if constexpr (kLz) {
    fb = sc + g.off_lz + (size_t)s * g.lz_stride;
    md = (unsigned*)(fb + g.lz_md);
    for (int k = tid; k < kSymPad; k += kThreads) Z.hist[k] = 0;
    if (tid < 32) { Z.dhist[tid] = 0; Z.clhist[tid] = 0; }
    if (tid == 0) { Z.nl = 0; Z.nd = 0; }
  }

  // CRC table and cleared LDS
  {
    unsigned c = (unsigned)tid;
#pragma unroll
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1;
    L.crctab[tid] = c;
  }
  for (int k = tid; k < kSymPad; k += kThreads) L.hist[k] = 0;
  for (int k = tid; k < kStageWords; k += kThreads) L.stage[k] = 0;
  if (tid < 32) L.clhist[tid] = 0;

  // ---- 1a: each row's filter (one wave per row) ----
  for (int r = wv; r < rows; r += kThreads / 64) {
    int ft = a.filter;
    if (a.filter == kFilterAdaptive) {
      const uint8_t* row = img + (size_t)(r0 + r) * W3;
      const uint8_t* up = (r0 + r) > 0 ? row - W3 : nullptr;
      unsigned sum[5] = {0, 0, 0, 0, 0};
      for (int c = lane; c < W3; c += 64) {
        const int x = row[c];
        const int av = c >= 3 ? row[c - 3] : 0;
        const int bv = up ? up[c] : 0;
        const int cv = (up && c >= 3) ? up[c - 3] : 0;
        sum[0] += msad((unsigned)x);
        sum[1] += msad((unsigned)(x - av) & 255u);
        sum[2] += msad((unsigned)(x - bv) & 255u);
        sum[3] += msad((unsigned)(x - ((av + bv) >> 1)) & 255u);
        sum[4] += msad((unsigned)(x - paeth_pred(av, bv, cv)) & 255u);
      }
#pragma unroll
      for (int k = 0; k < 5; ++k)
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) sum[k] += __shfl_xor(sum[k], d, 64);
      ft = 0;
#pragma unroll
      for (int k = 1; k < 5; ++k)
        if (sum[k] < sum[ft]) ft = k;
    }
    if (lane == 0) ftypes[r0 + r] = (uint8_t)ft;
  }
  __syncthreads();

  // ---- 1b: histogram of the filtered bytes and the Adler partial sums ----
  // filtered byte i of the strip: row i / rowb, filter type at column 0, raw byte col - 1 after it
  unsigned long long adA = 0, adB = 0;
  for (unsigned base = 0; base < n; base += kChunk) {
    unsigned i = base + (unsigned)tid * kRun;
    if (i >= n) continue;
    const unsigned end = min(i + (unsigned)kRun, n);
    int r = (int)(i / (unsigned)g.rowb), col = (int)(i - (unsigned)r * (unsigned)g.rowb);
    int ft = ftypes[r0 + r];
    const uint8_t* row = img + (size_t)(r0 + r) * W3;
    const uint8_t* up = (r0 + r) > 0 ? row - W3 : nullptr;
    unsigned prev = 256, run = 0;
    for (; i < end; ++i) {
      const unsigned d = col == 0 ? (unsigned)ft : filt_byte(row, up, col - 1, ft);
      if constexpr (kLz) {
        fb[i] = (uint8_t)d;
        if (in_lds) ((uint8_t*)lz_dyn)[i] = (uint8_t)d;
      }
      adA += d;
      adB += (unsigned long long)(n - i) * d;
      if (d == prev) ++run;
      else {
        if (run) atomicAdd(&L.hist[prev], run);
        prev = d; run = 1;
      }
      if (++col == g.rowb) {
        col = 0; ++r;
        if (r < rows) {
          ft = ftypes[r0 + r];
          up = row; row += W3;
        }
      }
    }
    if (run) atomicAdd(&L.hist[prev], run);
  }
  adA = block_sum_u64(adA, L.red64);
  adB = block_sum_u64(adB, L.red64);
  if (tid == 0) {
    L.hist[256] = 1;
    unsigned* ad = (unsigned*)(sc + g.off_adler) + 2 * s;
    ad[0] = (unsigned)(adA % kAdlerMod);
    ad[1] = (unsigned)(adB % kAdlerMod);
  }
  __syncthreads();

  // ---- 2: code lengths, codes, header size ----
  huff_lengths(L.hist, kLit, 15, L.lens, L.hw);
  // the 258 code lengths sent: 257 literal/length codes and one distance code of length 0
  for (int k = tid; k < kLit + 1; k += kThreads) atomicAdd(&L.clhist[k < kLit ? L.lens[k] : 0u], 1u);
  __syncthreads();
  huff_lengths(L.clhist, kCl, 7, L.cllens, L.hw);
  huff_codes(L.lens, kLit, L.codes, L.hw);
  huff_codes(L.cllens, kCl, L.clcodes, L.hw);
  unsigned long long bits = 0;
  for (int k = tid; k < kLit + 1; k += kThreads) {
    bits += L.cllens[k < kLit ? L.lens[k] : 0u];
    if (k < kLit) bits += (unsigned long long)L.hist[k] * L.lens[k];
  }
  bits = block_sum_u64(bits, L.red64) + 17 + 3 * kCl + 3;
  const unsigned pre = first ? 2u : 0u;  // the zlib header
  const unsigned long long huff_bytes = ((bits + 7) >> 3) + 4;
  const unsigned nblk = (n + 65534u) / 65535u;
  const unsigned long long stor_bytes = (unsigned long long)n + 5ull * nblk + 5;
  uint8_t* data = slot + 8;
  unsigned datalen = 0;

  // ---- match mode LZ: matches, the greedy parse, its two codes and its size ----
  bool use_lz = false;
  if constexpr (kLz) {
    unsigned short* ent2 = (unsigned short*)(L.stage + kStepTab);
    unsigned long long extra, nm;
    if (in_lds) lz_match(lz_dyn, md, n, (unsigned)g.rowb, Z, L.stage);
    else lz_match((const unsigned long long*)fb, md, n, (unsigned)g.rowb, Z, L.stage);
    lz_parse(fb, md, n, Z, ent2, ent2 + kRun, &extra, &nm);
    extra = block_sum_u64(extra, L.red64);
    nm = block_sum_u64(nm, L.red64);
    for (int k = tid; k < kStepTab + (kRun + kThreads) / 2; k += kThreads) L.stage[k] = 0;
    if (tid == 0) Z.hist[256] = 1;
    __syncthreads();
    if (nm) {  // uniform; without a match the strip is the literal-only block
      huff_lengths(Z.hist, kLl, 15, Z.lens, L.hw);
      huff_lengths(Z.dhist, kDist, 15, Z.dlens, L.hw);
      for (int k = tid; k < kLl; k += kThreads)
        if (Z.lens[k]) atomicMax(&Z.nl, (unsigned)k + 1);
      if (tid < kDist && Z.dlens[tid]) atomicMax(&Z.nd, (unsigned)tid + 1);
      __syncthreads();
      const unsigned nl = Z.nl, nd = Z.nd;  // nl >= 257: end-of-block is used
      for (unsigned k = tid; k < nl + nd; k += kThreads) atomicAdd(&Z.clhist[k < nl ? Z.lens[k] : Z.dlens[k - nl]], 1u);
      __syncthreads();
      huff_lengths(Z.clhist, kCl, 7, Z.cllens, L.hw);
      unsigned long long zb = 0;
      for (unsigned k = tid; k < nl + nd; k += kThreads) {
        if (k < nl) zb += Z.cllens[Z.lens[k]] + (unsigned long long)Z.hist[k] * Z.lens[k];
        else zb += Z.cllens[Z.dlens[k - nl]] + (unsigned long long)Z.dhist[k - nl] * Z.dlens[k - nl];
      }
      zb = block_sum_u64(zb, L.red64) + extra + 17 + 3 * kCl + 3;
      const unsigned long long lz_bytes = ((zb + 7) >> 3) + 4;
      use_lz = lz_bytes < huff_bytes && lz_bytes < stor_bytes;
    }
  }

  if (use_lz) {
    if constexpr (kLz) {
      // ---- 3z: block header and code lengths, one entry per filtered byte (nothing for a byte
      // inside a match), end-of-block and the empty stored block's 3 bits
      huff_codes(Z.lens, kLl, Z.codes, L.hw);
      huff_codes(Z.dlens, kDist, Z.dcodes, L.hw);
      huff_codes(Z.cllens, kCl, Z.clcodes, L.hw);
      const unsigned nl = Z.nl, nd = Z.nd;
      const unsigned P = first ? 1u : 0u;
      unsigned carry = 0, outw = 0;
      unsigned* dataw = (unsigned*)data;
      unsigned long long sym[kRun];
      static_assert(2 + kCl + kLl + kDist <= kChunk, "the header is one chunk");
#pragma unroll
      for (int k = 0; k < kRun; ++k) {
        const unsigned j = (unsigned)tid * kRun + (unsigned)k;
        unsigned e = 0;
        if (j < P) e = 0x0178u | (16u << 24);
        else if (j == P) e = (2u << 1) | ((nl - 257u) << 3) | ((nd - 1u) << 8) | (15u << 13) | (17u << 24);
        else if (j < P + 1 + kCl) e = Z.cllens[kClOrder[j - P - 1]] | (3u << 24);
        else if (j < P + 1 + kCl + nl) e = Z.clcodes[Z.lens[j - P - 1 - kCl]];
        else if (j < P + 1 + kCl + nl + nd) e = Z.clcodes[Z.dlens[j - P - 1 - kCl - nl]];
        sym[k] = (unsigned long long)(e & 0xffffffu) | (unsigned long long)(e >> 24) << 56;
      }
      emit_chunk(sym, L, dataw, carry, outw);
      for (unsigned base = 0; base < n; base += kChunk) {
#pragma unroll
        for (int k = 0; k < kRun; ++k) {
          const unsigned i = base + (unsigned)tid * kRun + (unsigned)k;
          unsigned long long v = 0;
          const unsigned m = i < n ? md[i] : 0u;
          if (m & kTaken) {
            const unsigned len = m & (kTaken - 1);
            if (len) {
              unsigned le, de;
              const unsigned dist = m >> 16;
              const unsigned lc = Z.codes[len_code(len, &le)], dc = Z.dcodes[dist_code(dist, &de)];
              unsigned c = lc >> 24;
              v = lc & 0xffffffu;
              v |= (unsigned long long)((len - 3) & ((1u << le) - 1)) << c;
              c += le;
              v |= (unsigned long long)(dc & 0xffffffu) << c;
              c += dc >> 24;
              v |= (unsigned long long)((dist - 1) & ((1u << de) - 1)) << c;
              c += de;
              v |= (unsigned long long)c << 56;
            } else {
              const unsigned lc = Z.codes[fb[i]];
              v = (unsigned long long)(lc & 0xffffffu) | (unsigned long long)(lc >> 24) << 56;
            }
          }
          sym[k] = v;
        }
        emit_chunk(sym, L, dataw, carry, outw);
      }
#pragma unroll
      for (int k = 0; k < kRun; ++k) {
        unsigned e = 0;
        if (tid == 0 && k == 0) e = Z.codes[256];
        if (tid == 0 && k == 1) e = (last ? 1u : 0u) | (3u << 24);
        sym[k] = (unsigned long long)(e & 0xffffffu) | (unsigned long long)(e >> 24) << 56;
      }
      emit_chunk(sym, L, dataw, carry, outw);
      const unsigned nby = (carry + 7) >> 3;
      if (tid == 0) {
        uint8_t* p = data + (size_t)outw * 4;
        const unsigned cw = L.stage[0];
        for (unsigned k = 0; k < nby; ++k) p[k] = (uint8_t)(cw >> (8 * k));
        p[nby] = 0; p[nby + 1] = 0; p[nby + 2] = 0xFF; p[nby + 3] = 0xFF;
      }
      datalen = outw * 4 + nby + 4;
    }
  } else if (huff_bytes < stor_bytes) {
    // ---- 3: the bit stream.  Symbol space: [zlib header] block header, 19 code-length
    // lengths, 258 coded lengths, n literals, end-of-block, the empty stored block's 3 bits
    const unsigned P = first ? 1u : 0u;
    const unsigned lit0 = P + 1 + kCl + kLit + 1;
    const unsigned J = lit0 + n + 2;
    unsigned carry = 0;       // bits already in stage[0]
    unsigned outw = 0;        // words flushed
    unsigned* dataw = (unsigned*)data;
    for (unsigned base = 0; base < J; base += kChunk) {
      unsigned sym[kRun];     // bits | count << 24
      unsigned nbits = 0;
      const unsigned j0 = base + (unsigned)tid * kRun;
      int r = 0, col = 0, ft = 0;
      const uint8_t* row = img;
      const uint8_t* up = nullptr;
      bool have = false;
#pragma unroll
      for (int k = 0; k < kRun; ++k) {
        const unsigned j = j0 + k;
        unsigned e = 0;
        if (j >= J) {
        } else if (j < P) {
          e = 0x0178u | (16u << 24);
        } else if (j == P) {
          e = (2u << 1) | (15u << 13) | (17u << 24);  // BTYPE 2, HLIT 0, HDIST 0, HCLEN 15
        } else if (j < P + 1 + kCl) {
          e = L.cllens[kClOrder[j - P - 1]] | (3u << 24);
        } else if (j < lit0) {
          const unsigned k2 = j - P - 1 - kCl;
          e = L.clcodes[k2 < kLit ? L.lens[k2] : 0u];
        } else if (j < lit0 + n) {
          if (!have) {
            const unsigned i = j - lit0;
            r = (int)(i / (unsigned)g.rowb);
            col = (int)(i - (unsigned)r * (unsigned)g.rowb);
            ft = ftypes[r0 + r];
            row = img + (size_t)(r0 + r) * W3;
            up = (r0 + r) > 0 ? row - W3 : nullptr;
            have = true;
          }
          const unsigned d = col == 0 ? (unsigned)ft : filt_byte(row, up, col - 1, ft);
          e = L.codes[d];
          if (++col == g.rowb) {
            col = 0; ++r;
            if (r < rows) {
              ft = ftypes[r0 + r];
              up = row; row += W3;
            }
          }
        } else if (j == lit0 + n) {
          e = L.codes[256];
        } else {
          e = (last ? 1u : 0u) | (3u << 24);
        }
        sym[k] = e;
        nbits += e >> 24;
      }
      unsigned total;
      unsigned pos = carry + block_excl_scan(nbits, L.red, &total);
      // merge at the run boundaries only: whole words of a run go out as they fill
      unsigned wi = pos >> 5, nb = pos & 31u;
      unsigned long long acc = 0;
#pragma unroll
      for (int k = 0; k < kRun; ++k) {
        acc |= (unsigned long long)(sym[k] & 0xffffffu) << nb;
        nb += sym[k] >> 24;
        if (nb >= 32) {
          atomicOr(&L.stage[wi], (unsigned)acc);
          ++wi; acc >>= 32; nb -= 32;
        }
      }
      if (nb) atomicOr(&L.stage[wi], (unsigned)acc);
      __syncthreads();
      const unsigned T = carry + total;
      const unsigned full = T >> 5;
      for (unsigned k = tid; k < full; k += kThreads) dataw[outw + k] = L.stage[k];
      const unsigned cw = L.stage[full];
      __syncthreads();
      for (unsigned k = tid; k <= full; k += kThreads) L.stage[k] = 0;
      __syncthreads();
      if (tid == 0) L.stage[0] = cw;
      __syncthreads();
      outw += full;
      carry = T & 31u;
    }
    // pad to the byte, then LEN = 0, NLEN = 0xFFFF of the empty stored block
    const unsigned nby = (carry + 7) >> 3;
    if (tid == 0) {
      uint8_t* p = data + (size_t)outw * 4;
      const unsigned cw = L.stage[0];
      for (unsigned k = 0; k < nby; ++k) p[k] = (uint8_t)(cw >> (8 * k));
      p[nby] = 0; p[nby + 1] = 0; p[nby + 2] = 0xFF; p[nby + 3] = 0xFF;
    }
    datalen = outw * 4 + nby + 4;
  } else {
    // ---- 3': stored blocks of at most 65535 bytes, then the empty stored block ----
    if (first && tid == 0) { data[0] = 0x78; data[1] = 0x01; }
    uint8_t* p = data + pre;
    for (unsigned k = tid; k < nblk; k += kThreads) {
      const unsigned len = min(65535u, n - k * 65535u);
      uint8_t* h = p + (size_t)k * 65540u;
      h[0] = 0; h[1] = (uint8_t)len; h[2] = (uint8_t)(len >> 8); h[3] = (uint8_t)~len; h[4] = (uint8_t)(~len >> 8);
    }
    for (unsigned i = tid; i < n; i += kThreads) {
      const int r = (int)(i / (unsigned)g.rowb), col = (int)(i - (unsigned)r * (unsigned)g.rowb);
      const int ft = ftypes[r0 + r];
      const uint8_t* row = img + (size_t)(r0 + r) * W3;
      const uint8_t* up = (r0 + r) > 0 ? row - W3 : nullptr;
      const unsigned d = col == 0 ? (unsigned)ft : filt_byte(row, up, col - 1, ft);
      p[(size_t)i + 5u * (i / 65535u + 1u)] = (uint8_t)d;
    }
    if (tid == 0) {
      uint8_t* e = p + (size_t)n + 5u * nblk;
      e[0] = last ? 1 : 0; e[1] = 0; e[2] = 0; e[3] = 0xFF; e[4] = 0xFF;
    }
    datalen = pre + n + 5u * nblk + 5u;
  }
  if (tid == 0) {
    put_be32(slot, datalen);
    slot[4] = 'I'; slot[5] = 'D'; slot[6] = 'A'; slot[7] = 'T';
  }
  __syncthreads();

  // ---- CRC-32 of type + data: one table-driven CRC per thread over a slice, each advanced by
  // the bytes behind its slice (times x^(8 n)), then XORed ----
  {
    const unsigned len = datalen + 4;
    const unsigned per = (len + kThreads - 1) / kThreads;
    const unsigned lo = min(len, (unsigned)tid * per), hi = min(len, lo + per);
    unsigned c = tid == 0 ? 0xFFFFFFFFu : 0u;
    const uint8_t* q = slot + 4;
    for (unsigned k = lo; k < hi; ++k) c = L.crctab[(c ^ q[k]) & 255u] ^ (c >> 8);
    if (c && hi < len) c = gf_mul(gf_x8n(len - hi), c);
    c = block_xor_u32(c, L.red) ^ 0xFFFFFFFFu;
    if (tid == 0) {
      put_be32(slot + 8 + datalen, c);
      ((unsigned*)(sc + g.off_sizes))[s] = datalen + 12;
    }
  }
}

// One workgroup per image: where each chunk goes, the Adler-32, and the fixed parts of the file.
__global__ __launch_bounds__(kThreads) void png_layout_kernel(PngArgs a) {
  __shared__ unsigned red[8];
  __shared__ unsigned long long red64[4];
  const int tid = threadIdx.x, b = blockIdx.x;
  const PngGeom& g = a.g;
  uint8_t* sc = a.scratch + (size_t)b * g.scratch_image;
  const unsigned* sizes = (const unsigned*)(sc + g.off_sizes);
  const unsigned* ad = (const unsigned*)(sc + g.off_adler);
  unsigned* offs = (unsigned*)(sc + g.off_offs);
  uint8_t* out = a.out + (size_t)b * a.out_stride;
  // each thread owns `per` consecutive strips
  const int per = (g.ns + kThreads - 1) / kThreads;
  const int lo = min(g.ns, tid * per), hi = min(g.ns, lo + per);
  unsigned bytes = 0, sumA = 0;
  for (int k = lo; k < hi; ++k) { bytes += sizes[k]; sumA = (sumA + ad[2 * k]) % kAdlerMod; }
  unsigned total, totalA;
  unsigned off = block_excl_scan(bytes, red, &total);
  unsigned preA = block_excl_scan(sumA, red, &totalA);  // < 256 * 65521
  // s1 before strip k = 1 + sum of A below it; s2 = sum over strips of n_k * s1 + B_k
  unsigned long long s2 = 0;
  unsigned s1 = (1u + preA) % kAdlerMod;
  for (int k = lo; k < hi; ++k) {
    offs[k] = off;
    off += sizes[k];
    const unsigned nk = (unsigned)min(g.rps, g.H - k * g.rps) * (unsigned)g.rowb;
    s2 += (unsigned long long)(nk % kAdlerMod) * s1 + ad[2 * k + 1];
    s1 = (s1 + ad[2 * k]) % kAdlerMod;
  }
  s2 = block_sum_u64(s2 % kAdlerMod, red64) % kAdlerMod;
  if (tid == 0) {
    const unsigned adler = ((unsigned)s2 << 16) | ((1u + totalA) % kAdlerMod);
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    for (int k = 0; k < 8; ++k) out[k] = sig[k];
    uint8_t* p = out + 8;
    put_be32(p, 13);
    p[4] = 'I'; p[5] = 'H'; p[6] = 'D'; p[7] = 'R';
    put_be32(p + 8, (unsigned)g.W);
    put_be32(p + 12, (unsigned)g.H);
    p[16] = 8; p[17] = 2; p[18] = 0; p[19] = 0; p[20] = 0;
    unsigned c = 0xFFFFFFFFu;
    for (int k = 4; k < 21; ++k) c = crc_bitwise(c, p[k]);
    put_be32(p + 21, ~c);
    uint8_t* t = out + kHeadBytes + total;
    put_be32(t, 4);
    t[4] = 'I'; t[5] = 'D'; t[6] = 'A'; t[7] = 'T';
    put_be32(t + 8, adler);
    c = 0xFFFFFFFFu;
    for (int k = 4; k < 12; ++k) c = crc_bitwise(c, t[k]);
    put_be32(t + 12, ~c);
    put_be32(t + 16, 0);
    t[20] = 'I'; t[21] = 'E'; t[22] = 'N'; t[23] = 'D';
    c = 0xFFFFFFFFu;
    for (int k = 20; k < 24; ++k) c = crc_bitwise(c, t[k]);
    put_be32(t + 24, ~c);
    a.sizes[b] = (long long)kHeadBytes + total + kTailBytes;
  }
}

__global__ __launch_bounds__(kThreads) void png_gather_kernel(PngArgs a) {
  const int s = blockIdx.x, b = blockIdx.y;
  const PngGeom& g = a.g;
  const uint8_t* sc = a.scratch + (size_t)b * g.scratch_image;
  const unsigned size = ((const unsigned*)(sc + g.off_sizes))[s];
  const unsigned off = ((const unsigned*)(sc + g.off_offs))[s];
  const uint8_t* src = sc + (size_t)s * g.cap;
  uint8_t* dst = a.out + (size_t)b * a.out_stride + kHeadBytes + off;
  // bytes up to dst's 4-byte boundary, then whole words assembled from the (aligned) source
  const unsigned head = min(size, (unsigned)((4 - ((size_t)dst & 3)) & 3));
  if (threadIdx.x < head) dst[threadIdx.x] = src[threadIdx.x];
  const unsigned words = (size - head) >> 2;
  const unsigned sh = head * 8;
  const unsigned* sw = (const unsigned*)src;
  unsigned* dw = (unsigned*)(dst + head);
  for (unsigned k = threadIdx.x; k < words; k += kThreads)
    dw[k] = sh ? (sw[k] >> sh) | (sw[k + 1] << (32 - sh)) : sw[k];
  const unsigned done = head + words * 4;
  if (threadIdx.x < size - done) dst[done + threadIdx.x] = src[done + threadIdx.x];
}

}  // namespace

int png_bound(int H, int W, int rps, int match, size_t* bytes_per_image, size_t* scratch_bytes) {
  PngGeom g;
  const int rc = png_geom(H, W, rps, match, &g);
  if (rc != kOk) return rc;
  if (bytes_per_image) *bytes_per_image = g.file_bound;
  if (scratch_bytes) *scratch_bytes = g.scratch_image;
  return kOk;
}

int launch_png_encode(const uint8_t* img, int B, int H, int W, int filter, int match, int rps, uint8_t* out,
                      size_t out_stride, long long* sizes, uint8_t* scratch, size_t scratch_bytes, hipStream_t st) {
  PngArgs a;
  const int rc = png_geom(H, W, rps, match, &a.g);
  if (rc != kOk) return rc;
  if (out_stride < a.g.file_bound) return kErrArg;
  if (scratch_bytes / (size_t)B < a.g.scratch_image) return kErrWorkspace;
  if (B > 65535 || a.g.ns > 0x7fffffff / 2) return kErrShape;
  a.img = img; a.scratch = scratch; a.out = out; a.sizes = sizes; a.out_stride = out_stride; a.filter = filter;
  const size_t strip_lds = align_up((size_t)a.g.rps * a.g.rowb + kFbSlack, 16);
  a.lds_bytes = (match == kMatchLz && strip_lds <= kLzLdsMax) ? (unsigned)strip_lds : 0u;
  if (match == kMatchLz) png_strip_kernel<true><<<dim3(a.g.ns, B), kThreads, a.lds_bytes, st>>>(a);
  else png_strip_kernel<false><<<dim3(a.g.ns, B), kThreads, 0, st>>>(a);
  png_layout_kernel<<<dim3(B), kThreads, 0, st>>>(a);
  png_gather_kernel<<<dim3(a.g.ns, B), kThreads, 0, st>>>(a);
  UPR_CHECK_HIP(hipGetLastError());
  return kOk;
}

}  // namespace upr
