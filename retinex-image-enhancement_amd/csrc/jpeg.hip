// Baseline JPEG encoder on the device (include/upr.h upr_jpeg_encode_ex).
//
// File: SOI, APP0 JFIF, DQT x2, SOF0 (8-bit, Y/Cb/Cr, every component 1x1), DHT x4 (the Annex K
// tables), DRI, SOS, the entropy-coded data, EOI.  A restart interval is restart_rows rows of
// MCUs: its DC predictors start at 0 and it ends on a byte boundary, so one workgroup
// writes it without knowing the others.  All arithmetic is integer and stated in DESIGN.md 4.6
// (tests/jpeg_ref.py and tests/jpeg_modes_ref.py restate it in numpy; the files are equal byte
// for byte).  Modes: 4:4:4 (an MCU is 8x8 pixels, units Y Cb Cr), 4:2:0 (16x16 pixels, units
// Y00 Y01 Y10 Y11 Cb Cr, chroma the 2x2 box of the per-pixel values) and gray (8x8 pixels, one
// unit, one DQT and two DHT segments); Huffman tables from Annex K or built per image from the
// image's own symbol counts (Annex K.2 with the Figure K.3 length limit).
//
//   jpeg_interval_kernel  one workgroup per (interval, image), one thread per block-component
//                         (unit), 256 units per pass in MCU order: colour, DCT, quantisation and
//                         zigzag in registers, the coefficients to LDS, the DC differences through
//                         LDS, a prefix sum of the units' bit lengths, the codes ORed as whole
//                         words into an LDS window of the bit stream, a second prefix sum over
//                         the 0xFF bytes, the stuffed bytes to a second LDS stage and from there
//                         as dwords into the interval's scratch slot.  Its counting form stops
//                         behind the DC differences: the symbols go into an LDS histogram per
//                         table and from there with integer atomics into the image's histogram
//   jpeg_huffman_kernel   one workgroup per image, one wave per table: the image's histograms ->
//                         code | length << 16 per symbol and the DHT payloads, in scratch
//   jpeg_layout_kernel    one workgroup per image: scan of the interval sizes, headers, EOI, sizes[b]
//   jpeg_gather_kernel    one workgroup per (interval, image): slot -> its place in the file
//
// Every byte is written with ordinary vector stores; nothing is computed on the host but the
// quality's scale factor.
#include "upr_common.h"

namespace upr {

namespace {

constexpr int kThreads = 256;
constexpr int kStageWords = 2048;               // words of the bit-stream window in LDS
constexpr unsigned kWindowBits = kStageWords * 32u;
constexpr int kHeadBytes = 629;                 // SOI .. SOS of a colour file with the Annex K tables
constexpr int kOffQ0 = 25, kOffQ1 = 94, kOffDim = 163, kOffRi = 613;  // fields of that header
constexpr int kSubs = 3;                        // UPR_JPEG_444, _420, _GRAY
constexpr int kSub444 = 0, kSub420 = 1, kSubGray = 2;
// segments of the colour header, as the layout kernel assembles every mode's header from them
constexpr int kSegApp0End = 20, kSegDqt = 69, kSegDht0 = 177;
constexpr int kSegDhtStdDc = 33, kSegDhtStdAc = 183;  // in the order DC0, AC0, DC1, AC1
// gray: one DQT, a SOF0 and a SOS of one component, DC0 and AC0 alone
constexpr int kHeadBytesGray = kSegApp0End + kSegDqt + 13 + kSegDhtStdDc + kSegDhtStdAc + 6 + 10;
static_assert(kHeadBytes == kSegApp0End + 2 * kSegDqt + 19 + 2 * (kSegDhtStdDc + kSegDhtStdAc) + 6 + 14 &&
                  kHeadBytesGray == 334,
              "UPR_JPEG_HEADER_BYTES and UPR_JPEG_HEADER_BYTES_GRAY of include/upr.h");
constexpr int kHuffTables = 4;                  // DC0, AC0, DC1, AC1: table t is class t & 1, id t >> 1
constexpr int kHuffFreq = 257;                  // counts of a table as upr_jpeg_huffman_build takes them
constexpr int kHuffPayload = 16 + 256;          // BITS, HUFFVAL
constexpr unsigned kHuffScale = 1u << 22;       // counts are halved while their total is above

// ---- the format's tables (Annex K), as a DQT / DHT segment carries them -------------------------
struct JpegConst {
  uint8_t baseq[2][64];     // K.1 / K.2 in zigzag order, scale 100
  uint8_t dc_bits[2][16], dc_vals[2][12];
  uint8_t ac_bits[2][16], ac_vals[2][162];
};
constexpr JpegConst kC = {
    {{16, 11, 12, 14, 12, 10, 16, 14, 13, 14, 18, 17, 16, 19, 24, 40, 26, 24, 22, 22, 24, 49,
      35, 37, 29, 40, 58, 51, 61, 60, 57, 51, 56, 55, 64, 72, 92, 78, 64, 68, 87, 69, 55, 56,
      80, 109, 81, 87, 95, 98, 103, 104, 103, 62, 77, 113, 121, 112, 100, 120, 92, 101, 103, 99},
     {17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66, 99, 99, 99, 99, 99, 99, 99, 99,
      99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
      99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}},
    {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}},
    {{0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}},
    {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}},
    {{1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177,
      193, 21, 82, 209, 240, 36, 51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53,
      54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102,
      103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146,
      147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181,
      182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216,
      217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249,
      250},
     {0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193,
      9, 35, 51, 82, 240, 21, 98, 114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42,
      53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101,
      102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137,
      138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179,
      180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214,
      215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249,
      250}}};

constexpr int longest_code(const uint8_t (&bits)[16]) {
  int l = 0;
  for (int k = 0; k < 16; ++k)
    if (bits[k]) l = k + 1;
  return l;
}
constexpr int cmax(int a, int b) { return a > b ? a : b; }
// no block is longer: a DC code and 11 value bits, 63 AC codes with 10 value bits each
constexpr int kMaxBlockBits = cmax(longest_code(kC.dc_bits[0]), longest_code(kC.dc_bits[1])) + 11 +
                              63 * (cmax(longest_code(kC.ac_bits[0]), longest_code(kC.ac_bits[1])) + 10);
static_assert(kMaxBlockBits == 22 + 63 * 26, "the bound documented in include/upr.h");
// with a table built per image the longest code, DC or AC, is 16 bits
constexpr int kMaxBlockBitsOpt = (16 + 11) + 63 * (16 + 10);
static_assert(kMaxBlockBitsOpt == 1665, "UPR_JPEG_MAX_BLOCK_BITS_OPTIMIZED of include/upr.h");
static_assert(kMaxBlockBitsOpt + 32 <= (int)kWindowBits, "a unit that starts in the window's first word fits the window");

// what the kernels read: the encoder's view of the Huffman tables (code | length << 16 per
// symbol), the base quantisation tables and the headers with quality 50 tables, H = W = Ri = 0
struct JpegTables {
  alignas(16) uint32_t ac[2][256];
  uint32_t dc[2][12];
  uint8_t baseq[2][64];
  uint8_t header[kHeadBytes + 3];
};

constexpr void canonical(const uint8_t* bits, const uint8_t* vals, uint32_t* out) {
  uint32_t code = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int j = 0; j < bits[len - 1]; ++j) out[vals[k++]] = code++ | (uint32_t)len << 16;
    code <<= 1;
  }
}

constexpr int put_segment(uint8_t* h, int p, int marker, const uint8_t* body, int n) {
  h[p++] = 0xFF; h[p++] = (uint8_t)marker;
  h[p++] = (uint8_t)((n + 2) >> 8); h[p++] = (uint8_t)(n + 2);
  for (int k = 0; k < n; ++k) h[p++] = body[k];
  return p;
}

constexpr JpegTables make_tables() {
  JpegTables t{};
  for (int c = 0; c < 2; ++c) {
    canonical(kC.dc_bits[c], kC.dc_vals[c], t.dc[c]);
    canonical(kC.ac_bits[c], kC.ac_vals[c], t.ac[c]);
    for (int k = 0; k < 64; ++k) t.baseq[c][k] = kC.baseq[c][k];
  }
  uint8_t* h = t.header;
  int p = 0;
  h[p++] = 0xFF; h[p++] = 0xD8;
  const uint8_t jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  p = put_segment(h, p, 0xE0, jfif, 14);
  for (int c = 0; c < 2; ++c) {
    uint8_t body[65] = {};
    body[0] = (uint8_t)c;
    for (int k = 0; k < 64; ++k) body[1 + k] = kC.baseq[c][k];
    p = put_segment(h, p, 0xDB, body, 65);
  }
  const uint8_t sof[15] = {8, 0, 0, 0, 0, 3, 1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1};
  p = put_segment(h, p, 0xC0, sof, 15);
  for (int c = 0; c < 2; ++c) {
    uint8_t body[179] = {};
    body[0] = (uint8_t)c;
    for (int k = 0; k < 16; ++k) body[1 + k] = kC.dc_bits[c][k];
    for (int k = 0; k < 12; ++k) body[17 + k] = kC.dc_vals[c][k];
    p = put_segment(h, p, 0xC4, body, 29);
    body[0] = (uint8_t)(0x10 | c);
    for (int k = 0; k < 16; ++k) body[1 + k] = kC.ac_bits[c][k];
    for (int k = 0; k < 162; ++k) body[17 + k] = kC.ac_vals[c][k];
    p = put_segment(h, p, 0xC4, body, 179);
  }
  const uint8_t dri[2] = {0, 0};
  p = put_segment(h, p, 0xDD, dri, 2);
  const uint8_t sos[10] = {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
  p = put_segment(h, p, 0xDA, sos, 10);
  h[kHeadBytes] = (uint8_t)(p == kHeadBytes);  // checked below
  return t;
}
constexpr JpegTables kTablesHost = make_tables();
static_assert(kTablesHost.header[kHeadBytes] == 1, "SOI .. SOS is kHeadBytes long");
static_assert(kTablesHost.header[kOffQ0 - 5] == 0xFF && kTablesHost.header[kOffQ0 - 4] == 0xDB &&
                  kTablesHost.header[kOffQ1 - 5] == 0xFF && kTablesHost.header[kOffQ1 - 4] == 0xDB &&
                  kTablesHost.header[kOffDim - 5] == 0xFF && kTablesHost.header[kOffDim - 4] == 0xC0 &&
                  kTablesHost.header[kOffRi - 4] == 0xFF && kTablesHost.header[kOffRi - 3] == 0xDD,
              "offsets of the patched header fields");
__device__ __constant__ const JpegTables kT = make_tables();

// what the Huffman kernel leaves in an image's scratch (and, in freq, what the counting pass does)
struct HuffImage {
  uint32_t freq[kHuffTables][kHuffFreq];
  uint32_t code[kHuffTables][256];             // code | length << 16 by symbol
  uint8_t bits_vals[kHuffTables][kHuffPayload];
  int32_t nvals[kHuffTables];
};

struct JpegGeom {
  int H, W, bw, bh, rr, ni;  // bw x bh MCUs, ni intervals of rr MCU rows (the last may be shorter)
  int sub, opt;              // UPR_JPEG_444 / _420 / _GRAY; tables built per image
  size_t cap;                // bytes of one interval's scratch slot
  size_t file_bound;         // bytes of one image's file, at most
  size_t scratch_image;      // scratch bytes of one image
  size_t off_sizes, off_offs;  // u32 arrays behind the ni slots
  size_t off_head;           // u32: the header's length, as the layout kernel wrote it
  size_t off_huff;           // HuffImage
};

constexpr int units_per_mcu(int sub) { return sub == kSub420 ? 6 : (sub == kSubGray ? 1 : 3); }

// an interval of `blocks` blocks: the blocks at their longest rounded up to bytes, doubled for
// the stuffing, and the marker behind it (RSTm; EOI behind the last)
inline long long interval_bound(long long blocks, int opt) {
  return 2 * ((blocks * (opt ? kMaxBlockBitsOpt : kMaxBlockBits) + 7) / 8) + 2;
}

int jpeg_geom(int H, int W, int restart_rows, int sub, int opt, JpegGeom* g) {
  if (H <= 0 || W <= 0 || restart_rows <= 0) return kErrArg;
  if (sub < 0 || sub >= kSubs || opt < 0 || opt > 1) return kErrArg;
  if (H > 65535 || W > 65535) return kErrShape;
  const int m = sub == kSub420 ? 16 : 8;
  const int bw = (W + m - 1) / m, bh = (H + m - 1) / m;
  const int rr = restart_rows < bh ? restart_rows : bh;
  if ((long long)bw * rr > 65535) return kErrShape;  // DRI's 16-bit Ri
  const int ni = (bh + rr - 1) / rr;
  const int last = bh - (ni - 1) * rr;
  const long long upm = units_per_mcu(sub);
  const long long bound = (sub == kSubGray ? kHeadBytesGray : kHeadBytes) +
                          (ni - 1) * interval_bound(upm * bw * rr, opt) + interval_bound(upm * bw * last, opt);
  if (bound > (1LL << 31)) return kErrShape;
  g->H = H; g->W = W; g->bw = bw; g->bh = bh; g->rr = rr; g->ni = ni; g->sub = sub; g->opt = opt;
  // the stuffed bytes leave the kernel in whole dwords
  g->cap = align_up((size_t)interval_bound(upm * bw * rr, opt) + 4, 16);
  g->file_bound = (size_t)bound;
  g->off_sizes = (size_t)ni * g->cap;
  g->off_offs = g->off_sizes + align_up((size_t)ni * 4, 16);
  g->off_head = g->off_offs + align_up((size_t)ni * 4, 16);
  g->off_huff = g->off_head + 16;
  g->scratch_image = g->off_huff + (opt ? align_up(sizeof(HuffImage), 16) : 0);
  return kOk;
}

struct JpegArgs {
  const uint8_t* img;  // [B][H][W][3]
  uint8_t* scratch;
  uint8_t* out;
  long long* sizes;
  size_t out_stride;
  JpegGeom g;
  int qscale;          // libjpeg's scale factor of the quality, in percent
};

// ---- small workgroup helpers (kThreads = 4 waves of 64), as in png.hip --------------------------
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

// q = clamp((base * scale + 50) / 100, 1, 255)
__device__ __forceinline__ unsigned quant_step(unsigned base, int qscale) {
  const unsigned q = (base * (unsigned)qscale + 50u) / 100u;
  return q < 1u ? 1u : (q > 255u ? 255u : q);
}

// 8-point forward DCT of v[0], v[S], .. v[7 S] in place: out[k] = (sum_n C[k][n] v[n] + 2^(SH-1))
// >> SH with C[k][n] = round(2^13 s_k cos((2n + 1) k pi / 16)).  C[k][7 - n] = (-1)^k C[k][n]
// holds for the rounded integers, so the even / odd split is exact.  |v| < 2^15 and |C| < 2^13:
// the 24-bit multiply is exact and every sum stays below 2^28.
template <int S, int SH>
__device__ __forceinline__ void dct8(int* v) {
  const int s0 = v[0] + v[7 * S], s1 = v[S] + v[6 * S], s2 = v[2 * S] + v[5 * S], s3 = v[3 * S] + v[4 * S];
  const int d0 = v[0] - v[7 * S], d1 = v[S] - v[6 * S], d2 = v[2 * S] - v[5 * S], d3 = v[3 * S] - v[4 * S];
  const int e0 = s0 + s3, e1 = s1 + s2, o0 = s0 - s3, o1 = s1 - s2;
  constexpr int r = 1 << (SH - 1);
  v[0] = (__mul24(2896, e0 + e1) + r) >> SH;
  v[4 * S] = (__mul24(2896, e0 - e1) + r) >> SH;
  v[2 * S] = (__mul24(3784, o0) + __mul24(1567, o1) + r) >> SH;
  v[6 * S] = (__mul24(1567, o0) - __mul24(3784, o1) + r) >> SH;
  v[S] = (__mul24(4017, d0) + __mul24(3406, d1) + __mul24(2276, d2) + __mul24(799, d3) + r) >> SH;
  v[3 * S] = (__mul24(3406, d0) - __mul24(799, d1) - __mul24(4017, d2) - __mul24(2276, d3) + r) >> SH;
  v[5 * S] = (__mul24(2276, d0) - __mul24(4017, d1) + __mul24(799, d2) + __mul24(3406, d3) + r) >> SH;
  v[7 * S] = (__mul24(799, d0) - __mul24(2276, d1) + __mul24(3406, d2) - __mul24(4017, d3) + r) >> SH;
}

struct IntervalLds {
  short coef[64][kThreads];            // quantised coefficients, zigzag position major
  unsigned stage[kStageWords + 2];     // a window of the bit stream, MSB first in each word
  unsigned s2[2 * kStageWords + 4];    // stuffed bytes on their way out (bytes in memory order)
  unsigned ac[2][256];                 // code | length << 16
  unsigned dc[2][12];
  unsigned qr[2][64];                  // ceil(2^20 / q) | (q / 2) << 21, zigzag order
  short dcs[kThreads + 6];             // DC of the units of one MCU before the pass, then the pass's
  unsigned red[8];
  unsigned next;
};
static_assert(sizeof(IntervalLds) <= 64 * 1024, "LDS of the interval kernel");

// Bytes [0, 4 nwords + tail) of the stage (big-endian within each word) go through the stuffing
// (0x00 behind every 0xFF) into s2 behind its `obytes & 3` carried bytes and from there, in whole
// dwords, to the slot; `marker` >= 0 appends 0xFF, marker unstuffed.  obytes: bytes of the
// interval written so far.  All threads call it.
__device__ __forceinline__ void flush_bytes(IntervalLds& L, unsigned* slotw, unsigned nwords, unsigned tail, int marker,
                                            unsigned& obytes) {
  const int tid = threadIdx.x;
  const unsigned nw = nwords + (tail ? 1u : 0u);
  const unsigned per = (nw + kThreads - 1) / kThreads;
  const unsigned lo = min(nw, (unsigned)tid * per), hi = min(nw, lo + per);
  unsigned nff = 0;
  for (unsigned k = lo; k < hi; ++k) {
    const unsigned w = L.stage[k], nb = k < nwords ? 4u : tail;
    for (unsigned j = 0; j < nb; ++j) nff += ((w >> (24 - 8 * j)) & 255u) == 255u ? 1u : 0u;
  }
  unsigned totff;
  const unsigned ffbefore = block_excl_scan(nff, L.red, &totff);
  const unsigned rel = obytes & 3u;
  uint8_t* s2b = (uint8_t*)L.s2;
  unsigned o = rel + lo * 4u + ffbefore;
  for (unsigned k = lo; k < hi; ++k) {
    const unsigned w = L.stage[k], nb = k < nwords ? 4u : tail;
    for (unsigned j = 0; j < nb; ++j) {
      const unsigned byte = (w >> (24 - 8 * j)) & 255u;
      s2b[o++] = (uint8_t)byte;
      if (byte == 255u) s2b[o++] = 0;
    }
  }
  unsigned end = rel + nwords * 4u + tail + totff;
  if (marker >= 0) {
    if (tid == 0) { s2b[end] = 0xFF; s2b[end + 1] = (uint8_t)marker; }
    end += 2;
  }
  __syncthreads();
  const unsigned nd = end >> 2;
  unsigned* dst = slotw + (obytes >> 2);
  for (unsigned k = tid; k < nd; k += kThreads) dst[k] = L.s2[k];
  const unsigned cw = L.s2[nd];
  __syncthreads();
  if (tid == 0) L.s2[0] = cw;
  obytes = obytes - rel + end;
}

// kPass of the interval kernel: the codes from the Annex K tables, the symbol counts alone, the
// codes from the tables the Huffman kernel built in the image's scratch
constexpr int kPassStd = 0, kPassCount = 1, kPassOpt = 2;
// 4:2:0 chroma: every thread converts its share of the pass's chroma samples into LDS and a chroma
// unit reads its 64 from there (a chroma unit that converts its 256 pixels itself keeps its wave
// waiting: 8-9 % slower per encode)
constexpr int kChromaMcuWords = 33;  // Cb then Cr, 16 words each, and one word so that MCUs start on different banks

template <int kSub, int kPass>
__global__ __launch_bounds__(kThreads) void jpeg_interval_kernel(JpegArgs a) {
  __shared__ IntervalLds L;
  constexpr unsigned kUpm = (unsigned)units_per_mcu(kSub);  // units of an MCU, DCs carried between passes
  constexpr int kMcu = kSub == kSub420 ? 16 : 8;
  const int tid = threadIdx.x;
  const int iv = blockIdx.x, b = blockIdx.y;
  const JpegGeom& g = a.g;
  const int brow0 = iv * g.rr;
  const int rows = min(g.rr, g.bh - brow0);
  const unsigned nu = kUpm * (unsigned)g.bw * (unsigned)rows;  // units of the interval
  const uint8_t* img = a.img + (size_t)b * g.H * g.W * 3;
  uint8_t* sc = a.scratch + (size_t)b * g.scratch_image;
  unsigned* slotw = (unsigned*)(sc + (size_t)iv * g.cap);
  unsigned* hist = L.stage;  // the counting pass: [kHuffTables][256]
  static_assert(kHuffTables * 256 <= kStageWords, "the histograms fit the stage");

  if constexpr (kPass == kPassStd) {
    L.ac[0][tid] = kT.ac[0][tid];
    L.ac[1][tid] = kT.ac[1][tid];
    if (tid < 24) (&L.dc[0][0])[tid] = (&kT.dc[0][0])[tid];
  } else if constexpr (kPass == kPassOpt) {
    const HuffImage* hi = (const HuffImage*)(sc + g.off_huff);
    for (int t = 0; t < (kSub == kSubGray ? 1 : 2); ++t) {
      L.ac[t][tid] = hi->code[2 * t + 1][tid];
      if (tid < 12) L.dc[t][tid] = hi->code[2 * t][tid];
    }
  }
  if (tid < 128) {
    const unsigned q = quant_step(kT.baseq[tid >> 6][tid & 63], a.qscale);
    L.qr[tid >> 6][tid & 63] = ((1u << 20) + q - 1u) / q | (q >> 1) << 21;
  }
  for (int k = tid; k < kStageWords + 2; k += kThreads) L.stage[k] = 0;
  if (tid < (int)kUpm) L.dcs[tid] = 0;
  if (tid == 0) L.s2[0] = 0;
  __syncthreads();

  unsigned B0 = 0;      // bit position of stage[0] in the interval's stream, a multiple of 32
  unsigned tbits = 0;   // bits of the units before this pass
  unsigned obytes = 0;  // stuffed bytes written

  for (unsigned base = 0; base < nu; base += kThreads) {
    const unsigned u = base + (unsigned)tid;
    const bool valid = u < nu;
    const unsigned mcu = u / kUpm;
    const int k6 = (int)(u - kUpm * mcu);  // the unit's place in its MCU
    // 4:2:0: Y00 Y01 Y10 Y11 Cb Cr
    const int comp = kSub == kSub444 ? k6 : (kSub == kSubGray ? 0 : (k6 < 4 ? 0 : k6 - 3));
    const int tab = comp ? 1 : 0;
    // the unit of the same component before this one in scan order: that many units back
    const int back = kSub == kSub444 ? 3 : (kSub == kSubGray ? 1 : (k6 == 0 ? 3 : (k6 < 4 ? 1 : 6)));
    unsigned nzlo = 0, nzhi = 0;  // non-zero quantised coefficients by zigzag position
    int mydc = 0;
    // chroma samples (0..255, the 2x2 box (a + b + c + d + 2) >> 2 of the per-pixel values) of the
    // pass's MCUs, in the second stage, which is idle between flushes (its word 0 carries the
    // partial dword)
    uint8_t* chroma = (uint8_t*)(L.s2 + 1);
    const unsigned mcu_lo = base / kUpm;
    if constexpr (kSub == kSub420) {
      static_assert(((kThreads + 5) / 6 + 1) * kChromaMcuWords <= 2 * kStageWords, "the pass's chroma fits the stage");
      const unsigned nm = min((unsigned)g.bw * (unsigned)rows, (base + kThreads + kUpm - 1) / kUpm) - mcu_lo;
      for (unsigned i = (unsigned)tid; i < nm * 64u; i += kThreads) {
        const unsigned m = mcu_lo + (i >> 6), py = (i >> 3) & 7u, px = i & 7u;
        const unsigned brow = m / (unsigned)g.bw, bcol = m - brow * (unsigned)g.bw;
        const int y = (brow0 + (int)brow) * 16 + 2 * (int)py, x = (int)bcol * 16 + 2 * (int)px;
        const uint8_t* row0 = img + (size_t)min(y, g.H - 1) * g.W * 3;
        const uint8_t* row1 = img + (size_t)min(y + 1, g.H - 1) * g.W * 3;
        const int xa = min(x, g.W - 1) * 3, xb = min(x + 1, g.W - 1) * 3;
        int sb = 2, sr = 2;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const uint8_t* p = (q < 2 ? row0 : row1) + (q & 1 ? xb : xa);
          const int r = p[0], gg = p[1], bl = p[2];
          sb += (__mul24(-11059, r) + __mul24(-21709, gg) + __mul24(32768, bl) + (128 << 16) + 32767) >> 16;
          sr += (__mul24(32768, r) + __mul24(-27439, gg) + __mul24(-5329, bl) + (128 << 16) + 32767) >> 16;
        }
        uint8_t* dst = chroma + (i >> 6) * (kChromaMcuWords * 4) + (i & 63u);
        dst[0] = (uint8_t)(sb >> 2);
        dst[64] = (uint8_t)(sr >> 2);
      }
      __syncthreads();
    }

    // ---- colour, DCT, quantisation, zigzag: everything of one block-component in registers ----
    if (valid) {
      const unsigned brow = mcu / (unsigned)g.bw, bcol = mcu - brow * (unsigned)g.bw;
      int y0 = (brow0 + (int)brow) * kMcu, x0 = (int)bcol * kMcu;
      const int cr = comp == 0 ? 19595 : (comp == 1 ? -11059 : 32768);
      const int cg = comp == 0 ? 38470 : (comp == 1 ? -21709 : -27439);
      const int cb = comp == 0 ? 7471 : (comp == 1 ? 32768 : -5329);
      const int off = comp == 0 ? 32768 : (128 << 16) + 32767;
      int x[64];
      if (kSub == kSub420 && comp != 0) {
        const unsigned* src = (const unsigned*)chroma + (mcu - mcu_lo) * kChromaMcuWords + (comp - 1) * 16;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
          const unsigned v = src[w];
#pragma unroll
          for (int j = 0; j < 4; ++j) x[4 * w + j] = (int)((v >> (8 * j)) & 255u) - 128;
        }
      } else {
        if (kSub == kSub420) { y0 += (k6 >> 1) * 8; x0 += (k6 & 1) * 8; }
#pragma unroll
        for (int py = 0; py < 8; ++py) {
          const uint8_t* row = img + (size_t)min(y0 + py, g.H - 1) * g.W * 3;
#pragma unroll
          for (int px = 0; px < 8; ++px) {
            const uint8_t* p = row + min(x0 + px, g.W - 1) * 3;
            const int v = __mul24(cr, (int)p[0]) + __mul24(cg, (int)p[1]) + __mul24(cb, (int)p[2]) + off;
            x[py * 8 + px] = (v >> 16) - 128;
          }
        }
      }
#pragma unroll
      for (int y = 0; y < 8; ++y) dct8<1, 10>(x + y * 8);
#pragma unroll
      for (int c = 0; c < 8; ++c) dct8<8, 16>(x + c);
      // v = sign(f) ((|f| + q / 2) / q): |f| + q / 2 < 2^12, where n / q == (n ceil(2^20 / q)) >> 20
#define UPR_JQ(k, nat)                                                              \
  {                                                                                 \
    const int f = x[nat];                                                           \
    const unsigned qr = L.qr[tab][k];                                               \
    const unsigned m = (((unsigned)abs(f) + (qr >> 21)) * (qr & 0x1FFFFFu)) >> 20;  \
    const int v = f < 0 ? -(int)m : (int)m;                                         \
    if (k == 0) mydc = v;                                                           \
    else L.coef[k][tid] = (short)v;                                                 \
    if (k > 0 && k < 32) nzlo |= (m ? 1u : 0u) << (k & 31);                         \
    if (k >= 32) nzhi |= (m ? 1u : 0u) << (k & 31);                                 \
  }
      UPR_JQ(0, 0) UPR_JQ(1, 1) UPR_JQ(2, 8) UPR_JQ(3, 16) UPR_JQ(4, 9) UPR_JQ(5, 2) UPR_JQ(6, 3) UPR_JQ(7, 10)
      UPR_JQ(8, 17) UPR_JQ(9, 24) UPR_JQ(10, 32) UPR_JQ(11, 25) UPR_JQ(12, 18) UPR_JQ(13, 11) UPR_JQ(14, 4)
      UPR_JQ(15, 5) UPR_JQ(16, 12) UPR_JQ(17, 19) UPR_JQ(18, 26) UPR_JQ(19, 33) UPR_JQ(20, 40) UPR_JQ(21, 48)
      UPR_JQ(22, 41) UPR_JQ(23, 34) UPR_JQ(24, 27) UPR_JQ(25, 20) UPR_JQ(26, 13) UPR_JQ(27, 6) UPR_JQ(28, 7)
      UPR_JQ(29, 14) UPR_JQ(30, 21) UPR_JQ(31, 28) UPR_JQ(32, 35) UPR_JQ(33, 42) UPR_JQ(34, 49) UPR_JQ(35, 56)
      UPR_JQ(36, 57) UPR_JQ(37, 50) UPR_JQ(38, 43) UPR_JQ(39, 36) UPR_JQ(40, 29) UPR_JQ(41, 22) UPR_JQ(42, 15)
      UPR_JQ(43, 23) UPR_JQ(44, 30) UPR_JQ(45, 37) UPR_JQ(46, 44) UPR_JQ(47, 51) UPR_JQ(48, 58) UPR_JQ(49, 59)
      UPR_JQ(50, 52) UPR_JQ(51, 45) UPR_JQ(52, 38) UPR_JQ(53, 31) UPR_JQ(54, 39) UPR_JQ(55, 46) UPR_JQ(56, 53)
      UPR_JQ(57, 60) UPR_JQ(58, 61) UPR_JQ(59, 54) UPR_JQ(60, 47) UPR_JQ(61, 55) UPR_JQ(62, 62) UPR_JQ(63, 63)
#undef UPR_JQ
      L.dcs[tid + kUpm] = (short)mydc;
    }
    __syncthreads();

    const unsigned long long nz = (unsigned long long)nzhi << 32 | nzlo;
    if constexpr (kPass == kPassCount) {
      // ---- the symbols the coding pass will emit, counted per table ----
      if (valid) {
        const int dcd = mydc - (int)L.dcs[tid + kUpm - back];
        atomicAdd(&hist[(2 * tab) * 256 + (32 - __clz(abs(dcd)))], 1u);
        unsigned* ach = hist + (2 * tab + 1) * 256;
        unsigned prev = 0;
        for (unsigned long long m = nz; m; m &= m - 1) {
          const unsigned k = (unsigned)__ffsll((long long)m) - 1u;
          const unsigned run = k - prev - 1u;
          prev = k;
          const unsigned sz = 32u - (unsigned)__clz(abs((int)L.coef[k][tid]));
          if (run >> 4) atomicAdd(&ach[0xF0], run >> 4);
          atomicAdd(&ach[(run & 15u) << 4 | sz], 1u);
        }
        if (!(nz >> 63)) atomicAdd(&ach[0x00], 1u);
      }
      __syncthreads();
      if (tid < (int)kUpm) L.dcs[tid] = L.dcs[kThreads + tid];
      __syncthreads();
      continue;
    }

    // ---- the unit's bit length: DC difference against the unit of its component before it, the
    // AC (run, size) symbols from the mask of non-zero coefficients ----
    const unsigned zrl = L.ac[tab][0xF0], eob = L.ac[tab][0x00];
    int dcd = 0;
    unsigned len = 0;
    if (valid) {
      dcd = mydc - (int)L.dcs[tid + kUpm - back];
      const unsigned cat = 32u - (unsigned)__clz(abs(dcd));
      len = (L.dc[tab][cat] >> 16) + cat;
      unsigned prev = 0;
      for (unsigned long long m = nz; m; m &= m - 1) {
        const unsigned k = (unsigned)__ffsll((long long)m) - 1u;
        const unsigned run = k - prev - 1u;
        prev = k;
        const unsigned sz = 32u - (unsigned)__clz(abs((int)L.coef[k][tid]));
        len += (run >> 4) * (zrl >> 16) + (L.ac[tab][(run & 15u) << 4 | sz] >> 16) + sz;
      }
      if (!(nz >> 63)) len += eob >> 16;
    }
    unsigned total;
    const unsigned pos = tbits + block_excl_scan(len, L.red, &total);
    const unsigned tend = tbits + total;
    if (tid < (int)kUpm) L.dcs[tid] = L.dcs[kThreads + tid];  // read by everyone before the scan's barriers

    // ---- the codes, in rounds of one window: every unit that ends inside the window ORs its
    // words into the stage (units meet only in the words they share), the rest wait ----
    bool done = !valid;
    for (;;) {
      if (tid == 0) L.next = tend;
      __syncthreads();
      if (!done && pos + len - B0 <= kWindowBits) {
        done = true;
        unsigned wi = (pos - B0) >> 5, n = (pos - B0) & 31u;
        unsigned long long acc = 0;
        auto put = [&](unsigned code, unsigned bits) {  // n < 32 and bits <= 27 on entry
          acc = acc << bits | code;
          n += bits;
          if (n >= 32) { atomicOr(&L.stage[wi++], (unsigned)(acc >> (n - 32))); n -= 32; }
        };
        {
          const unsigned cat = 32u - (unsigned)__clz(abs(dcd));
          const unsigned c = L.dc[tab][cat];
          put((c & 0xFFFFu) << cat | ((unsigned)(dcd + (dcd >> 31)) & ((1u << cat) - 1u)), (c >> 16) + cat);
        }
        unsigned prev = 0;
        for (unsigned long long m = nz; m; m &= m - 1) {
          const unsigned k = (unsigned)__ffsll((long long)m) - 1u;
          unsigned run = k - prev - 1u;
          prev = k;
          for (; run > 15u; run -= 16u) put(zrl & 0xFFFFu, zrl >> 16);
          const int v = L.coef[k][tid];
          const unsigned sz = 32u - (unsigned)__clz(abs(v));
          const unsigned c = L.ac[tab][run << 4 | sz];
          put((c & 0xFFFFu) << sz | ((unsigned)(v + (v >> 31)) & ((1u << sz) - 1u)), (c >> 16) + sz);
        }
        if (!(nz >> 63)) put(eob & 0xFFFFu, eob >> 16);
        if (n) atomicOr(&L.stage[wi], (unsigned)(acc << (32 - n)));
      } else if (!done) {
        atomicMin(&L.next, pos);
      }
      __syncthreads();
      const unsigned upto = L.next;  // the stage holds every bit below it
      const unsigned nfull = (upto - B0) >> 5;
      flush_bytes(L, slotw, nfull, 0, -1, obytes);
      const unsigned cw = L.stage[nfull];
      __syncthreads();
      for (unsigned k = tid; k <= nfull; k += kThreads) L.stage[k] = 0;
      __syncthreads();
      if (tid == 0) L.stage[0] = cw;
      B0 += nfull * 32u;
      if (upto == tend) break;
    }
    tbits = tend;
    __syncthreads();
  }

  if constexpr (kPass == kPassCount) {
    uint32_t* freq = &((HuffImage*)(sc + g.off_huff))->freq[0][0];
    for (int k = tid; k < kHuffTables * 256; k += kThreads)
      if (hist[k]) atomicAdd(&freq[(k >> 8) * kHuffFreq + (k & 255)], hist[k]);
    return;
  }

  // ---- the last partial byte padded with 1-bits, the marker, the last partial dword ----
  const unsigned r = tbits - B0, r8 = (r + 7u) & ~7u;  // r < 32
  if (tid == 0 && r8 != r) L.stage[0] |= (0xFFFFFFFFu >> r) & ~(r8 == 32u ? 0u : 0xFFFFFFFFu >> r8);
  __syncthreads();
  flush_bytes(L, slotw, 0, r8 >> 3, iv == g.ni - 1 ? -1 : 0xD0 + (iv & 7), obytes);
  __syncthreads();
  if (tid == 0) {
    if (obytes & 3u) slotw[obytes >> 2] = L.s2[0];
    ((unsigned*)(sc + g.off_sizes))[iv] = obytes;
  }
}

__global__ __launch_bounds__(kThreads) void jpeg_zero_freq_kernel(JpegArgs a) {
  uint32_t* freq = &((HuffImage*)(a.scratch + (size_t)blockIdx.x * a.g.scratch_image + a.g.off_huff))->freq[0][0];
  for (int k = threadIdx.x; k < kHuffTables * kHuffFreq; k += kThreads) freq[k] = 0;
}

// ---- Huffman tables from symbol counts (Annex K.2 as libjpeg's jpeg_gen_optimal_table states
// it; DESIGN.md 4.6, tests/jpeg_modes_ref.py optimal_table) ---------------------------------------
struct HuffArgs {
  const uint32_t* freq;   // [kHuffFreq] per table, entry 256 ignored
  uint32_t* code;         // [256] per table, or null
  uint8_t* bits_vals;     // [kHuffPayload] per table
  int32_t* nvals;
  // bytes from one workgroup's first table to the next workgroup's, per array
  size_t freq_stride, code_stride, bits_vals_stride, nvals_stride;
  int tables;             // tables of one workgroup, at most 4: one wave each
  int total;              // tables in all
};

struct HuffLds {
  unsigned size[4][kHuffFreq + 3];   // code length of each entry as the merges leave it
  unsigned bits[4][34];              // codes per length 1..32
  unsigned start[4][18], first[4][18];  // per length 1..16: position in HUFFVAL and code of its first symbol
  int nvals[4];
};

// One wave per table; lane l owns entries l, l + 64, l + 128, l + 192 and lane 0 the reserved
// entry 256 as well, all in registers.  A merge step: every lane's two smallest keys (count << 9 |
// 256 - index: the smallest count, ties to the largest index), a butterfly of the pairs over the
// wave, then c2 merges into c1 and every entry of either tree gets one bit longer (the walk along
// both `others` chains, with the tree kept as a label per entry).  The counts are at most 2^22 + 1
// in all, so a key fits 32 bits and no code is longer than 32 bits before the limit.
__global__ __launch_bounds__(kThreads) void jpeg_huffman_kernel(HuffArgs a) {
  __shared__ HuffLds S;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int table = blockIdx.x * a.tables + w;
  const bool active = w < a.tables && table < a.total;
  const uint32_t* freq = (const uint32_t*)((const uint8_t*)a.freq + blockIdx.x * a.freq_stride) + w * kHuffFreq;
  unsigned f[5], grp[5], sz[5];
  unsigned long long tot = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f[j] = active ? freq[lane + 64 * j] : 0u;
    tot += f[j];
  }
#pragma unroll
  for (int d = 32; d; d >>= 1) tot += __shfl_xor(tot, d, 64);
  while (tot > kHuffScale) {
    tot = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f[j] = (f[j] >> 1) + (f[j] & 1u);  // (f + 1) >> 1
      tot += f[j];
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) tot += __shfl_xor(tot, d, 64);
  }
  f[4] = active && lane == 0 ? 1u : 0u;
#pragma unroll
  for (int j = 0; j < 5; ++j) { grp[j] = (unsigned)(lane + 64 * j); sz[j] = 0; }
  for (;;) {
    unsigned m1 = ~0u, m2 = ~0u;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const unsigned key = f[j] ? f[j] << 9 | (unsigned)(256 - (lane + 64 * j)) : ~0u;
      m2 = min(m2, max(m1, key));
      m1 = min(m1, key);
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) {
      const unsigned o1 = __shfl_xor(m1, d, 64), o2 = __shfl_xor(m2, d, 64);
      m2 = min(max(m1, o1), min(m2, o2));
      m1 = min(m1, o1);
    }
    if (m2 == ~0u) break;
    const unsigned c1 = 256u - (m1 & 511u), c2 = 256u - (m2 & 511u), sum = (m1 >> 9) + (m2 >> 9);
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const unsigned idx = (unsigned)(lane + 64 * j);
      if (idx == c1) f[j] = sum;
      if (idx == c2) f[j] = 0;
      if (grp[j] == c1 || grp[j] == c2) { grp[j] = c1; ++sz[j]; }
    }
  }
#pragma unroll
  for (int j = 0; j < 5; ++j)
    if (lane + 64 * j < kHuffFreq) S.size[w][lane + 64 * j] = sz[j];
  if (lane < 34) S.bits[w][lane] = 0;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 5; ++j)
    if (lane + 64 * j < kHuffFreq && sz[j]) atomicAdd(&S.bits[w][min(sz[j], 32u)], 1u);
  __syncthreads();
  if (lane == 0) {
    unsigned* bits = S.bits[w];
    // Figure K.3: no code longer than 16 bits
    for (int i = 32; i > 16; --i) {
      while (bits[i] > 0) {
        int j = i - 2;
        while (j > 0 && bits[j] == 0) --j;
        if (j == 0) break;  // no such tree comes out of the merges
        bits[i] -= 2; bits[i - 1] += 1; bits[j + 1] += 2; bits[j] -= 1;
      }
    }
    int i = 16;
    while (i > 0 && bits[i] == 0) --i;
    if (i) --bits[i];  // the reserved entry leaves: no symbol has the all-ones code
    unsigned code = 0, k = 0;
    for (int len = 1; len <= 16; ++len) {
      S.first[w][len] = code;
      S.start[w][len] = k;
      code = (code + bits[len]) << 1;
      k += bits[len];
    }
    S.start[w][17] = k;
    S.nvals[w] = (int)k;
  }
  __syncthreads();
  if (!active) return;
  uint32_t* code = a.code ? (uint32_t*)((uint8_t*)a.code + blockIdx.x * a.code_stride) + w * 256 : nullptr;
  uint8_t* bv = a.bits_vals + blockIdx.x * a.bits_vals_stride + w * kHuffPayload;
  const unsigned nvals = (unsigned)S.nvals[w];
  // HUFFVAL: the symbols by (length the merges gave them, symbol); the limit moved counts between
  // lengths, not symbols in this order
  unsigned rank[4] = {0, 0, 0, 0};
  for (int s = 0; s < 256; ++s) {
    const unsigned c = S.size[w][s];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      rank[j] += c && (c < sz[j] || (c == sz[j] && s < lane + 64 * j)) ? 1u : 0u;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int sym = lane + 64 * j;
    unsigned cl = 0;
    if (sz[j] && rank[j] < nvals) {
      int len = 1;
      while (len < 16 && rank[j] >= S.start[w][len + 1]) ++len;
      cl = (S.first[w][len] + rank[j] - S.start[w][len]) | (unsigned)len << 16;
      bv[16 + rank[j]] = (uint8_t)sym;
    }
    if (code) code[sym] = cl;
    if ((unsigned)sym >= nvals) bv[16 + sym] = 0;
  }
  if (lane < 16) bv[lane] = (uint8_t)S.bits[w][lane + 1];
  if (lane == 0) *(int32_t*)((uint8_t*)a.nvals + blockIdx.x * a.nvals_stride + w * 4) = (int)nvals;
}

// One workgroup per image: where each interval goes, the headers, EOI and the file's size.
__global__ __launch_bounds__(kThreads) void jpeg_layout_kernel(JpegArgs a) {
  __shared__ unsigned red[8];
  __shared__ uint8_t hdr[kHeadBytes + 3];
  const int tid = threadIdx.x, b = blockIdx.x;
  const JpegGeom& g = a.g;
  uint8_t* sc = a.scratch + (size_t)b * g.scratch_image;
  const unsigned* sizes = (const unsigned*)(sc + g.off_sizes);
  unsigned* offs = (unsigned*)(sc + g.off_offs);
  uint8_t* out = a.out + (size_t)b * a.out_stride;
  // each thread owns `per` consecutive intervals
  const int per = (g.ni + kThreads - 1) / kThreads;
  const int lo = min(g.ni, tid * per), hi = min(g.ni, lo + per);
  unsigned bytes = 0;
  for (int k = lo; k < hi; ++k) bytes += sizes[k];
  unsigned total;
  unsigned off = block_excl_scan(bytes, red, &total);
  for (int k = lo; k < hi; ++k) { offs[k] = off; off += sizes[k]; }
  // the header, segment by segment: p is where the next one starts, the same in every thread
  const bool gray = g.sub == kSubGray;
  const int ncomp = gray ? 1 : 3;
  int p = kSegApp0End;
  if (tid < kSegApp0End) hdr[tid] = kT.header[tid];  // SOI, APP0
  for (int c = 0; c < (gray ? 1 : 2); ++c, p += kSegDqt)
    if (tid < kSegDqt)
      hdr[p + tid] = tid < 5 ? kT.header[kSegApp0End + kSegDqt * c + tid]
                             : (uint8_t)quant_step(kT.baseq[c][tid - 5], a.qscale);
  {  // SOF0: P = 8, Y, X, Nf, then (id, H << 4 | V, Tq) per component
    const int n = 10 + 3 * ncomp;
    if (tid < n) {
      const int i = tid - 10, ci = i / 3, r = i - 3 * ci;
      const int v = tid == 0 ? 0xFF : tid == 1 ? 0xC0 : tid == 2 ? 0 : tid == 3 ? n - 2 : tid == 4 ? 8
                  : tid == 5 ? g.H >> 8 : tid == 6 ? g.H : tid == 7 ? g.W >> 8 : tid == 8 ? g.W : tid == 9 ? ncomp
                  : r == 0 ? ci + 1 : r == 1 ? (ci == 0 && g.sub == kSub420 ? 0x22 : 0x11) : (ci ? 1 : 0);
      hdr[p + tid] = (uint8_t)v;
    }
    p += n;
  }
  const HuffImage* hf = (const HuffImage*)(sc + g.off_huff);
  int std_off = kSegDht0;
  for (int t = 0; t < (gray ? 2 : 4); ++t) {  // DHT: Tc << 4 | Th, BITS, HUFFVAL
    const int n_std = t & 1 ? kSegDhtStdAc : kSegDhtStdDc;
    const int n = g.opt ? 21 + hf->nvals[t] : n_std;
    const uint8_t* src = g.opt ? hf->bits_vals[t] : kT.header + std_off + 5;
    for (int k = tid; k < n; k += kThreads)
      hdr[p + k] = k == 0 ? 0xFF : k == 1 ? 0xC4 : k == 2 ? (uint8_t)((n - 2) >> 8) : k == 3 ? (uint8_t)(n - 2)
                 : k == 4 ? (uint8_t)((t & 1) << 4 | t >> 1) : src[k - 5];
    p += n;
    std_off += n_std;
  }
  if (tid < 6) {  // DRI
    const unsigned ri = (unsigned)g.bw * (unsigned)g.rr;
    hdr[p + tid] = (uint8_t)(tid == 0 ? 0xFF : tid == 1 ? 0xDD : tid == 2 ? 0 : tid == 3 ? 4 : tid == 4 ? ri >> 8 : ri);
  }
  p += 6;
  {  // SOS: Ns, (id, Td << 4 | Ta) per component, Ss = 0, Se = 63, Ah Al = 0
    const int n = 8 + 2 * ncomp;
    if (tid < n) {
      const int i = tid - 5;
      const int v = tid == 0 ? 0xFF : tid == 1 ? 0xDA : tid == 2 ? 0 : tid == 3 ? n - 2 : tid == 4 ? ncomp
                  : i < 2 * ncomp ? (i & 1 ? (i >> 1 ? 0x11 : 0) : (i >> 1) + 1) : (tid == n - 2 ? 63 : 0);
      hdr[p + tid] = (uint8_t)v;
    }
    p += n;
  }
  __syncthreads();
  for (int k = tid; k < p; k += kThreads) out[k] = hdr[k];
  if (tid == 0) {
    out[(size_t)p + total] = 0xFF;
    out[(size_t)p + total + 1] = 0xD9;
    a.sizes[b] = (long long)p + total + 2;
    *(unsigned*)(sc + g.off_head) = (unsigned)p;
  }
}

__global__ __launch_bounds__(kThreads) void jpeg_gather_kernel(JpegArgs a) {
  const int iv = blockIdx.x, b = blockIdx.y;
  const JpegGeom& g = a.g;
  const uint8_t* sc = a.scratch + (size_t)b * g.scratch_image;
  const unsigned size = ((const unsigned*)(sc + g.off_sizes))[iv];
  const unsigned off = ((const unsigned*)(sc + g.off_offs))[iv];
  const uint8_t* src = sc + (size_t)iv * g.cap;
  uint8_t* dst = a.out + (size_t)b * a.out_stride + *(const unsigned*)(sc + g.off_head) + off;
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

int jpeg_bound(int H, int W, int restart_rows, int subsampling, int huffman, size_t* bytes_per_image,
               size_t* scratch_bytes) {
  JpegGeom g;
  const int rc = jpeg_geom(H, W, restart_rows, subsampling, huffman, &g);
  if (rc != kOk) return rc;
  if (bytes_per_image) *bytes_per_image = g.file_bound;
  if (scratch_bytes) *scratch_bytes = g.scratch_image;
  return kOk;
}

namespace {

template <int kSub>
void launch_intervals(const JpegArgs& a, int B, hipStream_t st) {
  const dim3 grid(a.g.ni, B);
  if (!a.g.opt) {
    jpeg_interval_kernel<kSub, kPassStd><<<grid, kThreads, 0, st>>>(a);
    return;
  }
  HuffImage* hi = (HuffImage*)(a.scratch + a.g.off_huff);
  HuffArgs h;
  h.freq = &hi->freq[0][0]; h.code = &hi->code[0][0]; h.bits_vals = &hi->bits_vals[0][0]; h.nvals = hi->nvals;
  h.freq_stride = h.code_stride = h.bits_vals_stride = h.nvals_stride = a.g.scratch_image;
  h.tables = kSub == kSubGray ? 2 : 4;
  h.total = B * h.tables;
  jpeg_zero_freq_kernel<<<dim3(B), kThreads, 0, st>>>(a);
  jpeg_interval_kernel<kSub, kPassCount><<<grid, kThreads, 0, st>>>(a);
  jpeg_huffman_kernel<<<dim3(B), kThreads, 0, st>>>(h);
  jpeg_interval_kernel<kSub, kPassOpt><<<grid, kThreads, 0, st>>>(a);
}

}  // namespace

int launch_jpeg_encode(const uint8_t* img, int B, int H, int W, int quality, int restart_rows, int subsampling,
                       int huffman, uint8_t* out, size_t out_stride, long long* sizes, uint8_t* scratch,
                       size_t scratch_bytes, hipStream_t st) {
  JpegArgs a;
  const int rc = jpeg_geom(H, W, restart_rows, subsampling, huffman, &a.g);
  if (rc != kOk) return rc;
  if (out_stride < a.g.file_bound) return kErrArg;
  if (scratch_bytes / (size_t)B < a.g.scratch_image) return kErrWorkspace;
  if (B > 65535) return kErrShape;
  a.img = img; a.scratch = scratch; a.out = out; a.sizes = sizes; a.out_stride = out_stride;
  a.qscale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  if (subsampling == kSub420) launch_intervals<kSub420>(a, B, st);
  else if (subsampling == kSubGray) launch_intervals<kSubGray>(a, B, st);
  else launch_intervals<kSub444>(a, B, st);
  jpeg_layout_kernel<<<dim3(B), kThreads, 0, st>>>(a);
  jpeg_gather_kernel<<<dim3(a.g.ni, B), kThreads, 0, st>>>(a);
  UPR_CHECK_HIP(hipGetLastError());
  return kOk;
}

int launch_jpeg_huffman_build(const uint32_t* freq, int n, uint8_t* bits_vals, int32_t* nvals, hipStream_t st) {
  HuffArgs h;
  h.freq = freq; h.code = nullptr; h.bits_vals = bits_vals; h.nvals = nvals;
  h.tables = 4;
  h.total = n;
  h.freq_stride = (size_t)h.tables * kHuffFreq * 4; h.code_stride = 0;
  h.bits_vals_stride = (size_t)h.tables * kHuffPayload; h.nvals_stride = (size_t)h.tables * 4;
  jpeg_huffman_kernel<<<dim3((n + h.tables - 1) / h.tables), kThreads, 0, st>>>(h);
  UPR_CHECK_HIP(hipGetLastError());
  return kOk;
}

}  // namespace upr
