// Row-ring streaming convolution for the fp32 64 -> 64 channel stride-1 3x3
// convs at half resolution (dec2.conv.0, dec2.conv.3, enc1.conv2 with its
// projecting shortcut) in the weights-split-once form (ConvOp::mma16 == kMma16WSplit):
// the structure of conv_ring.hip's fp32 ring (persistent blocks walking column
// strips top to bottom, every input row staged once by LDS-DMA, one barrier
// per step, constant vmcnt waits) with the arithmetic of conv_wide32.hip's
// weights-split-once tile kernel.  The tile kernel re-stages every input row
// once per tap (nine times the L2 -> LDS traffic); here the nine taps read it
// from LDS.
//
// * Step = 2 output rows x 32 pixels.  64 fp32 channels are 16 chunk planes
//   (256 bytes per pixel); a ring group is 2 rows of the 34-pixel strip.
// * Four waves = 2 rows x 2 halves of N.  A wave keeps (W_hi, W_lo) of its 32
//   output channels for all 18 K slices in registers (288), read as they
//   stand from split_pack.hip pack_split_w's blob, and accumulates hi W_hi + hi
//   W_lo and lo W_hi (two sets of 2 pixel groups x 2 tiles) on
//   v_mfma_f32_16x16x32_f16: 216 MFMAs per wave and step.
// * The activations are split once per ring element, in LDS, in the blob's
//   k-slot order (wsplit_kslot): a conversion item is the 8 channels 4g..4g+3,
//   16+4g..16+4g+3 of one 32-channel half ks of a pixel -- planes 8ks + g and
//   8ks + 4 + g -- and writes hi over the first plane, lo over the second.
//   Lane group fg of an MFMA then reads plane 8ks + fg (hi) and 8ks + 4 + fg
//   (lo) as ready operands, and its weight fragment is 16-byte chunk fg of
//   the blob's W_hi / W_lo run.  Two schedules, as in conv_ring.hip: top of the
//   step (4 groups, DMA two steps ahead, the landed group converted behind a
//   second barrier) and ahead (kW64Ahead: 5 groups, DMA three steps ahead, the
//   group the next step reads first converted beside this step's MFMAs).
// * Residual (kW64Res: added after the ReLU) and the shortcut's source pixels
//   (kW64Sc: 1x1 stride 2 over 32 channels, k rows 576..607) are LDS-DMA'd
//   into a per-wave landing zone at the top of the step.  The shortcut is a
//   register-fed nineteenth K slice: its fragments are split after the read.
// * Finish: (acc + acc2 2^-11) / s_n + bias, ReLU, residual; a non-finite
//   accumulator of a stored output sets ConvOp::ovf after the last step.
#include <cstdlib>

#include "ring_common.h"

namespace upr {

typedef float f32x4_w __attribute__((ext_vector_type(4)));

enum W64Flags : int { kW64Res = 1, kW64Sc = 2, kW64Ahead = 4 };
// the schedule ConvOp::ring_split == kRingSplitDefault takes
constexpr bool kW64DefaultAhead = true;

template <int FL>
struct RingW64Cfg {
  static constexpr bool RES = (FL & kW64Res) != 0, SC = (FL & kW64Sc) != 0, AHEAD = (FL & kW64Ahead) != 0;
  static constexpr int NGRP = AHEAD ? 5 : 4, LEAD = AHEAD ? 3 : 2;
  static constexpr int ROWS = 2;   // output rows per step
  static constexpr int NT = 2, NG = 2;  // 16-channel tiles / 16-pixel groups per wave
  static constexpr int NSL = 18;   // K slices of the 3x3 segment (tap, channel half)
  // every plane stride is a multiple of 256 bytes (the four lane groups of a
  // fragment read start on one bank row: conflict-free); 5 groups: 5440 -> 5632
  using RA = Ring<16, 34, ROWS, false, NGRP, AHEAD ? 5632 : 0>;
  static_assert(RA::PLANE % 256 == 0, "plane stride: whole bank rows");
  static constexpr int NCVI = 8 * RA::GPX;           // conversion items of a group
  static constexpr int NCV = (NCVI + 255) / 256;     // per thread
  // landing zone per wave: 32 pixels x 32 fp32 channels (its half of the
  // residual / the shortcut's source pixels), 128-byte rows
  static constexpr int EW = RES || SC ? 4096 : 0;
  static constexpr int E = RES || SC ? 4 : 0;
  static constexpr int LDS = RA::BYTES + 4 * EW;
  static constexpr int G = RA::G;
  static constexpr int S = NG * NT;
  // vmcnt waits at the top of step k (conv_ring.hip Ring32Cfg): younger than
  // the DMA that must have landed are stores(k-2), landing(k-1), one DMA, stores(k-1)
  static constexpr int W0 = G, W1 = E + G + S, WK = 2 * S + E + G;
  static_assert(WK <= 63, "vmcnt immediate");
  static_assert(!(RES && SC), "the shortcut program has no residual");
  static_assert(LDS <= 160 * 1024, "one block per CU");
};

template <int FL>
__global__ __launch_bounds__(256) void conv_ring32_kernel_w64(RingArgs a) {
  using K = RingW64Cfg<FL>;
  using RA = typename K::RA;
  constexpr int NT = K::NT, NG = K::NG, NSL = K::NSL;
  constexpr bool RES = K::RES, SC = K::SC;
  typedef f32x4_w f32x4;
  const ConvOp& op = a.op;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* ringA = smem;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wrow = wave & 1;  // output row of the step
  const int nh = wave >> 1;   // half of N: channels 32 nh .. 32 nh + 31
  const int fr = lane & 15, fg = lane >> 4;
  unsigned char* epi = smem + RA::BYTES + wave * K::EW;
  const int H = op.Ho, W = op.Wo;
  const ConvSeg& sa = op.seg[0];
  const int per_xcd = gridDim.x >> 3;
  const int v0 = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
  const int nu = v0 < a.nunits ? (a.nunits - 1 - v0) / (int)gridDim.x + 1 : 0;
  const int KT = nu * a.steps;

  // filter: lane (fr = n within the tile, fg) holds k-slots 8 fg .. 8 fg + 7 of
  // every 32-deep K step of its row: chunk fg of the W_hi run, chunk fg of W_lo
  f16x8_t wh[NSL][NT], wl[NSL][NT];
  f16x8_t wsh[SC ? NT : 1], wsl[SC ? NT : 1];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const half_t* row = (const half_t*)op.W + (size_t)(nh * 32 + nt * 16 + fr) * op.Kpad * 2 + fg * 8;
#pragma unroll
    for (int t = 0; t < NSL; ++t) {
      wh[t][nt] = *(const f16x8_t*)(row + t * 64);
      wl[t][nt] = *(const f16x8_t*)(row + t * 64 + 32);
    }
    if constexpr (SC) {
      wsh[nt] = *(const f16x8_t*)(row + NSL * 64);
      wsl[nt] = *(const f16x8_t*)(row + NSL * 64 + 32);
    }
  }
  // per accumulator row (channel 32 nh + 16 nt + 4 fg + i): 1 / s_n and the bias
  float sc[NT][4], bv[NT][4];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int n = nh * 32 + nt * 16 + fg * 4 + i;
      sc[nt][i] = op.scale[n];
      bv[nt][i] = op.bias ? op.bias[n] : 0.f;
    }
  const bool relu = op.relu != 0;

  const half_t* srcA = (const half_t*)((const float*)sa.src + sa.coff);  // element offsets in halves below
  const int csA = sa.cs * 2;                                           // pixel stride in halves
  const half_t* zero = (const half_t*)g_ring_zero;
  RingLanes<RA> la;
  la.init(lane, sa.Win, csA);

  auto unit_of = [&](int j, int& b, int& y0, int& x0) {
    const int u = v0 + j * (int)gridDim.x;
    const int sx = u % a.nstrips, r = u / a.nstrips;
    b = r / a.nseg;
    y0 = (r % a.nseg) * a.rs;
    x0 = sx * 32;
  };
  const int S = a.steps - 1;  // compute steps per unit (s = -1 is DMA only)
  struct Cursor {
    int j, s, b, y0, x0;
  };
  Cursor cc{0, -1, 0, 0, 0};
  if (nu > 0) unit_of(0, cc.b, cc.y0, cc.x0);
  Cursor dc = cc;
  auto advance = [&](Cursor& c) {
    if (++c.s == S) {
      c.s = -1;
      if (++c.j < nu) unit_of(c.j, c.b, c.y0, c.x0);
    }
  };
  // DMA of the two input rows step dc.s of its unit first needs, into group ga
  auto issue = [&](int ga) {
    la.issue(srcA, csA, dc.b, sa.Hin, sa.Win, dc.y0 + K::ROWS * dc.s + 1, dc.x0 - 1, dc.j < nu, zero, ringA, ga, wave);
    advance(dc);
  };
  // the lane's conversion items of a group: item q = (octet o = q / GPX, group
  // pixel q % GPX), o = 4 ks + g, at planes 8 ks + g and 8 ks + 4 + g
  // (consecutive lanes take consecutive pixels: conflict-free 16-byte accesses)
  int cvoff[K::NCV];
#pragma unroll
  for (int j = 0; j < K::NCV; ++j) {
    const int q = j * 256 + tid, o = q / RA::GPX;
    cvoff[j] = q < K::NCVI ? ((o >> 2) * 8 + (o & 3)) * RA::PLANE + (q % RA::GPX) * 16 : -1;
  }

  __syncthreads();  // the filter, scale and bias loads are behind the first DMA
  issue(1);
  issue(2);
  if constexpr (K::LEAD == 3) issue(3);

  float bad = 0.f;  // NaN once an accumulator was not finite (ConvOp::ovf, stored after the loop)
  const int abase = fg * RA::PLANE + fr * 16;  // plane fg (+ 8 ks: hi, + 4: lo), pixel fr of a ring row
  const int ocs = op.out_cs, rcs = RES ? op.res2_cs : 0;
  const float* resp = RES ? (const float*)op.res2 + nh * 32 : nullptr;
  const ConvSeg& ss = op.seg[SC ? 1 : 0];
  const float* scsrc = (const float*)ss.src + ss.coff;
  const int sccs = ss.cs, scH = ss.Hin, scW = ss.Win;
  const int eswz = (fr >> 1) & 7;  // chunk permutation of the lane's landing rows
  int gb = 0;                      // kk mod NGRP (ring of 5 groups)

  for (int kk = 0; kk < KT; ++kk) {
    // group of DMA(kk + d - 1), 0 <= d < NGRP; ring row (2 kk + c) mod RR, 0 <= c < 4
    auto grp_at = [&](int d) {
      if constexpr (K::NGRP == 4) return (kk + d) & 3;
      else return gb + d >= K::NGRP ? gb + d - K::NGRP : gb + d;
    };
    auto ring_row = [&](int c) {
      if constexpr (K::NGRP == 4) return (K::ROWS * kk + c) & (RA::RR - 1);
      else return K::ROWS * gb + c >= RA::RR ? K::ROWS * gb + c - RA::RR : K::ROWS * gb + c;
    };
    // this wave's conversion writes of the previous step are done before the barrier publishes them
    __builtin_amdgcn_s_waitcnt(0xC07F);
    if (kk == 0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(K::W0) : "memory");
    else if (kk == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(K::W1) : "memory");
    else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(K::WK) : "memory");
    __builtin_amdgcn_s_barrier();
    const int s = cc.s, b = cc.b, x0 = cc.x0;
    const int yend = min(H, cc.y0 + a.rs);
    const int y = cc.y0 + K::ROWS * s + wrow;
    const bool rowok = s >= 0 && y < yend;
    const size_t prow = (size_t)(b * H + (rowok ? y : 0)) * W + x0;  // first pixel of this wave's output row
    bool ovalid[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) ovalid[g] = rowok && x0 + g * 16 + fr < W;
    // landing zone: 32 px x 8 chunks, the chunks of pixel l XOR-permuted by (l >> 1) & 7
    // (conflict-free 16-byte reads of chunks c and 4 + c by the four lane groups)
    if constexpr (RES) {
#pragma unroll
      for (int i = 0; i < K::E; ++i) {
        const int q = i * 64 + lane, px = q >> 3;
        const bool ok = rowok && x0 + px < W;
        const void* p = ok ? (const void*)(resp + (prow + px) * rcs + ((q & 7) ^ ((px >> 1) & 7)) * 4) : (const void*)zero;
        __builtin_amdgcn_global_load_lds(p, (lds_void_ptr_r)(epi + i * 1024), 16, 0, 0);
      }
    }
    if constexpr (SC) {
      // the 1x1 stride-2 shortcut's source pixels (2y, 2x) of the row, 32 channels
#pragma unroll
      for (int i = 0; i < K::E; ++i) {
        const int q = i * 64 + lane, px = q >> 3;
        const bool ok = rowok && x0 + px < W;
        const void* p = ok ? (const void*)(scsrc + ((size_t)(b * scH + 2 * y) * scW + 2 * (x0 + px)) * sccs +
                                           ((q & 7) ^ ((px >> 1) & 7)) * 4)
                           : (const void*)zero;
        __builtin_amdgcn_global_load_lds(p, (lds_void_ptr_r)(epi + i * 1024), 16, 0, 0);
      }
    }
    issue(grp_at(K::LEAD + 1));

    // a group's conversion = reads of the lane's items (cv_read), then per item
    // split_f32x8 and hi -> the first plane, lo -> the second (cv_write: the
    // item's own 32 bytes, nothing another lane touches)
    f32x4 ct[K::NCV][2];
    auto cv_on = [&](int j) { return (j + 1) * 256 <= K::NCVI || cvoff[j] >= 0; };
    auto cv_read = [&](int grp) {
#pragma unroll
      for (int j = 0; j < K::NCV; ++j)
        if (cv_on(j)) {
          const unsigned char* p = ringA + grp * (RA::GPX * 16) + cvoff[j];
          ct[j][0] = *(const f32x4*)p;
          ct[j][1] = *(const f32x4*)(p + 4 * RA::PLANE);
        }
    };
    auto cv_write = [&](int grp, int j) {
      if (cv_on(j)) {
        unsigned char* p = ringA + grp * (RA::GPX * 16) + cvoff[j];
        const float v[8] = {ct[j][0][0], ct[j][0][1], ct[j][0][2], ct[j][0][3],
                            ct[j][1][0], ct[j][1][1], ct[j][1][2], ct[j][1][3]};
        f16x8_t hi, lo;
        split_f32x8(v, hi, lo);
        *(f16x8_t*)p = hi;
        *(f16x8_t*)(p + 4 * RA::PLANE) = lo;
      }
    };
    auto cv_group = [&](int grp) {  // one whole group, nothing overlapped
      cv_read(grp);
#pragma unroll
      for (int j = 0; j < K::NCV; ++j) cv_write(grp, j);
    };
    const int cvg = grp_at(K::AHEAD ? 2 : 1);  // the group this step converts
    if constexpr (K::AHEAD) {
      // DMA(kk + 1)'s group, which step kk + 1 reads first; its reads go out
      // here, the splits and writes ride with the MFMAs below.  Step 0 also
      // converts DMA(0)'s group (both have landed: W0)
      if (kk == 0) cv_group(1);
      cv_read(cvg);
    } else {
      // DMA(kk)'s group, published by a second barrier
      cv_group(cvg);
      __builtin_amdgcn_s_waitcnt(0xC07F);
      __builtin_amdgcn_s_barrier();
    }

    // acc = hi W_hi + hi W_lo, acc2 = lo W_hi (folded in with 2^-11 below)
    f32x4 acc[NT][NG], acc2[NT][NG];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        acc[nt][g] = f32x4{0.f, 0.f, 0.f, 0.f};
        acc2[nt][g] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    auto mm3 = [&](int g, const f16x8_t& xh, const f16x8_t& xl, const f16x8_t (&whi)[NT], const f16x8_t (&wlo)[NT]) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[nt][g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(whi[nt], xh, acc[nt][g], 0, 0, 0);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc2[nt][g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(whi[nt], xl, acc2[nt][g], 0, 0, 0);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[nt][g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wlo[nt], xh, acc[nt][g], 0, 0, 0);
    };
#define RING_FENCE __builtin_amdgcn_sched_barrier(0)
#define RING_LDS_DONE                                                               \
  do {                                                                              \
    RING_FENCE;                                                                     \
    __builtin_amdgcn_s_waitcnt(0xC07F); /* lgkmcnt(0); vmcnt / expcnt untouched */ \
    RING_FENCE;                                                                     \
  } while (0)
    if (s >= 0) {
      // chunk c = (tap row r, channel half ks, pixel group g): the three taps'
      // (hi, lo) fragments; [reads of chunk c + 1] [18 MFMAs of chunk c] [lgkmcnt(0)]
      constexpr int NCH = 12;
      f32x4 bx[2][3][2];
      auto ld = [&](int c, f32x4 (&x)[3][2]) {
        const int g = c & 1, ks = (c >> 1) & 1, r = c >> 2;
        const unsigned char* xr = ringA + abase + ring_row(wrow + r) * (RA::RW * 16) + ks * 8 * RA::PLANE + g * 256;
#pragma unroll
        for (int t = 0; t < 3; ++t) {
          x[t][0] = *(const f32x4*)(xr + t * 16);
          x[t][1] = *(const f32x4*)(xr + 4 * RA::PLANE + t * 16);
        }
      };
      auto mm = [&](int c, const f32x4 (&x)[3][2]) {
        const int g = c & 1, ks = (c >> 1) & 1, r = c >> 2;
#pragma unroll
        for (int t = 0; t < 3; ++t) {
          const int sl = (r * 3 + t) * 2 + ks;
          mm3(g, __builtin_bit_cast(f16x8_t, x[t][0]), __builtin_bit_cast(f16x8_t, x[t][1]), wh[sl], wl[sl]);
        }
      };
      ld(0, bx[0]);
      ld(1, bx[1]);
      RING_LDS_DONE;
      mm(0, bx[0]);
#pragma unroll
      for (int c = 1; c < NCH; ++c) {
        RING_FENCE;
        if (c + 1 < NCH) ld(c + 1, bx[(c + 1) & 1]);
        RING_FENCE;
        mm(c, bx[c & 1]);
        // converting ahead: one item beside each of the first chunks' MFMAs
        if (K::AHEAD && c <= K::NCV) cv_write(cvg, c - 1);
        RING_LDS_DONE;
      }
    }
#undef RING_LDS_DONE
#undef RING_FENCE
    if constexpr (K::AHEAD) {
      // a unit's DMA-only step has no MFMAs to hide the conversion behind
      if (s < 0) {
#pragma unroll
        for (int j = 0; j < K::NCV; ++j) cv_write(cvg, j);
      }
    }

    // this step's landing zone is filled (only the ring DMA issued after it is younger)
    if constexpr (K::E > 0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(K::G) : "memory");
    if constexpr (SC) {
      if (s >= 0) {
#pragma unroll
        for (int g = 0; g < NG; ++g) {
          const unsigned char* row = epi + (g * 16 + fr) * 128;
          const f32x4 x0v = *(const f32x4*)(row + ((fg ^ eswz) * 16));
          const f32x4 x1v = *(const f32x4*)(row + (((4 + fg) ^ eswz) * 16));
          const float v[8] = {x0v[0], x0v[1], x0v[2], x0v[3], x1v[0], x1v[1], x1v[2], x1v[3]};
          f16x8_t xh, xl;
          split_f32x8(v, xh, xl);
          mm3(g, xh, xl, wsh, wsl);
        }
      }
    }

    // finish: (acc + acc2 2^-11) / s_n + bias.  The range guard looks at the
    // unscaled sum (v * 0 is NaN exactly when v is not finite), before the ReLU
    // and the residual, which would hide a NaN or a -inf
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      float* dg = ovalid[g] ? (float*)op.out + (prow + g * 16 + fr) * ocs + op.out_coff + nh * 32 + fg * 4
                            : g_ring_sink32 + tid * 64;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        f32x4 v;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float u = __builtin_fmaf(acc2[nt][g][i], kSplitLoInv, acc[nt][g][i]);
          bad = __builtin_fmaf(ovalid[g] ? u : 0.f, 0.f, bad);  // stored outputs only
          v[i] = __builtin_fmaf(u, sc[nt][i], bv[nt][i]);
        }
        if (relu) {
#pragma unroll
          for (int i = 0; i < 4; ++i) v[i] = fmaxf(v[i], 0.f);
        }
        if constexpr (RES) v += *(const f32x4*)(epi + (g * 16 + fr) * 128 + (((nt * 4 + fg) ^ eswz) * 16));
        *(f32x4*)(dg + nt * 16) = v;
      }
    }
    advance(cc);
    if constexpr (K::NGRP != 4) gb = gb + 1 == K::NGRP ? 0 : gb + 1;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  // one plain store after the last step (the steps' vmcnt waits count every memory instruction)
  if (bad != bad && op.ovf) *op.ovf = 1u;
}

template <int FL>
static int launch_w64_cfg(const ConvOp& op, hipStream_t st) {
  using K = RingW64Cfg<FL>;
  auto kern = conv_ring32_kernel_w64<FL>;
  static int occ = 0;
  if (!occ) {
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, K::LDS);
    if (e != hipSuccess) return (int)e;
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void*)kern, 256, K::LDS);
    if (e != hipSuccess) return (int)e;
    if (occ < 1) occ = 1;
  }
  RingArgs a;
  a.op = op;
  a.nstrips = cdiv(op.Wo, 32);
  const int grid = ring_cus() * occ;  // a multiple of 8 (XCD-contiguous unit order)
  ring_bands(a, op, grid, K::ROWS);
  int g = std::min(grid, cdiv(a.nunits, 8) * 8);
  g = std::max(8, g / 8 * 8);
  hipLaunchKernelGGL(kern, dim3(g), dim3(256), K::LDS, st, a);
  return (int)hipGetLastError();
}

// ConvOp::ring_split picks the schedule as it does for the 32-channel programs
// (2: top of the step, 3: ahead; otherwise the one that measured faster)
template <int FL>
static int w64_form(const ConvOp& op, hipStream_t st) {
  const bool ahead = op.ring_split == kRingSplitAhead || (op.ring_split != kRingSplitTop && kW64DefaultAhead);
  return ahead ? launch_w64_cfg<FL | kW64Ahead>(op, st) : launch_w64_cfg<FL>(op, st);
}

// A weights-split-once op (ConvOp::mma16 == kMma16WSplit, already validated by
// launch_conv_wsplit) on the row ring: 3x3 stride 1 pad 1, 64 -> 64, NHWC, with
// ReLU / a residual after the ReLU / the 1x1 stride-2 shortcut segment over 32
// channels; kErrUnsupported for every other op
int launch_conv_ring_w64(const ConvOp& op, hipStream_t st) {
  if (op.mma16 != kMma16WSplit || !op.scale || !op.W || !op.out) return kErrUnsupported;
  if (op.Ho < 4 || op.Wo < 16 || op.N != 64 || op.store != kStoreNHWC) return kErrUnsupported;
  if (op.res1 || op.pool || op.img_bias || op.out2 || op.out32) return kErrUnsupported;
  if (op.out_cs % 4 || op.out_coff % 4 || (uintptr_t)op.out % 16 || (uintptr_t)op.W % 16) return kErrUnsupported;
  if (op.res2 && (op.res2_cs % 4 || (uintptr_t)op.res2 % 16)) return kErrUnsupported;
  const ConvSeg& s = op.seg[0];
  if (s.kh != 3 || s.kw != 3 || s.stride != 1 || s.dil != 1 || s.pad != 1 || s.pre != kPreNone || s.kbase != 0 ||
      s.C != 64 || s.cs % 4 || s.coff % 4 || (uintptr_t)s.src % 16 || s.Hin != op.Ho || s.Win != op.Wo)
    return kErrUnsupported;
  if ((long long)op.B * op.Ho * op.Wo > 0x7fffffffll / 64) return kErrUnsupported;  // as the tile kernel
  if (op.nseg == 2) {
    const ConvSeg& q = op.seg[1];
    if (op.res2 || op.Kpad != 608 || q.kh != 1 || q.kw != 1 || q.stride != 2 || q.pad != 0 || q.pre != kPreNone ||
        q.C != 32 || q.kbase != 576 || q.cs % 4 || q.coff % 4 || (uintptr_t)q.src % 16)
      return kErrUnsupported;
    if ((q.Hin - 1) / 2 + 1 != op.Ho || (q.Win - 1) / 2 + 1 != op.Wo) return kErrUnsupported;
    return w64_form<kW64Sc>(op, st);
  }
  if (op.nseg != 1 || op.Kpad != 576) return kErrUnsupported;
  return op.res2 ? w64_form<kW64Res>(op, st) : w64_form<0>(op, st);
}

}  // namespace upr
