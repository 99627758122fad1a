// What the row-ring translation units share (conv_ring.hip: the fp16 programs
// and the 32-channel fp32 ones; conv_ring64.hip: the 64-channel fp32 program
// with the weights split once): the LDS ring's geometry and its per-lane DMA,
// the kernel argument block, the zero line and the write sinks, and the host
// side's row bands.  conv_ring.hip's header comment describes the structure.
#pragma once
#include <algorithm>

#include "upr_common.h"

namespace upr {

typedef __attribute__((address_space(3))) void* lds_void_ptr_r;

// zero 16-byte chunks for out-of-image pixels (16 chunks); a write sink for
// out-of-range outputs (128 bytes per thread, <= 512 threads; fp32 outputs: 256
// bytes per thread).  One copy per translation unit (no relocatable device code).
[[maybe_unused]] static __device__ __attribute__((aligned(256))) uint4 g_ring_zero[16];
[[maybe_unused]] static __device__ __attribute__((aligned(256))) uint2 g_ring_sink[512 * 16];
[[maybe_unused]] static __device__ __attribute__((aligned(256))) float g_ring_sink32[512 * 64];

// A ring of NPL chunk planes: NGRP (4) groups of GROWS rows of RW pixels.  DEINT:
// ring column p holds source column 2p (p < (RW+1)/2) or 2(p - (RW+1)/2) + 1.
// PLANE_ (bytes, 0 = dense): a padded plane stride.
template <int NPL, int RW_, int GROWS_, bool DEINT_ = false, int NGRP_ = 4, int PLANE_ = 0>
struct Ring {
  static constexpr int RW = RW_;
  static constexpr int GROWS = GROWS_;
  static constexpr int NGRP = NGRP_;
  static constexpr int RR = NGRP * GROWS;        // ring rows (a power of two with 4 groups)
  static constexpr int PLANE = PLANE_ ? PLANE_ : RR * RW * 16;  // bytes per chunk plane
  static constexpr int BYTES = NPL * PLANE;
  static constexpr int GPX = GROWS * RW;         // pixels per group
  static constexpr int NI = (GPX + 63) / 64;     // DMA instructions per plane per step
  static constexpr int PPW = NPL / 4;            // planes per wave
  static constexpr int G = NI * PPW;             // DMA instructions per wave per step
  static constexpr bool DEINT = DEINT_;
  static constexpr int HALF = (RW + 1) / 2;
  static_assert(NPL % 4 == 0, "planes are split over the 4 waves");
  static_assert(NGRP != 4 || (RR & (RR - 1)) == 0, "ring rows: power of two");
  static_assert(PLANE >= RR * RW * 16 && PLANE % 16 == 0, "a plane holds the ring's rows");
};

// Per-lane DMA geometry of one ring: for DMA instruction i the lane's group
// pixel (row dr, source column col) and its element offset (dr * W + col) * cs
// from the group origin; dr = -1 for the idle lanes of the last, partial
// instruction of a plane (exec-masked: they write nothing).
template <class R>
struct RingLanes {
  int dr[R::NI], col[R::NI], off[R::NI];
  __device__ __forceinline__ void init(int lane, int W, int cs) {
#pragma unroll
    for (int i = 0; i < R::NI; ++i) {
      const int q = i * 64 + lane;
      const int p = q % R::RW;
      dr[i] = q < R::GPX ? q / R::RW : -1;
      col[i] = R::DEINT ? (p < R::HALF ? 2 * p : 2 * (p - R::HALF) + 1) : p;
      off[i] = (dr[i] * W + col[i]) * cs;
    }
  }
  // DMA of one group: group pixel (dr, col) <- image pixel (iy0 + dr, ix0 +
  // col) of image b (fill outside the image or when !live)
  __device__ __forceinline__ void issue(const half_t* src, int cs, int b, int H, int W, int iy0, int ix0, bool live,
                                        const half_t* fill, unsigned char* ring, int grp, int wave) const {
    const half_t* base = src + ((long long)(b * H + iy0) * W + ix0) * cs;
#pragma unroll
    for (int i = 0; i < R::NI; ++i) {
      if (dr[i] >= 0) {
        const bool ok = live && (unsigned)(iy0 + dr[i]) < (unsigned)H && (unsigned)(ix0 + col[i]) < (unsigned)W;
        const half_t* p = ok ? base + off[i] : fill;
#pragma unroll
        for (int k = 0; k < R::PPW; ++k) {
          const int c = wave + 4 * k;
          __builtin_amdgcn_global_load_lds(p + c * 8, (lds_void_ptr_r)(ring + c * R::PLANE + grp * R::GPX * 16 + i * 1024),
                                           16, 0, 0);
        }
      }
    }
  }
};

struct RingArgs {
  ConvOp op;
  int nstrips, nseg, rs;  // strips per image row, row bands per image, rows per band (a multiple of the step's rows)
  int nunits, steps;      // units; steps per unit = rs / rows per step + 1 (first = DMA only)
};

inline int ring_cus() {
  static int cus = 0;
  if (!cus) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
      cus = 256;
  }
  return cus;
}

// row bands: minimise the makespan ceil(units / grid) * steps per unit (a step
// computes `rows` output rows)
inline void ring_bands(RingArgs& a, const ConvOp& op, int grid, int rows = 4) {
  const int per_band = op.B * a.nstrips;
  long best = -1;
  for (int nb = 1; nb <= 16; ++nb) {
    int rs = (cdiv(op.Ho, nb) + rows - 1) / rows * rows;
    if (rs < 8) rs = 8;
    const int nseg = cdiv(op.Ho, rs);
    const long cost = (long)cdiv(per_band * nseg, grid) * (rs / rows + 1);
    if (best < 0 || cost < best) {
      best = cost;
      a.rs = rs;
      a.nseg = nseg;
    }
  }
  a.nunits = per_band * a.nseg;
  a.steps = a.rs / rows + 1;
}

}  // namespace upr
