// Helpers shared by the fp16 wide-tile conv kernels (conv_wide.hip,
// conv_hw2.hip): LDS-DMA issue, XCD-aware tile order, compile-time loops and
// the direct-store epilogue of the operand-swapped MFMA tiles.
#pragma once
#include <utility>

#include "upr_common.h"

namespace upr {

typedef float f32x4_w __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8_w __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) void* lds_void_ptr;

constexpr int WBM = 256;  // output pixels per tile
constexpr int WBK = 64;   // channels per K step

__device__ __forceinline__ int wide_xcd_remap(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7;
  const int xcd = bid & 7, idx = bid >> 3;
  return ((xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

__device__ __forceinline__ void glds16(const void* g, unsigned char* lds) {
  __builtin_amdgcn_global_load_lds(g, (lds_void_ptr)lds, 16, 0, 0);
}

// the same DMA as a buffer load: a wave-uniform base read into SGPRs
// (readfirstlane) as a raw buffer descriptor + a per-lane 32-bit byte offset,
// so no DMA needs a 64-bit per-lane address.  (With 64-bit VGPR addresses --
// and even with global saddr + voffset, which hipcc widened back to 64-bit
// offsets -- it precomputed every step's addresses of the unrolled hwide4
// loop, spilled them, and each reload came with a vmcnt(0) wait that drained
// the DMA pipeline.)  The range check is disabled (all-ones record count):
// every offset is in bounds by construction.
__device__ __forceinline__ void glds16_s(const void* ubase, unsigned voff, unsigned char* lds) {
  const uint64_t b = (uint64_t)ubase;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)b);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32));
  void* sb = (void*)(((uint64_t)hi << 32) | lo);
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(sb, 0, (int)0xffffffff, 0x00020000);
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_void_ptr)lds, 16, voff, 0, 0, 0);
}


// Split-fp16 tensors (ConvOp::split_out): 8 channels of one pixel, hi at p, lo
// lo_off halfs further.  split_res_add: v += hi + lo * 2^-11 in fp32.
// split_store: writes both halves of the unrounded v (two 16-byte stores);
// returns true when a value is outside the fp16 range (|v| > 65504, inf, NaN).
__device__ __forceinline__ void split_res_add(float (&v)[8], const half_t* p, int lo_off) {
  const f16x8_w h = *(const f16x8_w*)p, l = *(const f16x8_w*)(p + lo_off);
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] += (float)h[e] + (float)l[e] * kSplitLoInv;
}
__device__ __forceinline__ bool split_store(half_t* p, int lo_off, const float (&v)[8]) {
  f16x8_w h, l;
  bool bad = false;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    h[e] = (half_t)v[e];
    l[e] = (half_t)((v[e] - (float)h[e]) * kSplitLoScale);
    bad = bad || !(__builtin_fabsf(v[e]) <= 65504.f);
  }
  *(f16x8_w*)p = h;
  *(f16x8_w*)(p + lo_off) = l;
  return bad;
}

template <typename F, int... S>
__device__ __forceinline__ void static_steps(F&& f, std::integer_sequence<int, S...>) {
  (f(std::integral_constant<int, S>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  static_steps(f, std::make_integer_sequence<int, N>{});
}

// Direct-store epilogue of conv_hwide4_kernel<DS = true> (no LDS parking, no
// block barriers).  The main loop ran the MFMAs with the operands swapped
// (weights first), so a lane's accumulator holds 4 consecutive CHANNELS of one
// pixel, and the B tile's rows were DMA'd in the order hw4_perm32 below, so
// tiles 2p / 2p + 1 of a lane hold channels 32p + 8fg + 0..3 / + 4..7 of pixel
// fr: 8 consecutive channels -> one 16-byte store per (fragment, pair), the
// scale / bias / residual / ReLU / out2 / pool arithmetic in registers.  The
// LDS epilogue parked 256 KiB of fp32 per block in 4 barrier-separated passes
// (~20% of the bottleneck conv, profiles/r3_hwide4_bneck_ablations_v2.txt).
__device__ __forceinline__ int hw4_perm32(int r) {
  // LDS row r of a 32-row group = (b' r4 | i3 r3 r2 | i1 r1 r0) holds channel i3*8 + b'*4 + i1
  return (r & ~31) | (((r >> 2) & 3) << 3) | (((r >> 4) & 1) << 2) | (r & 3);
}

// Shared by conv_hwide4_kernel<DS> and conv_wide_kernel<DS>: PIX(a) = the
// pixel (GEMM row) of the lane's fragment a, valid while < M; IMG >= 0: every
// pixel of the block is in image IMG (required for op.pool), else the image is
// divided out per fragment (only for the per-image bias).  PRE: the caller
// preloaded pair 0's residual rows into rv0 (hw4_res_load).  SPLIT: the op is
// an fp32 conv from split-fp16 operands (ConvOp::split_out / out_f32 /
// split_res); a kernel instance of its own, so the fp16 forms carry none of it.
template <int BN, int WM, int WN, int WAVES_M, bool PRE, bool SPLIT = false, typename PixF>
__device__ __forceinline__ void direct_epilogue(const ConvOp& op, f32x4_w (&acc)[WM][WN], int n0, int wm, int wn,
                                                int lane, const f16x8_w (&rv0)[WM], unsigned char* smem, PixF pix,
                                                int M, int HW, int IMG) {
  constexpr int NP = WN / 2;
  const int fr = lane & 15, fg = lane >> 4;
  const int cb = n0 + wn * WN * 16 + fg * 8;  // channel of pair p: cb + 32p
  const half_t* rpf = (const half_t*)(op.res1 ? op.res1 : op.res2);
  const int rcs = op.res1 ? op.res1_cs : op.res2_cs;
  // residual rows: pair 0's up front (or preloaded), pair p + 1's while pair p
  // is finished (each fragment's pair-p accumulators die as its pair-p + 1
  // residual arrives)
  f16x8_w rv[NP][WM];
  auto rload = [&](int p, int a) {
    const int m = pix(a);
    return m < M ? *(const f16x8_w*)(rpf + (size_t)m * rcs + cb + 32 * p) : f16x8_w{};
  };
  if constexpr (PRE) {
#pragma unroll
    for (int a = 0; a < WM; ++a) rv[0][a] = rv0[a];
  } else if (rpf) {
#pragma unroll
    for (int a = 0; a < WM; ++a) rv[0][a] = rload(0, a);
  }
  float psum[NP][8];
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int e = 0; e < 8; ++e) psum[p][e] = 0.f;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int c = cb + 32 * p;
    float sc[8], bi[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { sc[e] = 1.f; bi[e] = 0.f; }
    if (op.scale) {
      const f32x4_w s0 = *(const f32x4_w*)(op.scale + c), s1 = *(const f32x4_w*)(op.scale + c + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) { sc[e] = s0[e]; sc[e + 4] = s1[e]; }
    }
    if (op.bias) {
      const f32x4_w b0 = *(const f32x4_w*)(op.bias + c), b1 = *(const f32x4_w*)(op.bias + c + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) { bi[e] = b0[e]; bi[e + 4] = b1[e]; }
    }
    if (op.img_bias && IMG >= 0) {
#pragma unroll
      for (int e = 0; e < 8; ++e) bi[e] += op.img_bias[IMG * op.N + c + e];
    }
#pragma unroll
    for (int a = 0; a < WM; ++a) {
      const int mi = pix(a);
      const size_t m = (size_t)mi;
      float v[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] = acc[a][2 * p][e] * sc[e] + bi[e];
        v[e + 4] = acc[a][2 * p + 1][e] * sc[e + 4] + bi[e + 4];
      }
      if (rpf && p + 1 < NP) rv[p + 1][a] = rload(p + 1, a);
      if (mi >= M) continue;
      if (op.img_bias && IMG < 0) {
        const int im = mi / HW;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += op.img_bias[im * op.N + c + e];
      }
      if (SPLIT && op.split_res) {
        // split residual (one of res1 / res2): hi was prefetched into rv, lo is read here
        const f16x8_w l = *(const f16x8_w*)(rpf + m * rcs + op.N + c);
        if (op.res1) {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] += (float)rv[p][a][e] + (float)l[e] * kSplitLoInv;
        }
        if (op.relu) {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], 0.f);
        }
        if (!op.res1) {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] += (float)rv[p][a][e] + (float)l[e] * kSplitLoInv;
        }
      } else {
      if (op.res1) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += (float)rv[p][a][e];
      }
      if (op.relu) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], 0.f);
      }
      if (op.res2) {
        const f16x8_w r = op.res1 ? *(const f16x8_w*)((const half_t*)op.res2 + m * op.res2_cs + c) : rv[p][a];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += (float)r[e];
      }
      }
      if constexpr (SPLIT) {
        // the unrounded fp32 value: as hi / lo halves, or plain fp32 at the region's exit
        if (op.split_out) {
          if (split_store((half_t*)op.split_out + m * op.split_cs + c, op.split_lo, v) && op.ovf) *op.ovf = 1u;
        } else {
          float* d = op.out_f32 + m * op.out_f32_cs + c;
          *(f32x4_w*)d = f32x4_w{v[0], v[1], v[2], v[3]};
          *(f32x4_w*)(d + 4) = f32x4_w{v[4], v[5], v[6], v[7]};
        }
        continue;
      }
      f16x8_w o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = (half_t)v[e];
      if (op.out32) {
        // the training step's autocast convs (ConvOp::out32): the fp16-rounded
        // result in fp32 (+ res32), zeroed where mask16 <= 0, and its fp16 copy
        typedef _Float16 h4d __attribute__((ext_vector_type(4)));
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
          f32x4_w t;
#pragma unroll
          for (int e = 0; e < 4; ++e) t[e] = (float)o[hh * 4 + e];
          if (op.res32) t += *(const f32x4_w*)(op.res32 + m * op.res32_cs + c + hh * 4);
          if (op.mask16) {
            const h4d mk = *(const h4d*)((const half_t*)op.mask16 + m * op.mask16_cs + c + hh * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) t[e] = (float)mk[e] > 0.f ? t[e] : 0.f;
          }
          if (!op.skip32) *(f32x4_w*)(op.out32 + m * op.out32_cs + op.out32_coff + c + hh * 4) = t;
          if (op.out32_h16)
            *(h4d*)((half_t*)op.out32_h16 + m * op.out32_h16_cs + c + hh * 4) =
                h4d{(half_t)t[0], (half_t)t[1], (half_t)t[2], (half_t)t[3]};
        }
      } else {
        *(f16x8_w*)((half_t*)op.out + m * op.out_cs + op.out_coff + c) = o;
      }
      if (op.out2) {
        const f32x4_w s0 = *(const f32x4_w*)(op.pre2_scale + c), s1 = *(const f32x4_w*)(op.pre2_scale + c + 4);
        const f32x4_w h0 = *(const f32x4_w*)(op.pre2_shift + c), h1 = *(const f32x4_w*)(op.pre2_shift + c + 4);
        f16x8_w q;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          q[e] = (half_t)fmaxf(__builtin_fmaf((float)o[e], s0[e], h0[e]), 0.f);
          q[e + 4] = (half_t)fmaxf(__builtin_fmaf((float)o[e + 4], s1[e], h1[e]), 0.f);
        }
        *(f16x8_w*)((half_t*)op.out2 + m * op.out2_cs + c) = q;
      }
      if (op.pool) {
#pragma unroll
        for (int e = 0; e < 8; ++e) psum[p][e] += (float)o[e];
      }
    }
  }
  if (op.pool && IMG >= 0) {
    // per-lane partial sums -> LDS [16 fr][WAVES_M][BN] (the main loop is done
    // with LDS: the kernel waited for its DMAs and a barrier precedes this),
    // then one thread per channel adds its 16 * WAVES_M partials in a fixed
    // order and issues ONE fixed-point atomic: 256 coalesced atomics per block
    float* Ps = (float*)smem;
    const int cl = cb - n0;
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
      for (int e = 0; e < 8; ++e) Ps[(fr * WAVES_M + wm) * BN + cl + 32 * p + e] = psum[p][e];
    __syncthreads();
    const int tid = threadIdx.x;
    if (tid < BN) {
      float t = 0.f;
      for (int g = 0; g < 16 * WAVES_M; ++g) t += Ps[g * BN + tid];
      pool_add(op.pool, (size_t)IMG * op.N + n0 + tid, t);
    }
  }
}

template <int BN, int WM, int WN, int WAVES_M, int W, bool PRE = true>
__device__ __forceinline__ void hw4_direct_epilogue(const ConvOp& op, f32x4_w (&acc)[WM][WN], int m0, int n0,
                                                    int wm, int wn, int lane, const f16x8_w (&rv0)[WM],
                                                    unsigned char* smem) {
  constexpr int CW = W / WAVES_M, FPR = CW / 16;
  const int mb = m0 + CW * wm + (lane & 15);  // pixel of fragment a: mb + (a / FPR) * W + (a % FPR) * 16
  direct_epilogue<BN, WM, WN, WAVES_M, PRE>(
      op, acc, n0, wm, wn, lane, rv0, smem, [&](int a) { return mb + (a / FPR) * W + (a % FPR) * 16; }, 1 << 30,
      op.Ho * W, m0 / (op.Ho * W));
}

// pair-0 residual rows of a lane (see hw4_direct_epilogue), issued by the
// kernel after the DMAs of its second-to-last K step: the loads fly under the
// last 1.5 steps of MFMAs, and no counted vmcnt wait of the loop follows them
template <int WM, int WN, int WAVES_M, int W>
__device__ __forceinline__ void hw4_res_load(const ConvOp& op, f16x8_w (&rv0)[WM], int m0, int n0, int wm, int wn,
                                             int lane) {
  constexpr int CW = W / WAVES_M, FPR = CW / 16;
  const half_t* rpf = (const half_t*)(op.res1 ? op.res1 : op.res2);
  if (!rpf) return;
  const int rcs = op.res1 ? op.res1_cs : op.res2_cs;
  const int cb = n0 + wn * WN * 16 + (lane >> 4) * 8;
  const int mb = m0 + CW * wm + (lane & 15);
#pragma unroll
  for (int a = 0; a < WM; ++a) rv0[a] = *(const f16x8_w*)(rpf + (size_t)(mb + (a / FPR) * W + (a % FPR) * 16) * rcs + cb);
}

// the direct-store epilogue takes NHWC outputs with aligned channel runs:
// every inference op of the graph and the training step's autocast fp32
// outputs (out32 / res32 / mask16 / out32_h16)
inline bool hw4_ds_ok(const ConvOp& op) {
  if (op.store != kStoreNHWC) return false;
  if (op.out32) {
    if ((uintptr_t)op.out32 % 16 || op.out32_cs % 8 || op.out32_coff % 8) return false;
    if (op.res32 && ((uintptr_t)op.res32 % 16 || op.res32_cs % 8)) return false;
    if (op.mask16 && ((uintptr_t)op.mask16 % 8 || op.mask16_cs % 4)) return false;
    if (op.out32_h16 && ((uintptr_t)op.out32_h16 % 8 || op.out32_h16_cs % 4)) return false;
  } else if ((uintptr_t)op.out % 16 || op.out_cs % 8 || op.out_coff % 8) {
    return false;
  }
  if (op.res1 && ((uintptr_t)op.res1 % 16 || op.res1_cs % 8)) return false;
  if (op.res2 && ((uintptr_t)op.res2 % 16 || op.res2_cs % 8)) return false;
  if (op.out2 && op.out2_cs % 8) return false;
  if (((uintptr_t)op.scale | (uintptr_t)op.bias | (uintptr_t)op.pre2_scale | (uintptr_t)op.pre2_shift) % 16) return false;
  return true;
}

}  // namespace upr
