// Illumination-weighted non-local means on the u8 pixels of an output file
// (gfx950), in the integer arithmetic include/upr.h states for upr_denoise_lut /
// upr_denoise_nlm_u8; a numpy restatement agrees with it byte for byte
// (tests/denoise_ref.py).
//
//  nlm_kernel<P>    one workgroup per tile of 32 rows x (64 - 2P) content pixels
//                   of one image.  The tile plus its halo of search + patch,
//                   clamped to the content rectangle (I~), is staged once in LDS
//                   as two dwords per pixel: the packed pixel and the sum of its
//                   squared channels, so that a squared difference is
//                   |a|^2 + |b|^2 - 2 a.b with one packed dot product.  A wave
//                   owns 8 rows and 64 columns, a lane one column: per search
//                   offset it forms the squared difference of its column once
//                   per row (8 + 2P rows), slides the column sum down the rows
//                   in registers, and adds the 2P neighbouring columns' sums by
//                   DPP wave shifts: the separable box sum, 1 + 2P / 8 squared
//                   differences per pixel and offset instead of (2P + 1)^2, with
//                   no barrier inside the offset loop.  The P outer lanes on
//                   either side only feed their neighbours.  The weight's index
//                   (d * lut) >> 20 needs no 64-bit product: it is below 256
//                   exactly when d <= dmax = (2^28 - 1) / lut, a per-pixel bound.
//                   The strength table is a kernel argument (one for the batch,
//                   upr_denoise_nlm_u8) or a row per image in device memory
//                   (upr_denoise_nlm_u8_luts): two instantiations per patch
//                   radius that differ in the one load that fills sLut.
//  nlm_bars_kernel  copies the pixels outside the content rectangle.
//  lut_rows_kernel  upr_denoise_lut_dev: a table per image from a device array of
//                   noise levels (upr_noise_sigma_u8, noise.hip), a thread per entry.
#include <algorithm>
#include <cmath>
#include <type_traits>

#include "upr_common.h"
#include "../../include/upr.h"

namespace upr {
namespace {

constexpr int kRows = 8;                  // rows of a wave
constexpr int kTileH = 4 * kRows;         // rows of a workgroup (4 waves)
constexpr int kMaxSearch = 10, kMaxPatch = 3;

// floor(4095 exp(-i / 32) + 0.5); entry 256 is the weight of every t >= 256
__device__ const uint16_t kExpW[257] = {
    4095, 3969, 3847, 3729, 3614, 3503, 3395, 3290, 3189, 3091, 2996, 2904, 2814, 2728, 2644, 2563,
    2484, 2407, 2333, 2261, 2192, 2124, 2059, 1996, 1934, 1875, 1817, 1761, 1707, 1655, 1604, 1554,
    1506, 1460, 1415, 1372, 1329, 1289, 1249, 1210, 1173, 1137, 1102, 1068, 1035, 1004, 973, 943,
    914, 886, 858, 832, 806, 782, 757, 734, 712, 690, 668, 648, 628, 609, 590, 572,
    554, 537, 521, 505, 489, 474, 459, 445, 432, 418, 405, 393, 381, 369, 358, 347,
    336, 326, 316, 306, 297, 288, 279, 270, 262, 254, 246, 238, 231, 224, 217, 210,
    204, 198, 192, 186, 180, 174, 169, 164, 159, 154, 149, 145, 140, 136, 132, 128,
    124, 120, 116, 113, 109, 106, 103, 99, 96, 93, 90, 88, 85, 82, 80, 77,
    75, 73, 70, 68, 66, 64, 62, 60, 58, 57, 55, 53, 52, 50, 48, 47,
    45, 44, 43, 41, 40, 39, 38, 37, 35, 34, 33, 32, 31, 30, 29, 28,
    28, 27, 26, 25, 24, 24, 23, 22, 21, 21, 20, 20, 19, 18, 18, 17,
    17, 16, 16, 15, 15, 14, 14, 13, 13, 13, 12, 12, 12, 11, 11, 10,
    10, 10, 10, 9, 9, 9, 8, 8, 8, 8, 7, 7, 7, 7, 7, 6,
    6, 6, 6, 6, 5, 5, 5, 5, 5, 5, 5, 4, 4, 4, 4, 4,
    4, 4, 4, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 2, 2, 2,
    2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1,
    0};

// the strength table of a launch: one for the whole batch, passed as a kernel argument (1 KB), or a
// row per image in device memory (upr_denoise_nlm_u8_luts)
struct NlmLut {
  uint32_t v[256];
  __device__ __forceinline__ uint32_t at(int, int i) const { return v[i]; }
};
struct NlmLutRows {
  const uint32_t* rows;  // [B,256]
  __device__ __forceinline__ uint32_t at(int b, int i) const { return rows[(size_t)b * 256 + i]; }
};

// sum over the three channels of a_c * b_c of two packed pixels (byte 3 is zero)
__device__ __forceinline__ uint32_t dot_rgb(uint32_t a, uint32_t b) {
  return __builtin_amdgcn_udot4(a, b, 0u, false);  // v_dot4_u32_u8
}

// the value of the lane one to the left / right in the wave (0 at the wave's ends): a DPP move on the
// vector pipe, where __shfl_up / __shfl_down would go through the LDS crossbar
__device__ __forceinline__ uint32_t from_left(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138 /* wave_shr:1 */, 0xF, 0xF, true);
}
__device__ __forceinline__ uint32_t from_right(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x130 /* wave_shl:1 */, 0xF, 0xF, true);
}

template <int P, typename Lut>
__global__ __launch_bounds__(256) void nlm_kernel(const uint8_t* __restrict__ src, const uint8_t* __restrict__ illu,
                                                  int istride, int H, int W, int top, int left, int nh, int nw, int S,
                                                  Lut lut, uint8_t* __restrict__ out) {
  extern __shared__ __align__(16) uint8_t smem[];
  constexpr int TW = 64 - 2 * P, NR = kRows + 2 * P;
  const int R = S + P;
  const int LW = 64 + 2 * S, LH = kTileH + 2 * R;
  uint2* tile = (uint2*)smem;                     // [LH][LW]: packed pixel, sum of its squared channels
  uint32_t* sExp = (uint32_t*)(tile + LH * LW);   // [257]
  uint32_t* sLut = sExp + 257;                    // [256]
  const int tid = threadIdx.x;
  const int b = blockIdx.z, ty0 = blockIdx.y * kTileH, tx0 = blockIdx.x * TW;
  const size_t img = (size_t)b * H * W;
  for (int i = tid; i < LH * LW; i += 256) {
    const int ly = i / LW, lx = i - ly * LW;
    const int cy = min(max(ty0 - R + ly, 0), nh - 1), cx = min(max(tx0 - R + lx, 0), nw - 1);
    const uint8_t* p = src + (img + (size_t)(top + cy) * W + (left + cx)) * 3;
    const uint32_t r = p[0], g = p[1], bl = p[2];
    tile[i] = make_uint2(r | g << 8 | bl << 16, r * r + g * g + bl * bl);
  }
  for (int i = tid; i < 257; i += 256) sExp[i] = kExpW[i];
  sLut[tid] = lut.at(b, tid);
  __syncthreads();

  const int lane = tid & 63, wv = tid >> 6;
  const int cx = tx0 - P + lane;        // the lane's column, content coordinates
  const int cy0 = ty0 + wv * kRows;     // the wave's first output row
  if (cy0 >= nh) return;                // (the whole wave)
  const uint2* own = tile + (wv * kRows + S) * LW + (lane + S);  // row -P of the wave, the lane's column
  uint32_t pp[NR], pn[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const uint2 v = own[r * LW];
    pp[r] = v.x;
    pn[r] = v.y;
  }
  const bool col_ok = cx >= 0 && cx < nw;
  uint32_t scale[kRows], dmax[kRows], sw[kRows], sr[kRows], sg[kRows], sb[kRows];
#pragma unroll
  for (int k = 0; k < kRows; ++k) {
    uint32_t L = 255;
    if (illu && col_ok && cy0 + k < nh)
      L = illu[(img + (size_t)(top + cy0 + k) * W + (left + cx)) * (size_t)istride];
    scale[k] = sLut[L];
    dmax[k] = scale[k] ? 0x0FFFFFFFu / scale[k] : 0xFFFFFFFFu;  // the largest d with d * scale < 2^28
    sw[k] = sr[k] = sg[k] = sb[k] = 0u;
  }

  for (int sy = -S; sy <= S; ++sy) {
    for (int sx = -S; sx <= S; ++sx) {
      const uint2* q = own + sy * LW + sx;
      const bool x_in = (unsigned)(cx + sx) < (unsigned)nw;
      uint32_t D[NR], qp[kRows];
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const uint2 v = q[r * LW];
        D[r] = pn[r] + v.y - 2u * dot_rgb(pp[r], v.x);
        if (r >= P && r < P + kRows) qp[r - P] = v.x;
      }
      uint32_t C = 0u;
#pragma unroll
      for (int r = 0; r < 2 * P; ++r) C += D[r];
#pragma unroll
      for (int k = 0; k < kRows; ++k) {
        C += D[k + 2 * P];
        uint32_t d = C, l = C, r = C;  // the column's sum over rows k - P .. k + P; now the 2P neighbouring columns'
#pragma unroll
        for (int o = 1; o <= P; ++o) {
          l = from_left(l);
          r = from_right(r);
          d += l + r;
        }
        C -= D[k];
        // t = (d * scale) >> 20 < 256 exactly when d <= dmax; the product then fits 32 bits
        const bool in = x_in && (unsigned)(cy0 + k + sy) < (unsigned)nh && d <= dmax[k];
        const uint32_t w = sExp[in ? (d * scale[k]) >> 20 : 256u];
        const uint32_t v = qp[k];
        sw[k] += w;
        sr[k] += __umul24(w, v & 255u);
        sg[k] += __umul24(w, (v >> 8) & 255u);
        sb[k] += __umul24(w, v >> 16);
      }
    }
  }

  if (lane < P || lane >= 64 - P || cx >= nw) return;
#pragma unroll
  for (int k = 0; k < kRows; ++k) {
    if (cy0 + k >= nh) break;
    uint8_t* o = out + (img + (size_t)(top + cy0 + k) * W + (left + cx)) * 3;
    const uint32_t den = 2u * sw[k];
    o[0] = (uint8_t)((2u * sr[k] + sw[k]) / den);
    o[1] = (uint8_t)((2u * sg[k] + sw[k]) / den);
    o[2] = (uint8_t)((2u * sb[k] + sw[k]) / den);
  }
}

__global__ __launch_bounds__(256) void nlm_bars_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ out,
                                                       size_t npix, int H, int W, int top, int left, int nh, int nw) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (size_t)gridDim.x * 256) {
    const int x = (int)(i % (size_t)W), y = (int)((i / (size_t)W) % (size_t)H);
    if (y >= top && y < top + nh && x >= left && x < left + nw) continue;
    out[3 * i] = src[3 * i];
    out[3 * i + 1] = src[3 * i + 1];
    out[3 * i + 2] = src[3 * i + 2];
  }
}

template <int P, typename Lut>
int launch_nlm(const uint8_t* src, const uint8_t* illu, int istride, int B, int H, int W, int top, int left, int nh,
               int nw, int S, const Lut& lut, uint8_t* out, hipStream_t st) {
  const int R = S + P;
  const size_t lds = (size_t)(kTileH + 2 * R) * (64 + 2 * S) * sizeof(uint2) + (257 + 256) * sizeof(uint32_t);
  hipLaunchKernelGGL((nlm_kernel<P, Lut>), dim3(cdiv(nw, 64 - 2 * P), cdiv(nh, kTileH), B), dim3(256), lds, st, src,
                     illu, istride, H, W, top, left, nh, nw, S, lut, out);
  UPR_CHECK_HIP(hipGetLastError());
  return kOk;
}

// both entry points: the checks, the bars, the kernel of the patch radius
template <typename Lut>
int run_nlm(const uint8_t* src_u8, const uint8_t* illu_u8, int illu_stride, int B, int H, int W, int top, int left,
            int nh, int nw, int search, int patch, const uint32_t* lut, uint8_t* out_u8, void* stream) {
  if (!src_u8 || !out_u8 || !lut || B < 1 || H < 1 || W < 1 || nh < 1 || nw < 1 || top < 0 || left < 0 ||
      top > H - nh || left > W - nw || search < 1 || search > kMaxSearch || patch < 1 || patch > kMaxPatch)
    return UPR_ERR_ARG;
  if (illu_u8 && illu_stride != 1 && illu_stride != 3) return UPR_ERR_ARG;
  if (B > 65535) return UPR_ERR_SHAPE;
  const size_t npix = (size_t)B * H * W;
  if (src_u8 < out_u8 + 3 * npix && out_u8 < src_u8 + 3 * npix) return UPR_ERR_ARG;  // out aliases src
  Lut table;
  if constexpr (std::is_same<Lut, NlmLut>::value)
    std::copy(lut, lut + 256, table.v);
  else
    table.rows = lut;
  hipStream_t st = (hipStream_t)stream;
  if (nh != H || nw != W) {
    const int blocks = (int)std::min<size_t>((npix + 255) / 256, 4096);
    hipLaunchKernelGGL(nlm_bars_kernel, dim3(blocks), dim3(256), 0, st, src_u8, out_u8, npix, H, W, top, left, nh, nw);
    UPR_CHECK_HIP(hipGetLastError());
  }
  switch (patch) {
    case 1: return launch_nlm<1>(src_u8, illu_u8, illu_stride, B, H, W, top, left, nh, nw, search, table, out_u8, st);
    case 2: return launch_nlm<2>(src_u8, illu_u8, illu_stride, B, H, W, top, left, nh, nw, search, table, out_u8, st);
    default: return launch_nlm<3>(src_u8, illu_u8, illu_stride, B, H, W, top, left, nh, nw, search, table, out_u8, st);
  }
}

// one entry of the strength table (upr_denoise_lut), host and device: fp64, one operation at a time
__host__ __device__ inline uint32_t lut_entry(double strength, int floor, int patch, int L) {
  const double n = (double)(3 * (2 * patch + 1) * (2 * patch + 1));
  const double h = strength * 255.0 / (double)(L > floor ? L : floor);
  const double h2 = h * h;
  if (h2 == 0.0) return 4294967295u;
  const double v = ::floor(1048576.0 * 32.0 / (n * h2) + 0.5);
  return v < 4294967295.0 ? (uint32_t)v : 4294967295u;
}

__global__ __launch_bounds__(256) void lut_rows_kernel(const double* __restrict__ sigma, double scale, int floor,
                                                       int patch, uint32_t* __restrict__ lut) {
  lut[(size_t)blockIdx.x * 256 + threadIdx.x] = lut_entry(scale * sigma[blockIdx.x], floor, patch, threadIdx.x);
}

}  // namespace
}  // namespace upr

using namespace upr;

extern "C" {

int upr_denoise_lut(double strength, int floor, int patch, uint32_t* lut) {
  if (!lut || !(strength >= 0.0) || !std::isfinite(strength) || floor < 1 || floor > 255 || patch < 1 ||
      patch > kMaxPatch)
    return UPR_ERR_ARG;
  for (int L = 0; L < 256; ++L) lut[L] = lut_entry(strength, floor, patch, L);
  return UPR_OK;
}

int upr_denoise_lut_dev(const double* sigma, int B, double scale, int floor, int patch, uint32_t* lut, void* stream) {
  if (!sigma || !lut || B < 1 || !(scale >= 0.0) || !std::isfinite(scale) || floor < 1 || floor > 255 || patch < 1 ||
      patch > kMaxPatch)
    return UPR_ERR_ARG;
  hipLaunchKernelGGL(lut_rows_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, sigma, scale, floor, patch, lut);
  UPR_CHECK_HIP(hipGetLastError());
  return UPR_OK;
}

int upr_denoise_nlm_u8(const uint8_t* src_u8, const uint8_t* illu_u8, int illu_stride, int B, int H, int W, int top,
                       int left, int nh, int nw, int search, int patch, const uint32_t* lut, uint8_t* out_u8,
                       void* stream) {
  return run_nlm<NlmLut>(src_u8, illu_u8, illu_stride, B, H, W, top, left, nh, nw, search, patch, lut, out_u8, stream);
}

int upr_denoise_nlm_u8_luts(const uint8_t* src_u8, const uint8_t* illu_u8, int illu_stride, int B, int H, int W,
                            int top, int left, int nh, int nw, int search, int patch, const uint32_t* luts,
                            uint8_t* out_u8, void* stream) {
  return run_nlm<NlmLutRows>(src_u8, illu_u8, illu_stride, B, H, W, top, left, nh, nw, search, patch, luts, out_u8,
                             stream);
}

}  // extern "C"
