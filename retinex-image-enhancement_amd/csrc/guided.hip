// Guided-filter restore of the letterboxed result to the source's size (gfx950):
// the fast guided filter of He & Sun 2015, per channel, in the arithmetic
// include/upr.h states for upr_guided_fit / upr_guided_apply (integer window
// sums, then fp64 one operation at a time: this unit is built with
// -ffp-contract=off, and a numpy restatement agrees with it bit for bit).
//
//  guided_ab_kernel     T x T content pixels of one channel per block (T = 32
//                       up to radius 8: less halo per pixel; 16 above): the u8
//                       guide / target window plus its halo of `radius` staged
//                       once in LDS (zero outside the content rectangle), the
//                       four integer sums separably (rows, then columns), then
//                       a and b of the pixel in fp64 -> scratch [B,2,3,nh,nw]
//  guided_mean_kernel   the clipped window mean of one a or b plane: tile plus
//                       halo in LDS, row sums in increasing x, column sums of
//                       those in increasing y (no running sums), / N -> ab
//  guided_apply_kernel  16 rows x 64 full-resolution pixels per block; the
//                       coefficients (and the map's bytes) that the tile's
//                       bilinear taps touch are staged once in LDS; a lane
//                       makes 4 consecutive pixels: 12 source bytes in, 12
//                       bytes out per destination, as 3 dwords where the
//                       address allows it.  The groups of a row start where
//                       the enhanced output's address is a multiple of 4, so
//                       that output always stores dwords, whatever W is.
#include <algorithm>
#include <cmath>

#include "upr_common.h"
#include "../../include/upr.h"

namespace upr {
namespace {

constexpr int kFitSmallRadius = 8;  // up to here the fit kernels take 32 x 32 tiles, above 16 x 16
constexpr int kApplyRows = 16, kApplyCols = 64;

__device__ __forceinline__ int window_count(int c, int n, int r) { return min(c + r, n - 1) - max(c - r, 0) + 1; }

template <int T>
__global__ __launch_bounds__(256) void guided_ab_kernel(const uint8_t* __restrict__ guide,
                                                        const uint8_t* __restrict__ target, int Hl, int Wl, int top,
                                                        int left, int nh, int nw, int r, double eps_s,
                                                        double* __restrict__ ws) {
  extern __shared__ __align__(16) uint8_t smem[];
  const int S = T + 2 * r;
  uint8_t* sI = smem;
  uint8_t* sP = smem + S * S;
  int4* hs = (int4*)(smem + ((2 * S * S + 15) & ~15));  // [S][T]: S_I, S_p, S_II, S_Ip of a row's window
  const int b = blockIdx.z / 3, c = blockIdx.z % 3;
  const int ty0 = blockIdx.y * T, tx0 = blockIdx.x * T;
  const size_t img = (size_t)b * Hl * Wl;
  for (int i = threadIdx.x; i < S * S; i += 256) {
    const int cy = ty0 - r + i / S, cx = tx0 - r + i % S;
    uint8_t vi = 0, vp = 0;
    if (cy >= 0 && cy < nh && cx >= 0 && cx < nw) {
      const size_t o = (img + (size_t)(top + cy) * Wl + (left + cx)) * 3 + c;
      vi = guide[o];
      vp = target[o];
    }
    sI[i] = vi;
    sP[i] = vp;
  }
  __syncthreads();
  for (int j = threadIdx.x; j < S * T; j += 256) {
    const int ly = j / T, col = j % T;
    const uint8_t* pi = sI + ly * S + col;
    const uint8_t* pp = sP + ly * S + col;
    int4 s = make_int4(0, 0, 0, 0);
    for (int d = 0; d <= 2 * r; ++d) {
      const int vi = pi[d], vp = pp[d];
      s.x += vi; s.y += vp; s.z += vi * vi; s.w += vi * vp;
    }
    hs[j] = s;
  }
  __syncthreads();
  for (int j = threadIdx.x; j < T * T; j += 256) {
    const int ty = j / T, tx = j % T;
    const int cy = ty0 + ty, cx = tx0 + tx;
    if (cy >= nh || cx >= nw) continue;
    int4 s = make_int4(0, 0, 0, 0);
    for (int d = 0; d <= 2 * r; ++d) {
      const int4 h = hs[(ty + d) * T + tx];
      s.x += h.x; s.y += h.y; s.z += h.z; s.w += h.w;
    }
    const long long N = (long long)window_count(cy, nh, r) * window_count(cx, nw, r);
    const long long SI = s.x, SP = s.y, SII = s.z, SIP = s.w;
    const double num = (double)(N * SIP - SI * SP);
    const double den = (double)(N * SII - SI * SI) + eps_s * (double)(N * N);
    const double a = num / den;
    const double bb = ((double)SP - a * (double)SI) / (double)N;
    const size_t plane = (size_t)nh * nw, o = (size_t)cy * nw + cx;
    ws[((size_t)b * 6 + c) * plane + o] = a;
    ws[((size_t)b * 6 + 3 + c) * plane + o] = bb;
  }
}

template <int T>
__global__ __launch_bounds__(256) void guided_mean_kernel(const double* __restrict__ ws, int nh, int nw, int r,
                                                          double* __restrict__ ab) {
  extern __shared__ __align__(16) uint8_t smem[];
  const int S = T + 2 * r;
  double* v = (double*)smem;  // [S][S]
  double* hs = v + S * S;     // [S][T]
  const size_t plane = (size_t)nh * nw;
  const double* in = ws + blockIdx.z * plane;
  const int ty0 = blockIdx.y * T, tx0 = blockIdx.x * T;
  for (int i = threadIdx.x; i < S * S; i += 256) {
    const int cy = ty0 - r + i / S, cx = tx0 - r + i % S;
    v[i] = (cy >= 0 && cy < nh && cx >= 0 && cx < nw) ? in[(size_t)cy * nw + cx] : 0.0;
  }
  __syncthreads();
  for (int j = threadIdx.x; j < S * T; j += 256) {
    const int ly = j / T, col = j % T;
    const int cy = ty0 - r + ly, cx = tx0 + col;
    double acc = 0.0;
    if (cy >= 0 && cy < nh && cx < nw) {
      const int lo = max(cx - r, 0), hi = min(cx + r, nw - 1);
      const double* row = v + ly * S - (tx0 - r);
      acc = row[lo];
      for (int x = lo + 1; x <= hi; ++x) acc = acc + row[x];
    }
    hs[j] = acc;
  }
  __syncthreads();
  for (int j = threadIdx.x; j < T * T; j += 256) {
    const int tx = j % T;
    const int cy = ty0 + j / T, cx = tx0 + tx;
    if (cy >= nh || cx >= nw) continue;
    const int lo = max(cy - r, 0), hi = min(cy + r, nh - 1);
    const double* colp = hs + tx - (ty0 - r) * T;
    double acc = colp[lo * T];
    for (int y = lo + 1; y <= hi; ++y) acc = acc + colp[y * T];
    const double N = (double)((long long)window_count(cy, nh, r) * window_count(cx, nw, r));
    ab[blockIdx.z * plane + (size_t)cy * nw + cx] = acc / N;
  }
}

// the bilinear taps of full-resolution coordinate t on an axis of n coefficients
__device__ __forceinline__ void taps(int t, double scale, int n, int& i0, int& i1, double& w) {
  double f = ((double)t + 0.5) * scale - 0.5;
  f = f < 0.0 ? 0.0 : f;
  const double top = (double)(n - 1);
  f = f > top ? top : f;
  const double fl = floor(f);
  i0 = (int)fl;
  i1 = min(i0 + 1, n - 1);
  w = f - fl;
}

__device__ __forceinline__ double bilerp(double m00, double m01, double m10, double m11, double wx, double wy) {
  return (1.0 - wy) * ((1.0 - wx) * m00 + wx * m01) + wy * ((1.0 - wx) * m10 + wx * m11);
}

__device__ __forceinline__ uint32_t round_u8(double v) {
  v = v < 0.0 ? 0.0 : v;
  v = v > 255.0 ? 255.0 : v;
  return (uint32_t)floor(v + 0.5);
}

// 12 bytes (4 RGB pixels, memory order) of which the pixels k0 .. k1 - 1 exist
__device__ __forceinline__ void put12(uint8_t* p, const uint32_t (&q)[12], int k0, int k1) {
  if (k0 == 0 && k1 == 4 && ((uintptr_t)p & 3) == 0) {
    uint32_t* d = (uint32_t*)p;
#pragma unroll
    for (int j = 0; j < 3; ++j) d[j] = q[4 * j] | q[4 * j + 1] << 8 | q[4 * j + 2] << 16 | q[4 * j + 3] << 24;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k >= k0 && k < k1) {
        p[3 * k] = (uint8_t)q[3 * k]; p[3 * k + 1] = (uint8_t)q[3 * k + 1]; p[3 * k + 2] = (uint8_t)q[3 * k + 2];
      }
  }
}

__global__ __launch_bounds__(256) void guided_apply_kernel(const uint8_t* __restrict__ src, size_t src_stride, int H,
                                                           int W, const double* __restrict__ ab,
                                                           const uint8_t* __restrict__ illu_lb, int Hl, int Wl, int top,
                                                           int left, int nh, int nw, double sy, double sx,
                                                           uint8_t* __restrict__ enh, uint8_t* __restrict__ illu,
                                                           uint8_t* __restrict__ cmp, int P, int LY, int LX) {
  extern __shared__ __align__(16) uint8_t smem[];
  double* cf = (double*)smem;                      // [6][LY][LX]
  uint8_t* il = smem + (size_t)6 * LY * LX * 8;    // [LY][LX]
  const int b = blockIdx.z;
  const int Ya = blockIdx.y * kApplyRows, Yb = min(Ya + kApplyRows - 1, H - 1);
  const int Xa = max((int)blockIdx.x * kApplyCols - 3, 0);
  const int Xb = min((int)blockIdx.x * kApplyCols + kApplyCols - 1, W - 1);
  int cy_lo, cy_hi, cx_lo, cx_hi, t;
  double w;
  taps(Ya, sy, nh, cy_lo, t, w);
  taps(Yb, sy, nh, t, cy_hi, w);
  taps(Xa, sx, nw, cx_lo, t, w);
  taps(Xb, sx, nw, t, cx_hi, w);
  const int ny = min(cy_hi - cy_lo + 1, LY), nx = min(cx_hi - cx_lo + 1, LX);  // (the host sized LY, LX to hold them)
  const size_t plane = (size_t)nh * nw;
  const int per = ny * nx;
  for (int i = threadIdx.x; i < 6 * per; i += 256) {
    const int m = i / per, j = i - m * per, ly = j / nx, lx = j - ly * nx;
    cf[(m * LY + ly) * LX + lx] = ab[((size_t)b * 6 + m) * plane + (size_t)(cy_lo + ly) * nw + (cx_lo + lx)];
  }
  const bool need_i = illu_lb != nullptr;
  if (need_i)
    for (int j = threadIdx.x; j < per; j += 256) {
      const int ly = j / nx, lx = j - ly * nx;
      il[ly * LX + lx] = illu_lb[(((size_t)b * Hl + top + cy_lo + ly) * Wl + (left + cx_lo + lx)) * 3];
    }
  __syncthreads();
  const int Y = Ya + (int)threadIdx.x / 16;
  if (Y >= H) return;
  const size_t q = ((size_t)b * H + Y) * W;  // the row's first pixel among the output's pixels
  const int Xg = (int)blockIdx.x * kApplyCols + 4 * ((int)threadIdx.x & 15) - (int)(q & 3);
  const int k0 = Xg < 0 ? -Xg : 0, k1 = min(4, W - Xg);
  if (k0 >= k1) return;
  int y0, y1;
  double wy;
  taps(Y, sy, nh, y0, y1, wy);
  const int r0 = min(y0 - cy_lo, LY - 1) * LX, r1 = min(y1 - cy_lo, LY - 1) * LX;
  // the group's 12 source bytes
  const uint8_t* sp = src + (size_t)b * src_stride + ((long long)Y * W + Xg) * 3;
  uint32_t s[12], e[12], iv[12];
  if (k0 == 0 && k1 == 4 && ((uintptr_t)sp & 3) == 0) {
    const uint32_t* d = (const uint32_t*)sp;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const uint32_t v = d[j];
      s[4 * j] = v & 255; s[4 * j + 1] = (v >> 8) & 255; s[4 * j + 2] = (v >> 16) & 255; s[4 * j + 3] = v >> 24;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int c = 0; c < 3; ++c) s[3 * k + c] = (k >= k0 && k < k1) ? sp[3 * k + c] : 0u;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    e[3 * k] = e[3 * k + 1] = e[3 * k + 2] = 0u;
    iv[3 * k] = iv[3 * k + 1] = iv[3 * k + 2] = 0u;
    if (k < k0 || k >= k1) continue;
    int x0, x1;
    double wx;
    taps(Xg + k, sx, nw, x0, x1, wx);
    const int c0 = min(x0 - cx_lo, LX - 1), c1 = min(x1 - cx_lo, LX - 1);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double* A = cf + c * LY * LX;
      const double* Bm = cf + (3 + c) * LY * LX;
      const double va = bilerp(A[r0 + c0], A[r0 + c1], A[r1 + c0], A[r1 + c1], wx, wy);
      const double vb = bilerp(Bm[r0 + c0], Bm[r0 + c1], Bm[r1 + c0], Bm[r1 + c1], wx, wy);
      e[3 * k + c] = round_u8(va * (double)s[3 * k + c] + vb);
    }
    if (need_i) {
      const double vi = bilerp((double)il[r0 + c0], (double)il[r0 + c1], (double)il[r1 + c0], (double)il[r1 + c1], wx,
                               wy);
      iv[3 * k] = iv[3 * k + 1] = iv[3 * k + 2] = (uint32_t)floor(vi + 0.5);
    }
  }
  const long long o = ((long long)q + Xg) * 3;
  put12(enh + o, e, k0, k1);
  if (illu) put12(illu + o, iv, k0, k1);
  if (cmp) {
    uint8_t* cr = cmp + ((long long)q * P + Xg) * 3;  // panel p of the row: + p * 3W
    put12(cr, s, k0, k1);
    put12(cr + (size_t)W * 3, e, k0, k1);
    if (P == 3) put12(cr + (size_t)W * 6, iv, k0, k1);
  }
}

template <int T>
int launch_fit(const uint8_t* guide, const uint8_t* target, int B, int Hl, int Wl, int top, int left, int nh, int nw,
               int r, double eps_s, double* ab, double* ws, hipStream_t st) {
  const int S = T + 2 * r;
  const dim3 tiles(cdiv(nw, T), cdiv(nh, T));
  const size_t lds_ab = ((2 * (size_t)S * S + 15) & ~(size_t)15) + (size_t)S * T * sizeof(int4);
  const size_t lds_mean = ((size_t)S * S + (size_t)S * T) * sizeof(double);
  hipLaunchKernelGGL(guided_ab_kernel<T>, dim3(tiles.x, tiles.y, B * 3), dim3(256), lds_ab, st, guide, target, Hl, Wl,
                     top, left, nh, nw, r, eps_s, ws);
  UPR_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(guided_mean_kernel<T>, dim3(tiles.x, tiles.y, B * 6), dim3(256), lds_mean, st, (const double*)ws,
                     nh, nw, r, ab);
  UPR_CHECK_HIP(hipGetLastError());
  return kOk;
}

size_t fit_ws(int B, int nh, int nw) { return (size_t)B * 6 * nh * nw * sizeof(double); }

bool content_ok(int Hl, int Wl, int top, int left, int nh, int nw) {
  return Hl > 0 && Wl > 0 && nh > 0 && nw > 0 && top >= 0 && left >= 0 && top <= Hl - nh && left <= Wl - nw;
}

}  // namespace
}  // namespace upr

using namespace upr;

extern "C" {

size_t upr_guided_fit_workspace(int B, int nh, int nw) {
  if (B < 1 || nh < 1 || nw < 1) return 0;
  return fit_ws(B, nh, nw);
}

int upr_guided_fit(const uint8_t* guide_u8, const uint8_t* target_u8, int B, int Hl, int Wl, int top, int left, int nh,
                   int nw, int radius, double eps, double* ab, void* workspace, size_t workspace_bytes, void* stream) {
  if (!guide_u8 || !target_u8 || !ab || !workspace || B < 1 || !content_ok(Hl, Wl, top, left, nh, nw) || radius < 1 ||
      radius > 32 || !(eps > 0.0))
    return UPR_ERR_ARG;
  if (B > 65535 / 6) return UPR_ERR_SHAPE;
  if (workspace_bytes < fit_ws(B, nh, nw)) return UPR_ERR_WORKSPACE;
  // the larger tile stages less halo per pixel; its LDS (doubles, (32 + 2r)^2 + 32 (32 + 2r)) fits for small radii
  return radius <= kFitSmallRadius
             ? launch_fit<32>(guide_u8, target_u8, B, Hl, Wl, top, left, nh, nw, radius, eps * 65025.0, ab,
                              (double*)workspace, (hipStream_t)stream)
             : launch_fit<16>(guide_u8, target_u8, B, Hl, Wl, top, left, nh, nw, radius, eps * 65025.0, ab,
                              (double*)workspace, (hipStream_t)stream);
}

int upr_guided_apply(const uint8_t* src_u8, size_t src_stride, int B, int H, int W, const double* ab,
                     const uint8_t* illu_lb_u8, int Hl, int Wl, int top, int left, int nh, int nw, uint8_t* enh_u8,
                     uint8_t* illu_u8, uint8_t* cmp_u8, int cmp_panels, void* stream) {
  if (!src_u8 || !ab || !enh_u8 || B < 1 || H < 1 || W < 1 || !content_ok(Hl, Wl, top, left, nh, nw))
    return UPR_ERR_ARG;
  if (illu_u8 && !illu_lb_u8) return UPR_ERR_ARG;
  if (cmp_u8 && ((cmp_panels != 2 && cmp_panels != 3) || (cmp_panels == 3 && !illu_lb_u8))) return UPR_ERR_ARG;
  if (src_stride < (size_t)H * W * 3) return UPR_ERR_ARG;
  if (nh > H || nw > W || B > 65535 || cdiv(H, kApplyRows) > 65535) return UPR_ERR_SHAPE;
  // coefficient rows / columns a tile's taps can touch: floor(f + d) - floor(f) <= ceil(d), + 1 for the
  // second tap, + 1 for the rounding of f
  const int LY = std::min(nh, (int)std::ceil((kApplyRows - 1) * (double)nh / (double)H) + 3);
  const int LX = std::min(nw, (int)std::ceil((kApplyCols + 2) * (double)nw / (double)W) + 3);
  const size_t lds = ((size_t)LY * LX * 49 + 15) & ~(size_t)15;
  const bool need_i = illu_u8 || (cmp_u8 && cmp_panels == 3);
  hipLaunchKernelGGL(guided_apply_kernel, dim3(cdiv(W + 3, kApplyCols), cdiv(H, kApplyRows), B), dim3(256), lds,
                     (hipStream_t)stream, src_u8, src_stride, H, W, ab, need_i ? illu_lb_u8 : nullptr, Hl, Wl, top,
                     left, nh, nw, (double)nh / (double)H, (double)nw / (double)W, enh_u8, illu_u8, cmp_u8,
                     cmp_u8 ? cmp_panels : 0, LY, LX);
  UPR_CHECK_HIP(hipGetLastError());
  return UPR_OK;
}

}  // extern "C"
