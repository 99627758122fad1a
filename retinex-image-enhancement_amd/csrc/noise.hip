// Blind noise level of a u8 image (gfx950): the Laplacian-difference estimator
// (Immerkaer, "Fast noise variance estimation", CVIU 1996) with a median in
// place of the mean, in the arithmetic include/upr.h states for
// upr_noise_sigma_u8; a numpy restatement agrees with it bit for bit
// (tests/noise_ref.py).  The mask [1 -2 1] x [1 -2 1] is separable:
//   a(y, x) = I(y, x-1) - 2 I(y, x) + I(y, x+1),  r = a(y-1, x) - 2 a(y, x) + a(y+1, x)
//
//  noise_hist_kernel  one workgroup per tile of 64 x 64 samples of one image.
//                     The tile and its one-pixel ring are staged once in LDS
//                     with aligned dword loads: a staged row keeps the byte
//                     offset (0..3) its first pixel has in global memory, so
//                     a row is copied dword for dword whatever W and left are
//                     (the up to 3 bytes before and after a row's span are
//                     copied along and never looked at).  A wave owns 16
//                     rows, a lane one column: it walks down its column with
//                     the last two rows' a and clipped flags in registers,
//                     reading 3 bytes per row and channel.  Counting: bins
//                     0..7 are private to the lane (registers, one compare
//                     and add each; a flat image puts every sample there, and
//                     64 LDS adds to one word would serialise) and reduced
//                     over the wave at the end; the others are LDS atomics.
//                     The tile's non-zero bins are added to the image's
//                     histogram with integer atomics: any order, same bits.
//  noise_fin_kernel   one workgroup per image: the median bin of the 2041
//                     counts and the three fp64 steps.
#include "upr_common.h"
#include "../../include/upr.h"

namespace upr {
namespace {

constexpr int kBins = 2041;      // |r| <= 2040
constexpr int kBinsPad = 2048;   // an image's counters in the workspace (the last 7 stay zero)
constexpr int kTile = 64;        // samples per tile side
constexpr int kWaveRows = kTile / 4;
constexpr int kPitch = 52;       // dwords of a staged row: 3 bytes of offset + 66 pixels of 3 bytes, rounded up
constexpr int kRegBins = 8;      // bins counted in registers
static_assert(3 + (kTile + 2) * 3 + 3 <= kPitch * 4, "a staged row fits its pitch");

__global__ __launch_bounds__(256) void noise_hist_kernel(const uint8_t* __restrict__ src, uint32_t* __restrict__ hist,
                                                         int H, int W, int top, int left, int nh, int nw) {
  __shared__ uint32_t sTile[(kTile + 2) * kPitch];
  __shared__ uint32_t sHist[kBinsPad];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int b = blockIdx.z;
  // the tile's first sample and its sample counts (content coordinates; samples are 1 .. n - 2)
  const int x0 = 1 + blockIdx.x * kTile, y0 = 1 + blockIdx.y * kTile;
  const int cols = min(kTile, nw - 1 - x0), rows = min(kTile, nh - 1 - y0);
  // staged row ry is content row y0 - 1 + ry, columns x0 - 1 .. x0 + cols
  const size_t first = (((size_t)b * H + (size_t)(top + y0 - 1)) * W + (size_t)(left + x0 - 1)) * 3;
  const uint8_t* p0 = src + first;
  const uint32_t a0 = (uint32_t)(uintptr_t)p0, pitch3 = (uint32_t)W * 3u;  // (only the two low bits matter)
  for (int i = tid; i < kBinsPad; i += 256) sHist[i] = 0u;
  for (int i = tid; i < (rows + 2) * kPitch; i += 256) {
    const int ry = i / kPitch, d = i - ry * kPitch;
    const uint8_t* p = p0 + (size_t)ry * W * 3;
    const uint32_t off = (uint32_t)(uintptr_t)p & 3u;
    if (d < (int)((off + (uint32_t)(cols + 2) * 3u + 3u) >> 2)) sTile[i] = ((const uint32_t*)(p - off))[d];
  }
  __syncthreads();

  const int r0 = wv * kWaveRows;                 // the wave's first sample row in the tile
  const int nr = min(kWaveRows, rows - r0);      // (wave-uniform; may be <= 0)
  uint32_t cnt[kRegBins];
#pragma unroll
  for (int j = 0; j < kRegBins; ++j) cnt[j] = 0u;
  if (nr > 0) {
    const uint8_t* t8 = (const uint8_t*)sTile;
    const bool col_ok = lane < cols;
    int am[3], ac[3];      // a of the rows above the sample and of the sample's
    bool fm[3], fc[3];     // whether one of their three values is 0 or 255
    auto row = [&](int ry, int c, int& a, bool& f) {
      const uint8_t* q = t8 + ry * (kPitch * 4) + ((a0 + (uint32_t)ry * pitch3) & 3u) + lane * 3 + c;
      const int l = q[0], m = q[3], r = q[6];
      a = l - 2 * m + r;
      f = (unsigned)(l - 1) >= 254u || (unsigned)(m - 1) >= 254u || (unsigned)(r - 1) >= 254u;
    };
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      row(r0, c, am[c], fm[c]);
      row(r0 + 1, c, ac[c], fc[c]);
    }
    for (int k = 0; k < nr; ++k) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        int an;
        bool fn;
        row(r0 + k + 2, c, an, fn);
        const int r = am[c] - 2 * ac[c] + an;
        const bool ok = col_ok && !(fm[c] || fc[c] || fn);
        const int m = r < 0 ? -r : r;
#pragma unroll
        for (int j = 0; j < kRegBins; ++j) cnt[j] += (ok && m == j) ? 1u : 0u;
        if (ok && m >= kRegBins) atomicAdd(&sHist[m], 1u);
        am[c] = ac[c];
        fm[c] = fc[c];
        ac[c] = an;
        fc[c] = fn;
      }
    }
#pragma unroll
    for (int j = 0; j < kRegBins; ++j) {
      uint32_t v = cnt[j];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      if (lane == 0 && v) atomicAdd(&sHist[j], v);
    }
  }
  __syncthreads();
  uint32_t* hb = hist + (size_t)b * kBinsPad;
  for (int i = tid; i < kBins; i += 256) {
    const uint32_t v = sHist[i];
    if (v) atomicAdd(&hb[i], v);
  }
}

__global__ __launch_bounds__(256) void noise_fin_kernel(const uint32_t* __restrict__ hist, double* __restrict__ sigma) {
  __shared__ uint32_t part[257];
  const int tid = threadIdx.x;
  const uint32_t* hb = hist + (size_t)blockIdx.x * kBinsPad;
  // 8 consecutive bins per thread (n < 2^31: 32-bit sums)
  const uint4 lo4 = ((const uint4*)hb)[2 * tid], hi4 = ((const uint4*)hb)[2 * tid + 1];
  const uint32_t v[8] = {lo4.x, lo4.y, lo4.z, lo4.w, hi4.x, hi4.y, hi4.z, hi4.w};
  uint32_t s = 0u;
#pragma unroll
  for (int k = 0; k < 8; ++k) s += v[k];
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    uint32_t run = 0u;
    for (int i = 0; i < 256; ++i) {
      const uint32_t t = part[i];
      part[i] = run;
      run += t;
    }
    part[256] = run;
  }
  __syncthreads();
  const unsigned long long n = part[256];
  if (n == 0) {
    if (tid == 0) sigma[blockIdx.x] = 0.0;
    return;
  }
  unsigned long long cum = part[tid];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const unsigned long long below = cum;
    cum += v[k];
    if (2 * cum >= n && 2 * below < n) {  // the smallest bin with 2 cum >= n: exactly one thread, once
      const int bin = tid * 8 + k;
      const double lo = bin ? (double)bin - 0.5 : 0.0, wd = bin ? 1.0 : 0.5;
      const double frac = (double)(n - 2 * below) / (double)(2ull * v[k]);
      const double med = lo + wd * frac;
      sigma[blockIdx.x] = med / 4.0469385011764905;  // 6 x the normal's 0.75 quantile
    }
  }
}

size_t noise_ws(int B) { return (size_t)B * kBinsPad * sizeof(uint32_t); }

}  // namespace
}  // namespace upr

using namespace upr;

extern "C" {

size_t upr_noise_sigma_workspace(int B) { return B < 1 ? 0 : noise_ws(B); }

int upr_noise_sigma_u8(const uint8_t* src_u8, int B, int H, int W, int top, int left, int nh, int nw, double* sigma,
                       void* workspace, size_t workspace_bytes, void* stream) {
  if (!src_u8 || !sigma || !workspace || B < 1 || H < 1 || W < 1 || nh < 1 || nw < 1 || top < 0 || left < 0 ||
      top > H - nh || left > W - nw || (uintptr_t)workspace % 16 != 0)
    return UPR_ERR_ARG;
  if (3ll * nh * nw >= (1ll << 31) || B > 65535 || cdiv(nh, kTile) > 65535) return UPR_ERR_SHAPE;
  if (workspace_bytes < noise_ws(B)) return UPR_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  uint32_t* hist = (uint32_t*)workspace;
  UPR_CHECK_HIP(hipMemsetAsync(hist, 0, noise_ws(B), st));
  if (nh >= 3 && nw >= 3) {
    hipLaunchKernelGGL(noise_hist_kernel, dim3(cdiv(nw - 2, kTile), cdiv(nh - 2, kTile), B), dim3(256), 0, st, src_u8,
                       hist, H, W, top, left, nh, nw);
    UPR_CHECK_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(noise_fin_kernel, dim3(B), dim3(256), 0, st, hist, sigma);
  UPR_CHECK_HIP(hipGetLastError());
  return UPR_OK;
}

}  // extern "C"
