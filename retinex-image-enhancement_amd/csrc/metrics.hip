// Image-quality metrics of the reference's utils/utils.py:95-333 (calculate_metrics,
// calculate_psnr, calculate_ssim, calculate_niqe, calculate_saturation,
// calculate_naturalness), per image of a batch, in two launches.
//
// metrics_tile_kernel: one 256-thread block per 16 x 32 tile of one image.  The
// tile's 26 x 42 region (a 5-pixel halo: the 11 x 11 SSIM window; the 7 x 7
// NIQE window's halo of 3 lies inside it) is loaded once with buffer loads
// (wave-uniform row offset, per-lane column offset; positions off the image
// read as 0 without a memory access, which is SSIM's zero border).  Every
// value stays in registers for the pointwise sums (channel sums, histogram,
// saturation, squared error) and goes through LDS for the windows:
//   NIQE   gray (fp32, op by op) -> 7-tap row sums of g and g*g (fp64, border
//          by scipy's `reflect` rule on the image index) -> 7-tap column sums
//   SSIM   per channel: the region of x and y (fp32) -> 11-tap row sums of x,
//          y, xx, yy, xy (fp64) -> 11-tap column sums -> the SSIM quotient
// Windows are separable and each thread takes 4 consecutive outputs of a row
// (2 of a column) from one window held in registers: the first is a direct
// sum, the next add the entering and subtract the leaving sample (at most
// three slides, so no drift to speak of).  The window means are never formed:
// the SSIM quotient and the NIQE variance are written in the window sums, so a
// pixel costs one fp64 division per channel instead of six.  Each block writes
// its fp64 partial sums to the workspace; the histogram goes through per-wave
// LDS histograms and integer atomics.  Nothing in a tile depends on the
// image's position in the batch.
//
// metrics_fin_kernel: one block per image adds the tile partials in a fixed
// order and forms the nine metrics.
//
// Built with -ffp-contract=off: the gray, gray^2 and saturation steps round
// operation by operation in float32, as the reference's numpy expressions do.
#include <cfloat>

#include "upr_common.h"

namespace upr {

constexpr int MT_TH = 16, MT_TW = 32;     // tile rows, columns
constexpr int MT_HALO = 5;                // SSIM window radius
constexpr int MT_RH = MT_TH + 2 * MT_HALO;  // 26 region rows
constexpr int MT_RW = MT_TW + 2 * MT_HALO;  // 42 region columns
constexpr int MT_RP = MT_RW + 1;          // padded region row (floats)
constexpr int MT_NQ = 3;                  // NIQE window radius
constexpr int MT_NROWS = MT_TH + 2 * MT_NQ;  // 22 rows of NIQE row sums
constexpr int MT_NT = 256;
constexpr int MT_LR = (MT_RH + 3) / 4;    // 7 region rows per wave
constexpr int MT_CO = MT_TH * MT_TW / MT_NT;  // 2 column-pass outputs per thread
// a row of row sums, padded: the row pass's 16-byte stores of two adjacent
// rows (one 16-lane group) then fall on different banks
constexpr int MT_SP = MT_TW + 2;
constexpr int kMetricsNSums = 14;         // (UPR_METRICS_NSUMS)
constexpr int kMetricsN = 9;              // (UPR_METRICS_N)
// sums: 0-2 sum x per channel, 3-5 sum x^2 per channel, 6 saturation, 7 sigma,
// 8 mu, 9 mu^2, 10 squared error, 11-13 SSIM per channel (10-13 written as 0 without ref)
static_assert(MT_RW <= 64, "one lane per region column");
static_assert(MT_CO * MT_NT == MT_TH * MT_TW && MT_TW % 4 == 0, "thread maps");

template <typename T>
__device__ __forceinline__ float mt_bload(__amdgpu_buffer_rsrc_t rs, int voff, int soff) {
  if constexpr (sizeof(T) == 4) {
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, voff, soff, 0));
  } else {
    const unsigned short h = __builtin_amdgcn_raw_buffer_load_b16(rs, voff, soff, 0);
    return (float)__builtin_bit_cast(_Float16, h);
  }
}

// scipy.ndimage `reflect` (d c b a | a b c d) on an image index, one reflection
__device__ __forceinline__ int mt_reflect(int i, int n) { return i < 0 ? -1 - i : (i >= n ? 2 * n - 1 - i : i); }
__device__ __forceinline__ int mt_clampi(int i, int lo, int hi) { return i < lo ? lo : (i > hi ? hi : i); }

template <typename T, bool PAIRED>
__global__ __launch_bounds__(MT_NT, 2) void metrics_tile_kernel(const T* __restrict__ enh, const T* __restrict__ ref,
                                                              double* __restrict__ part, int* __restrict__ hist,
                                                              int H, int W, int tiles_x, int ntiles) {
  __shared__ float G[MT_RH][MT_RP];                  // gray of the region (0 off the image)
  __shared__ float PX[MT_RH][MT_RP], PY[MT_RH][MT_RP];  // one channel of enh / ref
  // row sums: SSIM [5][26][34], NIQE [2][22][34]; at the end the block's sums [NS][256]
  constexpr int NS = PAIRED ? kMetricsNSums : 10;
  constexpr int ROWS_H = PAIRED ? MT_RH : MT_NROWS, ROWS_Q = PAIRED ? 5 : 2;
  constexpr int ROWS_D = ROWS_Q * ROWS_H * MT_SP > NS * MT_NT ? ROWS_Q * ROWS_H * MT_SP : NS * MT_NT;
  __shared__ __attribute__((aligned(16))) double rowsbuf[ROWS_D];
  __shared__ int wh[4][256];
  double(*rows)[ROWS_H][MT_SP] = (double(*)[ROWS_H][MT_SP])rowsbuf;
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int b = blockIdx.y, tile = blockIdx.x;
  const int ty0 = (tile / tiles_x) * MT_TH, tx0 = (tile % tiles_x) * MT_TW;
  const int HW = H * W;
  const int ib = 3 * HW * (int)sizeof(T);
  const __amdgpu_buffer_rsrc_t rsx =
      __builtin_amdgcn_make_buffer_rsrc((void*)(enh + (size_t)b * 3 * HW), 0, ib, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsy =
      __builtin_amdgcn_make_buffer_rsrc((void*)((PAIRED ? ref : enh) + (size_t)b * 3 * HW), 0, ib, 0x00020000);
  constexpr int kOff = 0x40000000;  // past any image: the load returns 0

#pragma unroll
  for (int k = 0; k < 4; ++k) wh[k][t] = 0;

  // (1) the region: wave w takes region rows w, w + 4, ...; lane l column l
  const int gx = tx0 - MT_HALO + lane;
  const bool xin = lane < MT_RW && gx >= 0 && gx < W;
  const int vcol = xin ? gx * (int)sizeof(T) : kOff;
  float xv[MT_LR][3], yv[MT_LR][3];
#pragma unroll
  for (int k = 0; k < MT_LR; ++k) {
    const int ry = wave + 4 * k;
    const int gy = ty0 - MT_HALO + ry;
    const bool yin = ry < MT_RH && gy >= 0 && gy < H;  // (wave-uniform)
    const int voff = yin ? vcol : kOff;
    const int ro = yin ? gy * W : 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int so = (c * HW + ro) * (int)sizeof(T);
      xv[k][c] = mt_bload<T>(rsx, voff, so);
      if constexpr (PAIRED) yv[k][c] = mt_bload<T>(rsy, voff, so);
    }
  }
  __syncthreads();  // (the histogram is zeroed)

  double acc[kMetricsNSums];
#pragma unroll
  for (int k = 0; k < kMetricsNSums; ++k) acc[k] = 0.0;

  // pointwise sums of the tile's own pixels, gray of the whole region
#pragma unroll
  for (int k = 0; k < MT_LR; ++k) {
    const int ry = wave + 4 * k;
    if (ry < MT_RH && lane < MT_RW) {
      const float r = xv[k][0], g = xv[k][1], bl = xv[k][2];
      G[ry][lane] = (0.299f * r + 0.587f * g) + 0.114f * bl;
      const int gy = ty0 - MT_HALO + ry;
      const bool own = ry >= MT_HALO && ry < MT_HALO + MT_TH && lane >= MT_HALO && lane < MT_HALO + MT_TW && gy < H &&
                       gx < W;  // (gy, gx >= 0 here)
      if (own) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float v = xv[k][c];
          const double d = (double)v;
          acc[c] += d;
          acc[3 + c] += d * d;
          // np.histogram(bins=256, range=(0, 1)): NaN and values outside [0, 1] are dropped
          if (v >= 0.f && v <= 1.f) {
            const int bin = (int)(v * 256.f);
            atomicAdd(&wh[wave][bin > 255 ? 255 : bin], 1);
          }
          if constexpr (PAIRED) {
            const double e = d - (double)yv[k][c];
            acc[10] += e * e;
          }
        }
        const float mx = fmaxf(fmaxf(r, g), bl), mn = fminf(fminf(r, g), bl);
        const float sat = mx > 1e-8f ? (mx - mn) / mx : 0.f;
        acc[6] += (double)sat;
      }
    }
  }
  __syncthreads();

  // (2) NIQE rows: item = (row j of 22 = image row ty0 - 3 + j, quad of 4 tile columns)
  for (int it = t; it < MT_NROWS * (MT_TW / 4); it += MT_NT) {
    const int j = it / (MT_TW / 4), x0 = (it % (MT_TW / 4)) * 4;
    const int rr = mt_clampi(mt_reflect(ty0 - MT_NQ + j, H) - (ty0 - MT_HALO), 0, MT_RH - 1);
    double w[10], w2[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) {
      const int rc = mt_clampi(mt_reflect(tx0 + x0 - MT_NQ + i, W) - (tx0 - MT_HALO), 0, MT_RW - 1);
      const float g = G[rr][rc];
      w[i] = (double)g;
      w2[i] = (double)(g * g);
    }
    double s = w[0], s2 = w2[0];
#pragma unroll
    for (int i = 1; i < 7; ++i) { s += w[i]; s2 += w2[i]; }
    rows[0][j][x0] = s;
    rows[1][j][x0] = s2;
#pragma unroll
    for (int o = 1; o < 4; ++o) {
      s = (s + w[o + 6]) - w[o - 1];
      s2 = (s2 + w2[o + 6]) - w2[o - 1];
      rows[0][j][x0 + o] = s;
      rows[1][j][x0 + o] = s2;
    }
  }
  __syncthreads();
  // NIQE columns: thread = (column, MT_CO tile rows)
  const int col = t & (MT_TW - 1), yb = (t / MT_TW) * MT_CO;
  const int px = tx0 + col;
  {
    double s = 0.0, s2 = 0.0;
#pragma unroll
    for (int i = 0; i < 7; ++i) { s += rows[0][yb + i][col]; s2 += rows[1][yb + i][col]; }
#pragma unroll
    for (int o = 0; o < MT_CO; ++o) {
      if (o > 0) {
        s = (s + rows[0][yb + o + 6][col]) - rows[0][yb + o - 1][col];
        s2 = (s2 + rows[1][yb + o + 6][col]) - rows[1][yb + o - 1][col];
      }
      if (ty0 + yb + o < H && px < W) {
        // 49^2 (E[g^2] - mu^2) = 49 s2 - s^2: the three sums are scaled once, when the block writes them
        const double ss = s * s;
        const double var = 49.0 * s2 - ss;
        acc[7] += sqrt(var > 0.0 ? var : 0.0);
        acc[8] += s;
        acc[9] += ss;
      }
    }
  }

  // (3) SSIM, one channel at a time through the same LDS
  if constexpr (PAIRED) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      __syncthreads();  // the previous pass has read PX / PY / rows
#pragma unroll
      for (int k = 0; k < MT_LR; ++k) {
        const int ry = wave + 4 * k;
        if (ry < MT_RH && lane < MT_RW) {
          PX[ry][lane] = xv[k][c];
          PY[ry][lane] = yv[k][c];
        }
      }
      __syncthreads();
      // rows: item = (region row, quad of 4 tile columns); window = region columns x0 .. x0 + 13
      for (int it = t; it < MT_RH * (MT_TW / 4); it += MT_NT) {
        const int ry = it / (MT_TW / 4), x0 = (it % (MT_TW / 4)) * 4;
        double xw[14], yw[14];
#pragma unroll
        for (int i = 0; i < 14; ++i) {
          xw[i] = (double)PX[ry][x0 + i];
          yw[i] = (double)PY[ry][x0 + i];
        }
        double s[5] = {xw[0], yw[0], xw[0] * xw[0], yw[0] * yw[0], xw[0] * yw[0]};
#pragma unroll
        for (int i = 1; i < 11; ++i) {
          s[0] += xw[i];
          s[1] += yw[i];
          s[2] += xw[i] * xw[i];
          s[3] += yw[i] * yw[i];
          s[4] += xw[i] * yw[i];
        }
#pragma unroll
        for (int q = 0; q < 5; ++q) rows[q][ry][x0] = s[q];
#pragma unroll
        for (int o = 1; o < 4; ++o) {
          const double xi = xw[o + 10], yi = yw[o + 10], xo = xw[o - 1], yo = yw[o - 1];
          s[0] = (s[0] + xi) - xo;
          s[1] = (s[1] + yi) - yo;
          s[2] = (s[2] + xi * xi) - xo * xo;
          s[3] = (s[3] + yi * yi) - yo * yo;
          s[4] = (s[4] + xi * yi) - xo * yo;
#pragma unroll
          for (int q = 0; q < 5; ++q) rows[q][ry][x0 + o] = s[q];
        }
      }
      __syncthreads();
      // columns: window = region rows yb .. yb + 10 + MT_CO - 1
      double cs[5][MT_CO];
#pragma unroll
      for (int q = 0; q < 5; ++q) {
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < 11; ++i) s += rows[q][yb + i][col];
        cs[q][0] = s;
#pragma unroll
        for (int o = 1; o < MT_CO; ++o) {
          s = (s + rows[q][yb + o + 10][col]) - rows[q][yb + o - 1][col];
          cs[q][o] = s;
        }
      }
#pragma unroll
      for (int o = 0; o < MT_CO; ++o) {
        if (ty0 + yb + o < H && px < W) {
          // the SSIM quotient with numerator and denominator both scaled by 121^4: with N = 121 and the
          // window sums S, mu = S / N and sigma = S2 / N - mu^2, so 2 mu1 mu2 + C1 = (2 S1 S2 + C1 N^2) / N^2,
          // 2 sigma12 + C2 = (2 (N S12 - S1 S2) + C2 N^2) / N^2, and likewise below: one division, not six
          const double N = 121.0, C1 = (0.01 * 0.01) * (121.0 * 121.0), C2 = (0.03 * 0.03) * (121.0 * 121.0);
          const double p12 = cs[0][o] * cs[1][o];
          const double q = cs[0][o] * cs[0][o] + cs[1][o] * cs[1][o];
          const double num = (2.0 * p12 + C1) * (2.0 * (N * cs[4][o] - p12) + C2);
          const double den = (q + C1) * ((N * (cs[2][o] + cs[3][o]) - q) + C2);
          acc[11 + c] += num / den;
        }
      }
    }
  }

  // block sums in a fixed order: the four waves' lanes through LDS, then wave 0's lanes by butterfly
  // (a butterfly in every wave was 168 ds_bpermute per wave)
  __syncthreads();  // the last pass has read the row sums
  double(*bsum)[MT_NT] = (double(*)[MT_NT])rowsbuf;
#pragma unroll
  for (int k = 0; k < NS; ++k) bsum[k][t] = acc[k];
  __syncthreads();
  if (t < 64) {
    double out = 0.0;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      double v = ((bsum[k][t] + bsum[k][t + 64]) + bsum[k][t + 128]) + bsum[k][t + 192];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      if (t == k) out = v;
    }
    // NIQE: sigma and mu were summed as 49 sigma and 49 mu, mu^2 as 49^2 mu^2
    if (t == 7 || t == 8) out /= 49.0;
    if (t == 9) out /= 49.0 * 49.0;
    if (t < kMetricsNSums) part[((size_t)b * ntiles + tile) * kMetricsNSums + t] = out;
  }
  const int h = wh[0][t] + wh[1][t] + wh[2][t] + wh[3][t];
  if (h) atomicAdd(&hist[(size_t)b * 256 + t], h);
}

__global__ __launch_bounds__(256) void metrics_fin_kernel(const double* __restrict__ part,
                                                          const int* __restrict__ hist_ws,
                                                          double* __restrict__ metrics, double* __restrict__ sums,
                                                          int* __restrict__ hist, int ntiles, int H, int W,
                                                          int paired) {
  __shared__ double red[kMetricsNSums][256];
  __shared__ double s16[kMetricsNSums][16];
  __shared__ double S[kMetricsNSums];
  __shared__ double wsum[4];
  __shared__ long long wtot[4];
  const int t = threadIdx.x, b = blockIdx.x;
  // tile partials in a fixed order that depends on the tile count alone: thread
  // t adds tiles t, t + 256, ... (independent loads), 16 threads per sum add 16
  // of those each, one thread adds the 16
  {
    double a[kMetricsNSums];
#pragma unroll
    for (int k = 0; k < kMetricsNSums; ++k) a[k] = 0.0;
    for (int i = t; i < ntiles; i += 256) {
      const double* p = part + ((size_t)b * ntiles + i) * kMetricsNSums;
#pragma unroll
      for (int k = 0; k < kMetricsNSums; ++k) a[k] += p[k];
    }
#pragma unroll
    for (int k = 0; k < kMetricsNSums; ++k) red[k][t] = a[k];
  }
  const int cnt = hist_ws[(size_t)b * 256 + t];
  if (hist) hist[(size_t)b * 256 + t] = cnt;
  long long wcnt = cnt;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) wcnt += __shfl_xor(wcnt, o, 64);
  if ((t & 63) == 0) wtot[t >> 6] = wcnt;
  __syncthreads();
  const int q = t >> 4, j = t & 15;
  if (q < kMetricsNSums) {
    double a = red[q][16 * j];
    for (int k = 1; k < 16; ++k) a += red[q][16 * j + k];
    s16[q][j] = a;
  }
  // entropy terms: lanes by butterfly, then the four waves in order
  {
    const long long total = ((wtot[0] + wtot[1]) + wtot[2]) + wtot[3];
    const double p = (double)cnt / (double)total;
    double e = cnt > 0 ? p * log2(p) : 0.0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o, 64);
    if ((t & 63) == 0) wsum[t >> 6] = e;
  }
  __syncthreads();
  if (t < kMetricsNSums) {
    double a = s16[t][0];
    for (int k = 1; k < 16; ++k) a += s16[t][k];
    S[t] = a;
  }
  __syncthreads();
  if (t != 0) return;
  const double nan = __builtin_nan("");
  const double hw = (double)H * (double)W, n = 3.0 * hw;
  double* m = metrics + (size_t)b * kMetricsN;
  if (sums) {
    for (int k = 0; k < kMetricsNSums; ++k) sums[(size_t)b * kMetricsNSums + k] = (k >= 10 && !paired) ? nan : S[k];
  }
  const double mean = ((S[0] + S[1]) + S[2]) / n;
  const double var = ((S[3] + S[4]) + S[5]) / n - mean * mean;
  const double contrast = sqrt(var > 0.0 ? var : 0.0);
  const double e = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
  const double mmu = S[8] / hw;
  const double vmu = S[9] / hw - mmu * mmu;
  const double c0 = S[0] / hw, c1 = S[1] / hw, c2 = S[2] / hw;
  const double cm = ((c0 + c1) + c2) / 3.0;
  const double cstd = sqrt((((c0 - cm) * (c0 - cm) + (c1 - cm) * (c1 - cm)) + (c2 - cm) * (c2 - cm)) / 3.0);
  double cscore = 1.0 - fabs(contrast - 0.15) / 0.15;
  cscore = cscore < 0.0 ? 0.0 : (cscore > 1.0 ? 1.0 : cscore);
  double bscore = 1.0 - fabs(mean - 0.5) / 0.5;
  bscore = bscore < 0.0 ? 0.0 : (bscore > 1.0 ? 1.0 : bscore);
  m[0] = mean;
  m[1] = contrast;
  m[2] = -e;
  m[3] = (S[7] / hw) / (sqrt(vmu > 0.0 ? vmu : 0.0) + 1e-8);
  m[4] = S[6] / hw;
  m[5] = (0.3 * (1.0 - cstd) + 0.4 * cscore) + 0.3 * bscore;
  if (paired) {
    const double mse = S[10] / n;
    m[6] = mse;
    m[7] = mse < 1e-10 ? 100.0 : 20.0 * log10(1.0 / sqrt(mse));
    m[8] = ((S[11] / hw + S[12] / hw) + S[13] / hw) / 3.0;
  } else {
    m[6] = m[7] = m[8] = nan;
  }
}

static inline int metrics_tiles(int H, int W) { return cdiv(H, MT_TH) * cdiv(W, MT_TW); }

size_t metrics_ws(int B, int H, int W) {
  return align_up((size_t)B * metrics_tiles(H, W) * kMetricsNSums * sizeof(double), 256) + (size_t)B * 256 * sizeof(int);
}

int launch_metrics(const void* enh, const void* ref, double* metrics, double* sums, int* hist, uint8_t* ws, int B,
                   int H, int W, int dtype, hipStream_t st) {
  const int tiles_x = cdiv(W, MT_TW), ntiles = metrics_tiles(H, W);
  double* part = (double*)ws;
  int* hws = (int*)(ws + align_up((size_t)B * ntiles * kMetricsNSums * sizeof(double), 256));
  UPR_CHECK_HIP(hipMemsetAsync(hws, 0, (size_t)B * 256 * sizeof(int), st));
  // (blockIdx.y carries the image: at most 65535 per launch)
  for (int b0 = 0; b0 < B; b0 += 65535) {
    const int nb = B - b0 < 65535 ? B - b0 : 65535;
    const dim3 grid(ntiles, nb);
    const size_t io = (size_t)b0 * 3 * H * W;
    double* p = part + (size_t)b0 * ntiles * kMetricsNSums;
    int* hp = hws + (size_t)b0 * 256;
    if (dtype == kF16) {
      const half_t* x = (const half_t*)enh + io;
      if (ref)
        hipLaunchKernelGGL((metrics_tile_kernel<half_t, true>), grid, dim3(MT_NT), 0, st, x, (const half_t*)ref + io, p,
                           hp, H, W, tiles_x, ntiles);
      else
        hipLaunchKernelGGL((metrics_tile_kernel<half_t, false>), grid, dim3(MT_NT), 0, st, x, (const half_t*)nullptr, p,
                           hp, H, W, tiles_x, ntiles);
    } else {
      const float* x = (const float*)enh + io;
      if (ref)
        hipLaunchKernelGGL((metrics_tile_kernel<float, true>), grid, dim3(MT_NT), 0, st, x, (const float*)ref + io, p,
                           hp, H, W, tiles_x, ntiles);
      else
        hipLaunchKernelGGL((metrics_tile_kernel<float, false>), grid, dim3(MT_NT), 0, st, x, (const float*)nullptr, p,
                           hp, H, W, tiles_x, ntiles);
    }
    UPR_CHECK_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(metrics_fin_kernel, dim3(B), dim3(256), 0, st, part, hws, metrics, sums, hist, ntiles, H, W,
                     ref ? 1 : 0);
  UPR_CHECK_HIP(hipGetLastError());
  return kOk;
}

}  // namespace upr
