// TotalLoss terms with their gradients for gfx950 (reference
// losses/loss.py:12-753): the pixel terms over one workspace of fp64
// accumulators, texture complexity, MSE, VGG normalisation and the
// frequency term.
// Entries: include/upr_train.h; layout and precision: train_common.h.
#include <cmath>

#include "train_common.h"

namespace upr {

// ---------------------------------------------------------------------------
// TotalLoss pixel terms (loss.py): workspace of fp64 accumulators
// ---------------------------------------------------------------------------
enum {
  LA_COL = 0,      // 3: sum enh_c
  LA_SPA_H = 3, LA_SPA_V = 4,
  LA_SM_H = 5, LA_SM_V = 6,
  LA_TV_H = 7, LA_TV_V = 8,
  LA_GLOW = 9,
  LA_FIXED = 16,   // then per image LA_IMG: [sum illu_c (3), sum r_j (3), sum illu_c*r_j (3x3)]
  LA_IMG = 16,     // (one illumination channel: c = 0 only)
};

struct LossWS {
  double* acc;     // LA_FIXED + LA_IMG * B
  double* patch;   // B * (H/ps) * (W/ps) sums of gray(enh) (ps = exposure patch size)
  double* rowsum;  // B*H   sum_{x<W-1} edge
  double* colsum;  // B*W   sum_{y<H-1} edge
  double* ed;      // 2B    texture 'edge_density': per image sum of |Sobel|, count above threshold
  float* scal;     // finalised scalars for the gradient pass
  // loss module arguments (UprLossParams)
  int ps;          // AdaptiveExposureLoss patch_size
  float base_exp;  // base_target_exposure
  float lam_s, alpha;  // EdgeAwareSmoothnessLoss lambda_val, alpha
  float lam_d;     // IlluminationReflectanceDecouplingLoss lambda_val
  int dynamic;     // TotalLoss use_dynamic_smooth_weight
};

// finalised scalars: 64 + per image LS_IMG
static size_t loss_scal_bytes(int B) { return align_up(sizeof(float) * (64 + 16 * B), 256); }

static LossWS loss_ws(void* ws, int B, int H, int W, int ps) {
  LossWS l;
  char* p = (char*)ws;
  l.acc = (double*)p; p += align_up(sizeof(double) * (LA_FIXED + LA_IMG * B), 256);
  l.patch = (double*)p; p += align_up(sizeof(double) * B * (H / ps) * (W / ps), 256);
  l.rowsum = (double*)p; p += align_up(sizeof(double) * B * H, 256);
  l.colsum = (double*)p; p += align_up(sizeof(double) * B * W, 256);
  l.ed = (double*)p; p += align_up(sizeof(double) * 2 * B, 256);
  l.scal = (float*)p;
  return l;
}
static size_t loss_ws_bytes(int B, int H, int W, int ps) {
  return align_up(sizeof(double) * (LA_FIXED + LA_IMG * B), 256) +
         align_up(sizeof(double) * B * (H / ps) * (W / ps), 256) + align_up(sizeof(double) * B * H, 256) +
         align_up(sizeof(double) * B * W, 256) + align_up(sizeof(double) * 2 * B, 256) + loss_scal_bytes(B);
}

// scalar slots
// per image LS_IMG: covariance [c][j] (9; one illumination channel: [j] = row 0),
// mean differences (3 at +9; one channel: +9 = mean I - mean of the R means),
// illumination means (3 at +12)
enum { LS_T = 0, LS_NPATCH = 1, LS_WS = 2, LS_MU = 3 /*3*/, LS_NH = 6, LS_NV = 7, LS_DEC = 8, LS_IMG = 16 };

__device__ __forceinline__ float gray_at(const float* img, size_t base, int HW, int p) {
  return (img[base + p] + img[base + HW + p] + img[base + 2 * HW + p]) / 3.f;
}

// Sobel edge magnitude of gray(low) with reflect padding (loss.py:110-136)
__device__ float edge_at(const float* low, size_t base, int H, int W, int y, int x) {
  const int HW = H * W;
  float g[3][3];
  for (int dy = -1; dy <= 1; ++dy) {
    int yy = y + dy;
    yy = yy < 0 ? -yy : (yy >= H ? 2 * H - 2 - yy : yy);
    for (int dx = -1; dx <= 1; ++dx) {
      int xx = x + dx;
      xx = xx < 0 ? -xx : (xx >= W ? 2 * W - 2 - xx : xx);
      g[dy + 1][dx + 1] = gray_at(low, base, HW, yy * W + xx);
    }
  }
  // each tap next to its mirror tap, in gy as in gx: on a 2-sample axis the
  // reflect pad makes the two equal and the sum cancels exactly, term by term
  const float gx = -g[0][0] + g[0][2] - 2.f * g[1][0] + 2.f * g[1][2] - g[2][0] + g[2][2];
  const float gy = -g[0][0] + g[2][0] - 2.f * g[0][1] + 2.f * g[2][1] - g[0][2] + g[2][2];
  return sqrtf(gx * gx + gy * gy);
}

template <int CI>
constexpr int loss_nv() { return 10 + CI + 3 + 3 * CI; }  // fixed sums, then sum I_c, sum R_j, sum I_c R_j

// one pixel's pass-1 terms into v; ge = gray(enh), ed = Sobel magnitude of gray(low)
template <int CI>
__device__ __forceinline__ void loss_pixel1(const float* __restrict__ low, const float* __restrict__ enh,
                                            const float* __restrict__ illu, const float* __restrict__ refl, int b,
                                            size_t base, int H, int W, int q, int y, int x,
                                            double (&v)[loss_nv<CI>()], float& ge, float& ed) {
  const int HW = H * W;
  float le[3], ll[3];
  for (int c = 0; c < 3; ++c) { le[c] = enh[base + c * HW + q]; ll[c] = low[base + c * HW + q]; }
  for (int c = 0; c < 3; ++c) v[c] += le[c];
  v[9] += (ll[0] + ll[1] + ll[2]) / 3.f;
  if (x < W - 1) {
    for (int c = 0; c < 3; ++c) {
      const float de = le[c] - enh[base + c * HW + q + 1], dl = ll[c] - low[base + c * HW + q + 1];
      v[3] += (double)(de - dl) * (de - dl);
      v[7] += fabsf(dl);
    }
  }
  if (y < H - 1) {
    for (int c = 0; c < 3; ++c) {
      const float de = le[c] - enh[base + c * HW + q + W], dl = ll[c] - low[base + c * HW + q + W];
      v[4] += (double)(de - dl) * (de - dl);
      v[8] += fabsf(dl);
    }
  }
  float il[CI];
#pragma unroll
  for (int c = 0; c < CI; ++c) {
    il[c] = illu[((size_t)b * CI + c) * HW + q];
    v[10 + c] += il[c];
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float r = refl[base + j * HW + q];
    v[10 + CI + j] += r;
#pragma unroll
    for (int c = 0; c < CI; ++c) v[13 + CI + c * 3 + j] += (double)il[c] * r;
  }
  ge = (le[0] + le[1] + le[2]) / 3.f;
  ed = edge_at(low, base, H, W, y, x);
}

template <int CI>
__device__ __forceinline__ void loss_pass1_flush(double (&v)[loss_nv<CI>()], const LossWS& ws, int b) {
  constexpr int NV = loss_nv<CI>();
  double* dst[NV];
  for (int k = 0; k < 10; ++k) dst[k] = ws.acc + k;
  double* img = ws.acc + LA_FIXED + b * LA_IMG;
  for (int c = 0; c < CI; ++c) dst[10 + c] = img + c;
  for (int j = 0; j < 3; ++j) dst[10 + CI + j] = img + 3 + j;
  for (int k = 0; k < 3 * CI; ++k) dst[13 + CI + k] = img + 6 + k;
  block_sum_atomic<NV>(v, dst);
}

// pass 1, any shape: grid (chunks, B); CI = illumination channels (1 or 3)
template <int CI>
__global__ __launch_bounds__(256) void loss_pass1_kernel(const float* __restrict__ low, const float* __restrict__ enh,
                                                         const float* __restrict__ illu,
                                                         const float* __restrict__ refl, int H, int W, LossWS ws) {
  const int b = blockIdx.y;
  const int HW = H * W;
  const size_t base = (size_t)b * 3 * HW;
  const int per = (HW + gridDim.x - 1) / gridDim.x;
  const int p0 = blockIdx.x * per, p1 = min(HW, p0 + per);
  double v[loss_nv<CI>()] = {};
  const int ps = ws.ps, PH = H / ps, PW = W / ps;
  for (int q = p0 + threadIdx.x; q < p1; q += 256) {
    const int y = q / W, x = q - y * W;
    float ge, ed;
    loss_pixel1<CI>(low, enh, illu, refl, b, base, H, W, q, y, x, v, ge, ed);
    // exposure patches, edge row / column sums (per-pixel atomics on small arrays)
    // F.avg_pool2d(kernel = stride = ps): floor(H/ps) x floor(W/ps) patches, the remainder ignored
    if (y < PH * ps && x < PW * ps) atomicAdd(ws.patch + ((size_t)b * PH + y / ps) * PW + x / ps, (double)ge);
    if (x < W - 1) atomicAdd(ws.rowsum + (size_t)b * H + y, (double)ed);
    if (y < H - 1) atomicAdd(ws.colsum + (size_t)b * W + x, (double)ed);
  }
  loss_pass1_flush<CI>(v, ws, b);
}

// pass 1 on patch-row bands (H, W multiples of ps, ps a power of two <= 64):
// grid (ceil(W / 256), H / ps, B), one column per thread over the band's ps
// rows.  A patch is ps adjacent lanes of one wave (a shuffle sum, stored: each
// patch has one owner), a row's edge sum is a block sum (one atomic per row per
// 256 columns), a column's one atomic per band -- instead of the three fp64
// atomics per pixel of the generic pass (contended 256 / W / H ways; ~0.3 ms
// at 8 x 512 x 512)
template <int CI>
__global__ __launch_bounds__(256) void loss_pass1_band_kernel(const float* __restrict__ low,
                                                              const float* __restrict__ enh,
                                                              const float* __restrict__ illu,
                                                              const float* __restrict__ refl, int H, int W,
                                                              LossWS ws) {
  __shared__ double rowred[64][4];
  const int b = blockIdx.z, band = blockIdx.y, ps = ws.ps;
  const int x = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t base = (size_t)b * 3 * H * W;
  const bool in = x < W;
  double v[loss_nv<CI>()] = {};
  double cpatch = 0.0, ccol = 0.0;
  for (int r = 0; r < ps; ++r) {
    const int y = band * ps + r;
    double red = 0.0;
    if (in) {
      float ge, ed;
      loss_pixel1<CI>(low, enh, illu, refl, b, base, H, W, y * W + x, y, x, v, ge, ed);
      cpatch += (double)ge;
      if (y < H - 1) ccol += (double)ed;
      if (x < W - 1) red = (double)ed;
    }
    for (int o = 32; o > 0; o >>= 1) red += __shfl_xor(red, o);
    if (lane == 0) rowred[r][wave] = red;
  }
  for (int o = ps / 2; o > 0; o >>= 1) cpatch += __shfl_xor(cpatch, o);
  if (in) {
    if ((x & (ps - 1)) == 0) ws.patch[((size_t)b * (H / ps) + band) * (W / ps) + x / ps] = cpatch;
    atomicAdd(ws.colsum + (size_t)b * W + x, ccol);
  }
  __syncthreads();
  if (threadIdx.x < ps) {
    const int t = threadIdx.x;
    atomicAdd(ws.rowsum + (size_t)b * H + band * ps + t, ((rowred[t][0] + rowred[t][1]) + rowred[t][2]) + rowred[t][3]);
  }
  loss_pass1_flush<CI>(v, ws, b);
}

// pass 2: edge-aware smoothness sums (needs the row / column edge means),
// summed over the CI illumination planes (the finaliser divides by CI)
template <int CI>
__global__ __launch_bounds__(256) void loss_pass2_kernel(const float* __restrict__ low, const float* __restrict__ illu,
                                                         int H, int W, LossWS ws) {
  const int b = blockIdx.y;
  const int HW = H * W;
  const size_t base = (size_t)b * 3 * HW;
  const int per = (HW + gridDim.x - 1) / gridDim.x;
  const int p0 = blockIdx.x * per, p1 = min(HW, p0 + per);
  double v[2] = {0.0, 0.0};
  for (int q = p0 + threadIdx.x; q < p1; q += 256) {
    const int y = q / W, x = q - y * W;
    const float* ip = illu + (size_t)b * CI * HW + q;
    if (x < W - 1) {
      float s = 0.f;
      for (int c = 0; c < 3; ++c) s += fabsf(low[base + c * HW + q] - low[base + c * HW + q + 1]);
      const float wh = expf(-ws.lam_s * (s / 3.f));
      const float ef = 1.f + ws.alpha * (float)(ws.rowsum[(size_t)b * H + y] / (W - 1));
#pragma unroll
      for (int c = 0; c < CI; ++c) v[0] += wh * ef * fabsf(ip[c * HW] - ip[c * HW + 1]);
    }
    if (y < H - 1) {
      float s = 0.f;
      for (int c = 0; c < 3; ++c) s += fabsf(low[base + c * HW + q] - low[base + c * HW + q + W]);
      const float wv = expf(-ws.lam_s * (s / 3.f));
      const float ef = 1.f + ws.alpha * (float)(ws.colsum[(size_t)b * W + x] / (H - 1));
#pragma unroll
      for (int c = 0; c < CI; ++c) v[1] += wv * ef * fabsf(ip[c * HW] - ip[c * HW + W]);
    }
  }
  double* dst[2] = {ws.acc + LA_SM_H, ws.acc + LA_SM_V};
  block_sum_atomic<2>(v, dst);
}

// texture complexity 'edge_density' (loss.py:549-577): per image, the share of
// pixels whose Sobel magnitude of gray(low) exceeds 1.5x the image mean.
// mode 0: per-image sum of magnitudes; mode 1: per-image count above threshold
__global__ __launch_bounds__(256) void edge_density_kernel(const float* __restrict__ low, int H, int W, LossWS ws,
                                                           int mode) {
  const int b = blockIdx.y;
  const int HW = H * W;
  const size_t base = (size_t)b * 3 * HW;
  const int per = (HW + gridDim.x - 1) / gridDim.x;
  const int p0 = blockIdx.x * per, p1 = min(HW, p0 + per);
  const float thr = mode ? (float)(ws.ed[b] / HW) * 1.5f : 0.f;
  double v[1] = {0.0};
  for (int q = p0 + threadIdx.x; q < p1; q += 256) {
    const int y = q / W, x = q - y * W;
    const float e = edge_at(low, base, H, W, y, x);
    v[0] += mode ? (e > thr ? 1.0 : 0.0) : (double)e;
  }
  double* dst[1] = {ws.ed + mode * gridDim.y + b};
  block_sum_atomic<1>(v, dst);
}

// calculate_texture_complexity (losses/loss.py:523-583) called on its own, for
// any channel count: img [B][C][H][W] fp32.  grid (chunks, B).
//   method 0 'tv':  acc[b] += sum |x[..,w] - x[..,w+1]|, acc[B+b] += sum |x[h] - x[h+1]|
//   method 1 'edge_density': gray = channel mean (torch.mean dim 1), reflect-
//     padded Sobel magnitude; mode 0 acc[b] += sum of magnitudes, mode 1
//     acc[B+b] += count of magnitudes > 1.5 * fp32 mean
__device__ __forceinline__ float gray_mean_c(const float* img, size_t base, int C, int HW, int q) {
  float s = img[base + q];
  for (int c = 1; c < C; ++c) s += img[base + (size_t)c * HW + q];
  return C > 1 ? s / (float)C : s;
}

__global__ __launch_bounds__(256) void texture_kernel(const float* __restrict__ img, int C, int H, int W, int method,
                                                      int mode, double* __restrict__ acc) {
  const int b = blockIdx.y, B = gridDim.y;
  const int HW = H * W;
  const size_t base = (size_t)b * C * HW;
  const int per = (HW + gridDim.x - 1) / gridDim.x;
  const int p0 = blockIdx.x * per, p1 = min(HW, p0 + per);
  double v[2] = {0.0, 0.0};
  const float thr = (method == 1 && mode == 1) ? (float)(acc[b] / HW) * 1.5f : 0.f;
  for (int q = p0 + threadIdx.x; q < p1; q += 256) {
    const int y = q / W, x = q - y * W;
    if (method == 0) {
      for (int c = 0; c < C; ++c) {
        const float* pl = img + base + (size_t)c * HW;
        const float a = pl[q];
        if (x + 1 < W) v[0] += fabsf(a - pl[q + 1]);
        if (y + 1 < H) v[1] += fabsf(a - pl[q + W]);
      }
    } else {
      float g[3][3];
      for (int dy = -1; dy <= 1; ++dy) {
        int yy = y + dy;
        yy = yy < 0 ? -yy : (yy >= H ? 2 * H - 2 - yy : yy);
        for (int dx = -1; dx <= 1; ++dx) {
          int xx = x + dx;
          xx = xx < 0 ? -xx : (xx >= W ? 2 * W - 2 - xx : xx);
          g[dy + 1][dx + 1] = gray_mean_c(img, base, C, HW, yy * W + xx);
        }
      }
      const float gx = -g[0][0] + g[0][2] - 2.f * g[1][0] + 2.f * g[1][2] - g[2][0] + g[2][2];
      const float gy = -g[0][0] + g[2][0] - 2.f * g[0][1] + 2.f * g[2][1] - g[0][2] + g[2][2];  // as edge_at
      const float e = sqrtf(gx * gx + gy * gy);
      if (mode == 0) v[0] += (double)e;
      else v[1] += e > thr ? 1.0 : 0.0;
    }
  }
  double* dst[2] = {(method == 0 || mode == 0) ? acc + b : nullptr, (method == 0 || mode == 1) ? acc + B + b : nullptr};
  block_sum_atomic<2>(v, dst);
}

__global__ void texture_final_kernel(const double* __restrict__ acc, int B, int C, int H, int W, int method,
                                     float* __restrict__ out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  if (method == 0) {
    // torch.mean per direction (fp32 results), then their fp32 sum
    const float th = (float)(acc[b] / ((double)C * H * (W - 1)));
    const float tv = (float)(acc[B + b] / ((double)C * (H - 1) * W));
    out[b] = th + tv;
  } else {
    out[b] = (float)(acc[B + b] / ((double)H * W));
  }
}

// finalise: one block
__global__ void loss_final_kernel(int B, int H, int W, LossWS ws, float* __restrict__ terms, int texture,
                                  float w_smooth, int CI) {
  __shared__ double ex[256];
  const int HW = H * W;
  const double N = (double)B * HW;
  // adaptive target base + (0.8 - base) * (1 - mean gray(low)) (loss.py:49)
  const double T = ws.base_exp + (0.8 - (double)ws.base_exp) * (1.0 - ws.acc[LA_GLOW] / N);
  const int NP = B * (H / ws.ps) * (W / ws.ps);
  const double parea = (double)ws.ps * ws.ps;
  double e = 0.0;
  for (int k = threadIdx.x; k < NP; k += blockDim.x) e += fabs(ws.patch[k] / parea - T);
  ex[threadIdx.x] = e;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) ex[threadIdx.x] += ex[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const double nh = (double)B * 3 * H * (W - 1), nv = (double)B * 3 * (H - 1) * W;
  const double nh1 = (double)B * H * (W - 1), nv1 = (double)B * (H - 1) * W;
  const double mu0 = ws.acc[0] / N, mu1 = ws.acc[1] / N, mu2 = ws.acc[2] / N;
  const double col = (mu0 - mu1) * (mu0 - mu1) + (mu0 - mu2) * (mu0 - mu2) + (mu1 - mu2) * (mu1 - mu2);
  const double spa = ws.acc[LA_SPA_H] / nh + ws.acc[LA_SPA_V] / nv;
  // smoothness: torch.mean over B x CI x H x (W-1) (loss.py:171-172)
  const double smo = (ws.acc[LA_SM_H] / nh1 + ws.acc[LA_SM_V] / nv1) / CI;
  double tc = ws.acc[LA_TV_H] / nh + ws.acc[LA_TV_V] / nv;
  if (texture == 1) {
    tc = 0.0;
    for (int b = 0; b < B; ++b) tc += ws.ed[B + b] / HW;
    tc /= B;
  }
  double wsm = (double)w_smooth;
  if (ws.dynamic) {  // loss.py:705-720
    wsm = (double)w_smooth * (1.0 - tc * 0.8);
    wsm = wsm < 0.1 ? 0.1 : (wsm > 5.0 ? 5.0 : wsm);
  }
  double frob = 0.0, md = 0.0;
  for (int b = 0; b < B; ++b) {
    const double* a = ws.acc + LA_FIXED + b * LA_IMG;  // [sI_c (3), sR_j (3), sIR_cj (9)]
    float* sc = ws.scal + LS_DEC + b * LS_IMG;
    if (CI == 1) {
      // loss.py:308-312: illumination expanded to 3 rows, NOT centred; each
      // row of the 3x3 covariance is the same cov_j -> Frobenius^2 = 3 sum_j cov_j^2;
      // mean term: mse of the channel means' means (:326-329)
      const double im = a[0] / HW;
      double rmm = 0.0;
      for (int j = 0; j < 3; ++j) {
        const double cov = (a[6 + j] - a[3 + j] * a[0] / HW) / (HW - 1);
        frob += 3.0 * cov * cov;
        sc[j] = (float)cov;
        rmm += a[3 + j] / HW / 3.0;
      }
      md += (im - rmm) * (im - rmm) / B;
      sc[9] = (float)(im - rmm);
      sc[12] = (float)im;
    } else {
      // loss.py:302-304: both centred, cov[c][j] over the 3x3 channel pairs;
      // mean term: F.mse_loss of the [B,3,1] means (:323-324)
      for (int c = 0; c < 3; ++c) {
        for (int j = 0; j < 3; ++j) {
          const double cov = (a[6 + c * 3 + j] - a[c] * a[3 + j] / HW) / (HW - 1);
          frob += cov * cov;
          sc[c * 3 + j] = (float)cov;
        }
        const double d = a[c] / HW - a[3 + c] / HW;
        md += d * d / (3.0 * B);
        sc[9 + c] = (float)d;
        sc[12 + c] = (float)(a[c] / HW);
      }
    }
  }
  const double dec = frob + (double)ws.lam_d * md;
  terms[0] = (float)(ex[0] / NP);
  terms[1] = (float)smo;
  terms[2] = (float)col;
  terms[3] = (float)spa;
  terms[4] = (float)dec;
  terms[8] = (float)wsm;
  ws.scal[LS_T] = (float)T;
  ws.scal[LS_NPATCH] = (float)NP;
  ws.scal[LS_WS] = (float)wsm;
  ws.scal[LS_MU + 0] = (float)mu0;
  ws.scal[LS_MU + 1] = (float)mu1;
  ws.scal[LS_MU + 2] = (float)mu2;
}

// gradient pass: one thread per pixel, overwrites g_enh / g_illu / g_refl
template <int CI>
__global__ __launch_bounds__(256) void loss_grad_kernel(const float* __restrict__ low, const float* __restrict__ enh,
                                                        const float* __restrict__ illu,
                                                        const float* __restrict__ refl, int B, int H, int W,
                                                        LossWS ws, float* __restrict__ g_enh,
                                                        float* __restrict__ g_illu, float* __restrict__ g_refl,
                                                        float w_exp, float w_col, float w_spa, float w_dec) {
  const int HW = H * W;
  const long long n = (long long)B * HW;
  const float T = ws.scal[LS_T];
  const float NP = ws.scal[LS_NPATCH];
  const float wsm = ws.scal[LS_WS];
  const float mu0 = ws.scal[LS_MU], mu1 = ws.scal[LS_MU + 1], mu2 = ws.scal[LS_MU + 2];
  const float N = (float)n;
  const float dcol[3] = {2.f * (mu0 - mu1) + 2.f * (mu0 - mu2), -2.f * (mu0 - mu1) + 2.f * (mu1 - mu2),
                         -2.f * (mu0 - mu2) - 2.f * (mu1 - mu2)};
  const float nh = (float)B * 3 * H * (W - 1), nv = (float)B * 3 * (H - 1) * W;
  const float nh1 = (float)B * H * (W - 1), nv1 = (float)B * (H - 1) * W;
  const int ps = ws.ps, PH = H / ps, PW = W / ps;
  const float parea = (float)(ps * ps);
  GSTRIDE(i, n) {
    const int b = (int)(i / HW), q = (int)(i - (long long)b * HW);
    const int y = q / W, x = q - y * W;
    const size_t base = (size_t)b * 3 * HW;
    // exposure: sign(P - T) / NP / ps^2 / 3 (pixels outside the pooled area: 0)
    float gexp = 0.f;
    if (y < PH * ps && x < PW * ps) {
      const float P = (float)(ws.patch[((size_t)b * PH + y / ps) * PW + x / ps] / parea);
      const float dp = P - T;
      gexp = w_exp * (dp > 0.f ? 1.f : (dp < 0.f ? -1.f : 0.f)) / NP / parea / 3.f;
    }
    for (int c = 0; c < 3; ++c) {
      const size_t k = base + c * HW + q;
      float g = gexp + w_col * dcol[c] / N;
      // spatial: d/de of mean((De - Dl)^2), horizontal and vertical
      const float e0 = enh[k], l0 = low[k];
      if (x < W - 1) g += w_spa * 2.f * ((e0 - enh[k + 1]) - (l0 - low[k + 1])) / nh;
      if (x > 0) g -= w_spa * 2.f * ((enh[k - 1] - e0) - (low[k - 1] - l0)) / nh;
      if (y < H - 1) g += w_spa * 2.f * ((e0 - enh[k + W]) - (l0 - low[k + W])) / nv;
      if (y > 0) g -= w_spa * 2.f * ((enh[k - W] - e0) - (low[k - W] - l0)) / nv;
      g_enh[k] = g;
    }
    // smoothness on each illumination plane (weight wsm; mean over CI planes)
    auto sgn = [](float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); };
    auto wgt = [&](int qa, int qb) {
      float s = 0.f;
      for (int c = 0; c < 3; ++c) s += fabsf(low[base + c * HW + qa] - low[base + c * HW + qb]);
      return expf(-ws.lam_s * (s / 3.f));
    };
    const float efh = 1.f + ws.alpha * (float)(ws.rowsum[(size_t)b * H + y] / (W - 1));
    const float efv = 1.f + ws.alpha * (float)(ws.colsum[(size_t)b * W + x] / (H - 1));
    const float wr = x < W - 1 ? wgt(q, q + 1) * efh : 0.f, wl = x > 0 ? wgt(q - 1, q) * efh : 0.f;
    const float wd = y < H - 1 ? wgt(q, q + W) * efv : 0.f, wu = y > 0 ? wgt(q - W, q) * efv : 0.f;
    const float* sc = ws.scal + LS_DEC + b * LS_IMG;
    const double* a = ws.acc + LA_FIXED + b * LA_IMG;
    const float inv = 1.f / (float)(HW - 1);
    float il[CI], r[3], rm[3];
#pragma unroll
    for (int c = 0; c < CI; ++c) il[c] = illu[((size_t)b * CI + c) * HW + q];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      r[j] = refl[base + j * HW + q];
      rm[j] = (float)(a[3 + j] / HW);
    }
#pragma unroll
    for (int c = 0; c < CI; ++c) {
      const size_t ii = ((size_t)b * CI + c) * HW + q;
      float gi = 0.f;
      if (x < W - 1) gi += wr * sgn(il[c] - illu[ii + 1]) / nh1;
      if (x > 0) gi -= wl * sgn(illu[ii - 1] - il[c]) / nh1;
      if (y < H - 1) gi += wd * sgn(il[c] - illu[ii + W]) / nv1;
      if (y > 0) gi -= wu * sgn(illu[ii - W] - il[c]) / nv1;
      gi *= wsm / CI;
      float gd = 0.f;
      if (CI == 1) {
        // 3 * sum_j cov_j^2 (uncentred I) + lam_d (imean - mean_j rmean_j)^2 / B
#pragma unroll
        for (int j = 0; j < 3; ++j) gd += 6.f * sc[j] * (r[j] - rm[j]) * inv;
        gd += ws.lam_d * 2.f * sc[9] / ((float)B * HW);
      } else {
        // sum_cj cov_cj^2 (centred) + lam_d sum_c (imean_c - rmean_c)^2 / (3B)
#pragma unroll
        for (int j = 0; j < 3; ++j) gd += 2.f * sc[c * 3 + j] * (r[j] - rm[j]) * inv;
        gd += ws.lam_d * 2.f * sc[9 + c] / (3.f * B * HW);
      }
      g_illu[ii] = gi + w_dec * gd;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      float g;
      if (CI == 1) {
        g = 6.f * sc[j] * (il[0] - sc[12]) * inv - ws.lam_d * 2.f * sc[9] / (B * 3.f * HW);
      } else {
        g = 0.f;
#pragma unroll
        for (int c = 0; c < CI; ++c) g += 2.f * sc[c * 3 + j] * (il[c] - sc[12 + c]) * inv;
        g -= ws.lam_d * 2.f * sc[9 + j] / (3.f * B * HW);
      }
      g_refl[base + j * HW + q] = w_dec * g;
    }
  }
}

__global__ void loss_total_kernel(float* t, float we, float wc, float wsp, float wd, float wp, float wf) {
  if (threadIdx.x == 0)
    t[7] = we * t[0] + t[8] * t[1] + wc * t[2] + wsp * t[3] + wd * t[4] + wp * t[5] + wf * t[6];
}

__global__ __launch_bounds__(256) void mse_kernel(const float* __restrict__ a, const float* __restrict__ b, long long n,
                                                  double* acc, float* g, float scale) {
  double v[1] = {0.0};
  GSTRIDE(i, n) {
    const float d = a[i] - b[i];
    v[0] += (double)d * d;
    if (g) g[i] = scale * 2.f * d;
  }
  v[0] /= (double)n;
  double* dst[1] = {acc};
  block_sum_atomic<1>(v, dst);
}

// the same over two fp16 tensors (the frozen VGG's features under autocast,
// which exist in fp16 only: the reference's mse_loss promotes them to fp32),
// 4 elements per thread
__global__ __launch_bounds__(256) void mse16_kernel(const half_t* __restrict__ a, const half_t* __restrict__ b,
                                                    long long n4, long long n, double* acc, float* g, float scale) {
  typedef _Float16 h4 __attribute__((ext_vector_type(4)));
  double v[1] = {0.0};
  GSTRIDE(i, n4) {
    const h4 x = *(const h4*)(a + 4 * i), y = *(const h4*)(b + 4 * i);
    float d[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      d[k] = (float)x[k] - (float)y[k];
      v[0] += (double)d[k] * d[k];
    }
    if (g) *(float4*)(g + 4 * i) = make_float4(scale * 2.f * d[0], scale * 2.f * d[1], scale * 2.f * d[2], scale * 2.f * d[3]);
  }
  v[0] /= (double)n;
  double* dst[1] = {acc};
  block_sum_atomic<1>(v, dst);
}

__constant__ float kVggMean[3] = {0.485f, 0.456f, 0.406f};
__constant__ float kVggStd[3] = {0.229f, 0.224f, 0.225f};

__global__ void vgg_norm_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int HW) {
  const long long n = (long long)B * HW;
  GSTRIDE(i, n) {
    const int b = (int)(i / HW), p = (int)(i - (long long)b * HW);
    for (int c = 0; c < 3; ++c) y[i * 3 + c] = (x[((size_t)b * 3 + c) * HW + p] - kVggMean[c]) / kVggStd[c];
  }
}

__global__ void vgg_norm_bwd_kernel(const float* __restrict__ gy, float* __restrict__ gx, int B, int HW) {
  const long long n = (long long)B * HW;
  GSTRIDE(i, n) {
    const int b = (int)(i / HW), p = (int)(i - (long long)b * HW);
    for (int c = 0; c < 3; ++c) gx[((size_t)b * 3 + c) * HW + p] += gy[i * 3 + c] / kVggStd[c];
  }
}

__global__ __launch_bounds__(256) void freq_kernel(const float2* __restrict__ ze, const float2* __restrict__ zl, int BC,
                                                   int H, int W, double* acc, float2* G, float scale, float w_high,
                                                   float w_low) {
  const long long n = (long long)BC * H * W;
  const int ch = H / 2, cw = W / 2, rad = min(H, W) / 4;
  double v[1] = {0.0};
  GSTRIDE(i, n) {
    const int q = (int)(i % ((long long)H * W));
    const int y = q / W, x = q - y * W;
    const float dist = sqrtf((float)((x - cw) * (x - cw)) + (float)((y - ch) * (y - ch)));
    const float w = dist <= (float)rad ? w_low : w_high;
    const float2 a = ze[i], c = zl[i];
    const float me = sqrtf(a.x * a.x + a.y * a.y), ml = sqrtf(c.x * c.x + c.y * c.y);
    const float d = me - ml;
    v[0] += (double)w * d * d;
    if (G) {
      const float k = me > 0.f ? scale * 2.f * w * d / me : 0.f;
      G[i] = make_float2(k * a.x, k * a.y);
    }
  }
  double* dst[1] = {acc};
  block_sum_atomic<1>(v, dst);
}

__global__ void add_real_kernel(const float2* __restrict__ z, float* g, long long n, float scale) {
  GSTRIDE(i, n) g[i] += scale * z[i].x;
}

__global__ void scale_acc_kernel(const double* __restrict__ acc, int n, float scale, float* out) {
  const int i = threadIdx.x;
  if (i < n) out[i] = (float)(acc[i] * scale);
}

static const UprLossParams kLossDefaults = {16, 0.6f, 10.f, 1.f, 0.1f, 1.f, 0.5f, 1, 1};

}  // namespace upr

using namespace upr;

extern "C" {

size_t upr_t_loss_workspace(int B, int H, int W) { return upr_t_loss_workspace_p(B, H, W, 16); }

size_t upr_t_loss_workspace_p(int B, int H, int W, int patch) {
  if (B <= 0 || patch <= 0 || H < patch || W < patch || H < 2 || W < 2) return 0;
  return loss_ws_bytes(B, H, W, patch);
}

int upr_t_loss_pixel(const float* low, const float* enh, const float* illu, const float* refl, int B, int H, int W,
                     void* ws, float* terms, float* g_enh, float* g_illu, float* g_refl, int grads, float w_exp,
                     float w_col, float w_spa, float w_dec, float w_smooth, int texture, void* stream) {
  if (H % 16 || W % 16) return UPR_ERR_SHAPE;
  return upr_t_loss_pixel_p(low, enh, illu, refl, B, H, W, ws, terms, g_enh, g_illu, g_refl, grads, w_exp, w_col,
                            w_spa, w_dec, w_smooth, texture, &kLossDefaults, stream);
}

int upr_t_loss_pixel_p(const float* low, const float* enh, const float* illu, const float* refl, int B, int H, int W,
                       void* ws, float* terms, float* g_enh, float* g_illu, float* g_refl, int grads, float w_exp,
                       float w_col, float w_spa, float w_dec, float w_smooth, int texture,
                       const UprLossParams* prm, void* stream) {
  if (!low || !enh || !illu || !refl || !ws || !terms || !prm || B <= 0) return UPR_ERR_ARG;
  if (texture != 0 && texture != 1) return UPR_ERR_ARG;
  if (prm->patch <= 0 || H < prm->patch || W < prm->patch || H < 2 || W < 2) return UPR_ERR_SHAPE;
  if (grads && (!g_enh || !g_illu || !g_refl)) return UPR_ERR_ARG;
  const int CI = prm->illu_channels == 0 ? 1 : prm->illu_channels;
  if (CI != 1 && CI != 3) return UPR_ERR_UNSUPPORTED;
  hipStream_t st = ST(stream);
  const size_t zero_bytes = loss_ws_bytes(B, H, W, prm->patch) - loss_scal_bytes(B);
  UPR_CHECK_HIP(hipMemsetAsync(ws, 0, zero_bytes, st));
  LossWS l = loss_ws(ws, B, H, W, prm->patch);
  l.ps = prm->patch;
  l.base_exp = prm->base_exposure;
  l.lam_s = prm->smooth_lambda;
  l.alpha = prm->smooth_alpha;
  l.lam_d = prm->decouple_lambda;
  l.dynamic = prm->dynamic_smooth ? 1 : 0;
  int chunks = (H * W) / 4096;
  chunks = chunks < 1 ? 1 : (chunks > 128 ? 128 : chunks);
  const int ps = l.ps;
  const bool banded = ps <= 64 && (ps & (ps - 1)) == 0 && H % ps == 0 && W % ps == 0;
  const dim3 bgrid((W + 255) / 256, H / ps, B);
  if (CI == 1) {
    if (banded) hipLaunchKernelGGL(loss_pass1_band_kernel<1>, bgrid, dim3(256), 0, st, low, enh, illu, refl, H, W, l);
    else hipLaunchKernelGGL(loss_pass1_kernel<1>, dim3(chunks, B), dim3(256), 0, st, low, enh, illu, refl, H, W, l);
    UPR_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(loss_pass2_kernel<1>, dim3(chunks, B), dim3(256), 0, st, low, illu, H, W, l);
  } else {
    if (banded) hipLaunchKernelGGL(loss_pass1_band_kernel<3>, bgrid, dim3(256), 0, st, low, enh, illu, refl, H, W, l);
    else hipLaunchKernelGGL(loss_pass1_kernel<3>, dim3(chunks, B), dim3(256), 0, st, low, enh, illu, refl, H, W, l);
    UPR_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(loss_pass2_kernel<3>, dim3(chunks, B), dim3(256), 0, st, low, illu, H, W, l);
  }
  UPR_CHECK_HIP(hipGetLastError());
  if (texture == 1 && l.dynamic) {
    for (int mode = 0; mode < 2; ++mode) {
      hipLaunchKernelGGL(edge_density_kernel, dim3(chunks, B), dim3(256), 0, st, low, H, W, l, mode);
      UPR_CHECK_HIP(hipGetLastError());
    }
  }
  hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(256), 0, st, B, H, W, l, terms, texture, w_smooth, CI);
  UPR_CHECK_HIP(hipGetLastError());
  if (grads) {
    if (CI == 1)
      hipLaunchKernelGGL(loss_grad_kernel<1>, dim3(grid_for((long long)B * H * W)), dim3(256), 0, st, low, enh, illu,
                         refl, B, H, W, l, g_enh, g_illu, g_refl, w_exp, w_col, w_spa, w_dec);
    else
      hipLaunchKernelGGL(loss_grad_kernel<3>, dim3(grid_for((long long)B * H * W)), dim3(256), 0, st, low, enh, illu,
                         refl, B, H, W, l, g_enh, g_illu, g_refl, w_exp, w_col, w_spa, w_dec);
  }
  LAUNCH_CHECK();
}

int upr_t_texture_complexity(const float* img, int B, int C, int H, int W, int method, double* acc, float* out,
                             void* stream) {
  if (!img || !acc || !out || B <= 0 || C <= 0 || (method != 0 && method != 1)) return UPR_ERR_ARG;
  if (H < 2 || W < 2) return UPR_ERR_SHAPE;  // a finite difference / a reflect pad needs two samples per axis
  hipStream_t st = ST(stream);
  UPR_CHECK_HIP(hipMemsetAsync(acc, 0, sizeof(double) * 2 * B, st));
  int chunks = (H * W) / 4096;
  chunks = chunks < 1 ? 1 : (chunks > 128 ? 128 : chunks);
  for (int mode = 0; mode < (method == 1 ? 2 : 1); ++mode) {
    hipLaunchKernelGGL(texture_kernel, dim3(chunks, B), dim3(256), 0, st, img, C, H, W, method, mode, acc);
    UPR_CHECK_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(texture_final_kernel, dim3((B + 63) / 64), dim3(64), 0, st, acc, B, C, H, W, method, out);
  LAUNCH_CHECK();
}

int upr_t_loss_total(float* terms, float w_exp, float w_col, float w_spa, float w_dec, float w_per, float w_freq,
                     void* stream) {
  if (!terms) return UPR_ERR_ARG;
  hipLaunchKernelGGL(loss_total_kernel, dim3(1), dim3(64), 0, ST(stream), terms, w_exp, w_col, w_spa, w_dec, w_per,
                     w_freq);
  LAUNCH_CHECK();
}

int upr_t_mse16(const void* a16, const void* b16, size_t n, double* acc, float* g, float scale, void* stream) {
  if (!a16 || !b16 || !acc) return UPR_ERR_ARG;
  if (n % 4 || ((uintptr_t)a16 | (uintptr_t)b16) % 8 || (uintptr_t)g % 16) return UPR_ERR_UNSUPPORTED;
  if (n == 0) return UPR_OK;
  const long long n4 = (long long)(n / 4);
  hipLaunchKernelGGL(mse16_kernel, dim3(grid_for(n4, 256, 4096)), dim3(256), 0, ST(stream), (const half_t*)a16,
                     (const half_t*)b16, n4, (long long)n, acc, g, scale);
  LAUNCH_CHECK();
}

int upr_t_mse(const float* a, const float* b, size_t n, double* acc, float* g, float scale, void* stream) {
  if (!a || !b || !acc) return UPR_ERR_ARG;
  if (n == 0) return UPR_OK;  // the mean of nothing: acc keeps its value (0 / 0 would poison it)
  hipLaunchKernelGGL(mse_kernel, dim3(grid_for((long long)n, 256, 4096)), dim3(256), 0, ST(stream), a, b,
                     (long long)n, acc, g, scale);
  LAUNCH_CHECK();
}

int upr_t_vgg_norm(const float* x, float* y, int B, int H, int W, void* stream) {
  if (!x || !y) return UPR_ERR_ARG;
  hipLaunchKernelGGL(vgg_norm_kernel, dim3(grid_for((long long)B * H * W)), dim3(256), 0, ST(stream), x, y, B, H * W);
  LAUNCH_CHECK();
}

int upr_t_vgg_norm_bwd(const float* g_y, float* g_x, int B, int H, int W, void* stream) {
  if (!g_y || !g_x) return UPR_ERR_ARG;
  hipLaunchKernelGGL(vgg_norm_bwd_kernel, dim3(grid_for((long long)B * H * W)), dim3(256), 0, ST(stream), g_y, g_x, B,
                     H * W);
  LAUNCH_CHECK();
}

int upr_t_freq(const float* Ze, const float* Zl, int BC, int H, int W, double* acc, float* G, float scale,
               void* stream) {
  return upr_t_freq_p(Ze, Zl, BC, H, W, acc, G, scale, 1.f, 0.5f, stream);
}

int upr_t_freq_p(const float* Ze, const float* Zl, int BC, int H, int W, double* acc, float* G, float scale,
                 float w_high, float w_low, void* stream) {
  if (!Ze || !Zl || !acc) return UPR_ERR_ARG;
  hipLaunchKernelGGL(freq_kernel, dim3(grid_for((long long)BC * H * W, 256, 4096)), dim3(256), 0, ST(stream),
                     (const float2*)Ze, (const float2*)Zl, BC, H, W, acc, (float2*)G, scale, w_high, w_low);
  LAUNCH_CHECK();
}

int upr_t_add_real(const float* z, float* g, size_t n, float scale, void* stream) {
  if (!z || !g) return UPR_ERR_ARG;
  hipLaunchKernelGGL(add_real_kernel, dim3(grid_for((long long)n)), dim3(256), 0, ST(stream), (const float2*)z, g,
                     (long long)n, scale);
  LAUNCH_CHECK();
}

int upr_t_scale_acc(const double* acc, int n, float scale, float* out, void* stream) {
  if (!acc || !out || n <= 0 || n > 256) return UPR_ERR_ARG;
  hipLaunchKernelGGL(scale_acc_kernel, dim3(1), dim3(256), 0, ST(stream), acc, n, scale, out);
  LAUNCH_CHECK();
}

}  // extern "C"
